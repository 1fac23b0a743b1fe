#!/usr/bin/env python3
"""Times svm.SVR / svm.fit_svr_folds on the GPU beside scikit-learn on the host.

    python tools/bench_svr.py [--out FILE] [--no-sklearn] [--rows N] [--d D]

Shape: the SVR of the reference's regression stack (multi_input_data_regression_opt_transformer_cnn_opt_more.py:117-149) --
SVR(kernel='rbf', C=1.0, epsilon=0.1) on each of KFold(5, shuffle=True, random_state=42) -- on seeded data of --rows rows (default 1062, so
a fold trains on about 850) and --d features (default 100; the solver's time does not depend on d), float64:
X = randn, t = X w + sin(2 X[:, 0]) + 0.3 randn.  Steps:

* iteration: microseconds per solver iteration, from the wall time of one launch of up to 2000 iterations (median of three) (C = 10 and tol = 1e-12 so that
  the problem does not converge first; the launch and the host's read of the flags are included): bbbp_svr_smo at n = 850 (one base row per
  thread, state in registers), the same five side by side, n = 4096 (four rows per thread), n = 8000 (state in global memory: the
  classification solver's scheme run over 2n variables); and bbbp_svm_smo, the classification solver, at n = 1700 and n = 8000 on the
  labels t > median(t) for comparison;
* folds: the reference's five-fold job: svm.fit_svr_folds (five problems side by side, matrices included) and five SVR.fit one after the
  other, wall time behind a device synchronise (median of three after a warm-up call) and iteration counts;
* sklearn_folds: sklearn.svm.SVR on the same five folds on the host's CPU, one job, wall time.

Every GPU step runs in a child process of its own under a time limit; after a step that fails or runs out of time nothing more is started
on the GPU.  Nothing outside this repository is read.  Prints one JSON line per step.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT_S = {"iteration": 180, "folds": 180}
PARAMS = dict(kernel="rbf", C=1.0, epsilon=0.1)


def synth(n, d, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    X = rs.randn(n, d)
    w = rs.randn(d) / np.sqrt(d)
    return X, X @ w + np.sin(2.0 * X[:, 0]) + 0.3 * rs.randn(n)


def _folds(n):
    from sklearn.model_selection import KFold
    import numpy as np
    return list(KFold(n_splits=5, shuffle=True, random_state=42).split(np.zeros((n, 1))))


def step_iteration(d):
    import numpy as np
    import torch
    from bbbp_amd import svm
    dev = torch.device("cuda:0")
    res = {"step": "iteration", "d": d, "iters_per_launch": 2000}

    def timed(make, solve, name):
        solve(make(), max_iter=50)                                               # warm-up
        per = []
        for _ in range(3):                                                       # the same launch three times: the median
            problems = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = solve(problems, max_iter=2000, iters_per_launch=2000)
            dt = time.perf_counter() - t0
            ran = max(it for it, _ in out)
            per.append(dt * 1e6 / max(ran, 1))
        res[f"us_per_iteration_{name}"] = sorted(per)[1]
        res[f"us_per_iteration_{name}_all"] = per
        res[f"iterations_{name}"] = ran

    for n in (850, 4096, 8000, 1700):
        X, t = synth(n, d)
        Xd = torch.from_numpy(X).to(dev)
        K = svm.kernel_matrix(Xd, "rbf", svm._resolve_gamma("scale", Xd))[0]
        td = torch.from_numpy(t).to(dev)
        yd = torch.from_numpy(np.where(t > np.median(t), 1.0, -1.0)).to(dev)
        if n != 1700:
            timed(lambda: [svm._SvrProblem(K, td, 10.0, 0.1, 1e-12)], svm._solve_svr, f"svr_n{n}")
        if n == 850:
            timed(lambda: [svm._SvrProblem(K, td, 10.0, 0.1 + 0.01 * q, 1e-12) for q in range(5)], svm._solve_svr, "svr_n850_five_side_by_side")
        if n in (1700, 8000):
            timed(lambda: [svm._Problem(K, yd, 10.0, 1e-12)], svm._solve, f"svc_n{n}")
        del K
    return res


def step_folds(rows, d):
    import torch
    from bbbp_amd import svm
    X, t = synth(rows, d)
    folds = _folds(rows)

    def median_of_three(f):
        f()                                                                      # warm-up: every shape the timed calls use
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return out, sorted(times)[1], times

    models, together, together_all = median_of_three(lambda: svm.fit_svr_folds(X, t, folds, **PARAMS))
    singles, alone, alone_all = median_of_three(lambda: [svm.SVR(**PARAMS).fit(X[tr], t[tr]) for tr, _ in folds])
    preds, predict, _ = median_of_three(lambda: [m.predict(X[te]) for m, (_, te) in zip(models, folds)])
    return {"step": "folds", "rows": rows, "d": d, "train_rows": [len(tr) for tr, _ in folds], "fit_svr_folds_s": together, "fit_svr_folds_s_all": together_all,
            "five_single_fits_s": alone, "five_single_fits_s_all": alone_all,
            "predict_five_folds_s": predict, "iterations": [m.n_iter_ for m in models], "iterations_single": [m.n_iter_ for m in singles],
            "support_vectors": [len(m.support_) for m in models], "held_out_rows": sum(len(p) for p in preds), "iters_per_launch": svm.SVR_ITERS_PER_LAUNCH}


def sklearn_folds(rows, d):
    from sklearn.svm import SVR
    X, t = synth(rows, d)
    folds = _folds(rows)
    t0 = time.perf_counter()
    fits = [SVR(**PARAMS).fit(X[tr], t[tr]) for tr, _ in folds]
    fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    for m, (_, te) in zip(fits, folds):
        m.predict(X[te])
    return {"step": "sklearn_folds", "rows": rows, "d": d, "five_fits_s": fit, "predict_five_folds_s": time.perf_counter() - t0,
            "iterations": [int(m.n_iter_) for m in fits], "host_cpus": os.cpu_count(), "n_jobs": 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--rows", type=int, default=1062)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--step", help=argparse.SUPPRESS)                 # child mode: run one GPU step and print its JSON line
    a = ap.parse_args()
    if a.rows < 100 or a.d < 1:
        ap.error("--rows must be at least 100 and --d positive")
    if a.step:
        res = step_iteration(a.d) if a.step == "iteration" else step_folds(a.rows, a.d)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    lines = []
    rc = 0
    for name in ("iteration", "folds"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--rows", str(a.rows), "--d", str(a.d)],
                               capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"[bench_svr] {name}: no result within {LIMIT_S[name]} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_svr] {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
            break
        lines.append(json.loads(got[-1]))
        print(got[-1], flush=True)
    if rc == 0 and not a.no_sklearn:
        row = sklearn_folds(a.rows, a.d)
        lines.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
