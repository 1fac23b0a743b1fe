#!/usr/bin/env python3
"""Times linear_model.LogisticRegression / linear_model.grid_search_cv on the GPU beside scikit-learn on the host.

    python tools/bench_logreg.py [--out FILE] [--no-sklearn] [--n N] [--tol T]

Shape: the reference's classifier grid -- n = 8000 SMOTE-balanced rows of d = 100 PCA features, float64, C in {0.1, 1, 10}, penalty l2,
max_iter = 1000, five stratified folds -- on seeded two-class data (y uniform, X = randn + 0.5 y on the first three features).  Steps:

* round: the time of one solver round (row pass, weighted Gram matrix, step) over all n rows, C = 1, by HIP events over a call of 8
  rounds that no problem finishes within (max_iter and tol out of reach), median of 5 calls: one problem alone and 16 side by side; and
  the wall time of a host read of the done flags -- the two figures linear_model.ROUNDS_PER_SYNC is sized by;
* grid: linear_model.grid_search_cv over the grid, wall time, with the iteration count of the refit;
* sklearn_grid: GridSearchCV(LogisticRegression(max_iter=1000), grid, cv=5, scoring='f1') on the host's CPUs, one job, wall time.

Every GPU step runs in a child process of its own under a time limit; after a step that fails or runs out of time nothing more is
started on the GPU.  Nothing outside this repository is read.  Prints one JSON line per step.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GRID = {"C": [0.1, 1, 10], "penalty": ["l2"]}
LIMIT_S = {"round": 120, "grid": 180}
ROUNDS = 8


def synth(n, d=100, sep=0.5, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    y = np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0)
    X = rs.randn(n, d)
    X[:, :3] += sep * y[:, None]
    return X, y


def step_round(n):
    import numpy as np
    import torch
    from bbbp_amd import _dense, _lib
    from bbbp_amd import linear_model as lm
    X, y = synth(n)
    dev = torch.device("cuda:0")
    Xd = torch.from_numpy(X).to(dev)
    td = torch.from_numpy(np.where(y > 0, 1.0, 0.0)).to(dev)
    L = _lib.lib()
    res = {"step": "round", "n": n, "d": X.shape[1], "rounds_per_call": ROUNDS}
    for name, count in (("alone", 1), ("sixteen_side_by_side", 16)):
        times = []
        for rep in range(6):                                  # the first call is the warm-up
            # a tolerance out of reach and no iteration limit in range: every round of the call evaluates, factors and solves
            problems = [lm._Problem(Xd, td, 1.0 + 0.01 * q, 1e-300, 1 << 30, True) for q in range(count)]
            arr = (_lib.LogregProblem * count)(*[p.desc for p in problems])
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(L.bbbp_logreg_rounds(_dense.stream(), arr, count, ROUNDS), "bbbp_logreg_rounds")
            b.record()
            torch.cuda.synchronize()
            if rep:
                times.append(a.elapsed_time(b) * 1e3 / ROUNDS)
            done = [int(p.flags[2].item()) for p in problems]
        res[f"us_per_round_{name}"] = sorted(times)[2]
        res[f"done_{name}"] = sum(done)
    reads = []
    for _ in range(20):
        t0 = time.perf_counter()
        torch.stack([p.flags for p in problems]).cpu()
        reads.append((time.perf_counter() - t0) * 1e6)
    res["us_per_flag_read_16"] = sorted(reads)[10]
    return res


def step_grid(n, tol):
    import torch
    from bbbp_amd import linear_model as lm
    X, y = synth(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lm.LogisticRegression(max_iter=3).fit(X[:500], y[:500])                      # load the library, warm the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best, scores, fitted = lm.grid_search_cv(X, y, GRID, cv=5, tol=tol, max_iter=1000)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"step": "grid", "n": n, "d": X.shape[1], "tol": tol, "grid_search_cv_s": dt, "best": best, "scores": scores,
            "refit_iterations": int(fitted.n_iter_[0]), "rounds_per_sync": lm.ROUNDS_PER_SYNC}


def sklearn_grid(n, tol):
    from sklearn.linear_model import LogisticRegression
    from sklearn.model_selection import GridSearchCV
    X, y = synth(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        sk = GridSearchCV(LogisticRegression(max_iter=1000, tol=tol), GRID, cv=5, scoring="f1").fit(X, y)
        dt = time.perf_counter() - t0
    return {"step": "sklearn_grid", "n": n, "d": X.shape[1], "tol": tol, "grid_search_cv_s": dt, "best": sk.best_params_,
            "scores": [float(v) for v in sk.cv_results_["mean_test_score"]], "host_cpus": os.cpu_count(), "n_jobs": 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--n", type=int, default=8000)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--step", help=argparse.SUPPRESS)                 # child mode: run one GPU step and print its JSON line
    a = ap.parse_args()
    if a.n < 100 or not a.tol > 0:
        ap.error("--n must be at least 100 and --tol positive")
    if a.step:
        res = step_round(a.n) if a.step == "round" else step_grid(a.n, a.tol)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    lines = []
    rc = 0
    for name in ("round", "grid"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(a.n), "--tol", repr(a.tol)],
                               capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"[bench_logreg] {name}: no result within {LIMIT_S[name]} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_logreg] {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
            break
        lines.append(json.loads(got[-1]))
        print(got[-1], flush=True)
    if rc == 0 and not a.no_sklearn:
        row = sklearn_grid(a.n, a.tol)
        lines.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
