#!/usr/bin/env python3
"""Times svm.SVC / svm.grid_search_cv on the GPU beside scikit-learn on the host.

    python tools/bench_svc.py [--out FILE] [--no-sklearn] [--n N] [--max-iter I]

Shape: the reference's classifier grid -- n = 8000 SMOTE-balanced rows of d = 100 PCA features, float64, C in {0.1, 1, 10} x kernel in
{linear, rbf}, five stratified folds -- on seeded two-class data (y uniform, X = randn + 0.5 y on the first three features).  Steps:

* iteration: one RBF problem over all n rows, C = 1: the kernel matrix's time (HIP events, median of 5), then the wall time of launches of
  500 solver iterations, alone and three C values side by side -- microseconds per iteration, the figure svm.ITERS_PER_LAUNCH is sized by;
* grid: svm.grid_search_cv over the grid, wall time, with the iteration counts of the refit;
* sklearn_grid: GridSearchCV(SVC(), grid, cv=5, scoring='f1') on the host's CPUs, one job (libsvm is single-threaded), wall time.

Both sides stop a fit after --max-iter iterations (default 100 000; scikit-learn then warns, as svm.SVC does): the linear kernel at C = 10
otherwise runs for an unbounded time on data that is not separable.  Every GPU step runs in a child process of its own under a time
limit; after a step that fails or runs out of time nothing more is started on the GPU.  Nothing outside this repository is read.  Prints
one JSON line per step.
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

GRID = {"C": [0.1, 1, 10], "kernel": ["linear", "rbf"]}
LIMIT_S = {"iteration": 120, "grid": 420}


def synth(n, d=100, sep=0.5, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    y = np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0)
    X = rs.randn(n, d)
    X[:, :3] += sep * y[:, None]
    return X, y


def step_iteration(n):
    import torch
    from bbbp_amd import svm
    X, y = synth(n)
    dev = torch.device("cuda:0")
    Xd = torch.from_numpy(X).to(dev)
    yd = torch.from_numpy(-y).to(dev)
    g = svm._resolve_gamma("scale", Xd)
    K = svm.kernel_matrix(Xd, "rbf", g)[0]
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        K = svm.kernel_matrix(Xd, "rbf", g)[0]
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    res = {"step": "iteration", "n": n, "d": X.shape[1], "kernel_matrix_ms": sorted(times)[2]}
    for name, Cs in (("alone", (1.0,)), ("three_side_by_side", (0.1, 1.0, 10.0))):
        svm._solve([svm._Problem(K, yd, C, 1e-3) for C in Cs], max_iter=50)          # warm-up
        problems = [svm._Problem(K, yd, C, 1e-3) for C in Cs]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = svm._solve(problems, max_iter=500, iters_per_launch=500)
        dt = time.perf_counter() - t0
        ran = max(it for it, _ in out)
        res[f"us_per_iteration_{name}"] = dt * 1e6 / max(ran, 1)
        res[f"iterations_{name}"] = ran
    return res


def step_grid(n, max_iter):
    import torch
    from bbbp_amd import svm
    X, y = synth(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        svm.SVC(max_iter=10).fit(X[:500], y[:500])                                   # load the library, warm the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best, scores, fitted = svm.grid_search_cv(X, y, GRID, cv=5, max_iter=max_iter)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"step": "grid", "n": n, "d": X.shape[1], "max_iter": max_iter, "grid_search_cv_s": dt, "best": best, "scores": scores,
            "refit_iterations": fitted.n_iter_, "iters_per_launch": svm.ITERS_PER_LAUNCH}


def sklearn_grid(n, max_iter):
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import SVC
    X, y = synth(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        sk = GridSearchCV(SVC(max_iter=max_iter), GRID, cv=5, scoring="f1").fit(X, y)
        dt = time.perf_counter() - t0
    return {"step": "sklearn_grid", "n": n, "d": X.shape[1], "max_iter": max_iter, "grid_search_cv_s": dt, "best": sk.best_params_,
            "scores": [float(v) for v in sk.cv_results_["mean_test_score"]], "host_cpus": os.cpu_count(), "n_jobs": 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--n", type=int, default=8000)
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--step", help=argparse.SUPPRESS)                 # child mode: run one GPU step and print its JSON line
    a = ap.parse_args()
    if a.n < 100 or a.max_iter < 1:
        ap.error("--n must be at least 100 and --max-iter positive")
    if a.step:
        res = step_iteration(a.n) if a.step == "iteration" else step_grid(a.n, a.max_iter)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    lines = []
    rc = 0
    for name in ("iteration", "grid"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(a.n), "--max-iter", str(a.max_iter)],
                               capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"[bench_svc] {name}: no result within {LIMIT_S[name]} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_svc] {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
            break
        lines.append(json.loads(got[-1]))
        print(got[-1], flush=True)
    if rc == 0 and not a.no_sklearn:
        row = sklearn_grid(a.n, a.max_iter)
        lines.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
