#!/usr/bin/env python3
"""Times gradient_boosting.GradientBoostingClassifier / gradient_boosting.grid_search_cv on the GPU beside scikit-learn on the host.

    python tools/bench_gbt.py [--out FILE] [--no-sklearn] [--n N] [--trees T]

Shapes, on seeded two-class data (y uniform, X = randn + 0.5 y on the first three features):

* grid: the reference's classifier grid -- n = 8000 SMOTE-balanced rows of d = 100 PCA features, n_estimators in {50, 100, 200} (scaled by
  --trees / 200), learning_rate in {0.01, 0.05, 0.1}, max_depth in {3, 5, 7}, min_samples_split in {2, 5, 10}, five stratified folds: 81
  points, 27 chains per fold, 135 chains in one batch, then the refit.  Wall time of gradient_boosting.grid_search_cv behind a device
  synchronise, after a small warm-up fit.
* stack: the StackingClassifier's final estimator -- n rows of d = 8 base-learner outputs, 100 trees of depth 3: one fit, wall time.
* sklearn: on the host's CPUs, one job -- the stack shape in full, and of the grid a stated subset: one fit of SKLEARN_TREES trees on one
  fold (4/5 of the rows) at each max_depth, as seconds per tree.  The grid's scikit-learn time is NOT measured; ``sklearn_grid_s_extrapolated``
  is 5 folds x sum over the 81 points of n_estimators x the measured seconds per tree at the point's depth, and says so in its name.

Every GPU step runs in a child process of its own under a time limit; after a step that fails or runs out of time nothing more is
started on the GPU.  Nothing outside this repository is read.  Prints one JSON line.
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

LIMIT_S = {"grid": 900, "stack": 120}
SKLEARN_TREES = 4


def grid_of(trees):
    return {"n_estimators": sorted({max(1, trees // 4), max(1, trees // 2), trees}), "learning_rate": [0.01, 0.05, 0.1], "max_depth": [3, 5, 7],
            "min_samples_split": [2, 5, 10]}


def synth(n, d, sep=0.5, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 2, n)
    X = rs.randn(n, d)
    X[:, :3] += sep * (2.0 * y[:, None] - 1.0)
    return X, y


def step_grid(n, trees):
    import torch
    from bbbp_amd import gradient_boosting as gb
    X, y = synth(n, 100)
    gb.GradientBoostingClassifier(3, max_depth=7).fit(X[:500], y[:500])          # load the library, warm the allocator
    torch.cuda.synchronize()
    grid = grid_of(trees)
    t0 = time.perf_counter()
    best, scores, fitted = gb.grid_search_cv(X, y, grid, cv=5)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"n": n, "d": 100, "grid": grid, "points": len(scores), "chains": 27 * 5, "grid_search_cv_s": dt, "best": best, "best_f1": max(scores),
            "worst_f1": min(scores), "refit_train_score": float(fitted.train_score_[-1])}


def step_stack(n):
    import torch
    from bbbp_amd import gradient_boosting as gb
    X, y = synth(n, 8)
    gb.GradientBoostingClassifier(3).fit(X[:500], y[:500])
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        clf = gb.GradientBoostingClassifier(100, 0.1, 3).fit(X, y)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"n": n, "d": 8, "n_estimators": 100, "max_depth": 3, "fit_s": sorted(times)[1], "train_score": float(clf.train_score_[-1])}


def sklearn_rows(n, trees):
    from sklearn.ensemble import GradientBoostingClassifier
    X, y = synth(n, 8)
    t0 = time.perf_counter()
    sk = GradientBoostingClassifier(n_estimators=100, max_depth=3, random_state=0).fit(X, y)
    stack = {"fit_s": time.perf_counter() - t0, "train_score": float(sk.train_score_[-1])}
    X, y = synth(n, 100)
    m = n * 4 // 5
    per_tree = {}
    for depth in (3, 5, 7):
        t0 = time.perf_counter()
        GradientBoostingClassifier(n_estimators=SKLEARN_TREES, max_depth=depth, random_state=0).fit(X[:m], y[:m])
        per_tree[str(depth)] = (time.perf_counter() - t0) / SKLEARN_TREES
    grid = grid_of(trees)
    total = 5 * sum(T * per_tree[str(depth)] for T in grid["n_estimators"] for depth in grid["max_depth"]) * 9
    return {"stack": stack, "grid_subset": {"rows": m, "d": 100, "trees_timed": SKLEARN_TREES, "s_per_tree_by_depth": per_tree},
            "sklearn_grid_s_extrapolated": total, "host_cpus": os.cpu_count(), "n_jobs": 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--n", type=int, default=8000)
    ap.add_argument("--trees", type=int, default=200, help="the grid's largest n_estimators (the reference's: 200)")
    ap.add_argument("--step", help=argparse.SUPPRESS)                 # child mode: run one GPU step and print its JSON line
    a = ap.parse_args()
    if not 100 <= a.n <= 8192 or a.trees < 4:
        ap.error("--n must be within 100..8192 and --trees at least 4")
    if a.step:
        res = step_grid(a.n, a.trees) if a.step == "grid" else step_stack(a.n)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    result = {"bench": "gbt"}
    rc = 0
    for name in ("stack", "grid"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(a.n), "--trees", str(a.trees)],
                               capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"[bench_gbt] {name}: no result within {LIMIT_S[name]} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_gbt] {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
            break
        result[name] = json.loads(got[-1])
    if rc == 0 and not a.no_sklearn:
        result["sklearn"] = sklearn_rows(a.n, a.trees)
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
