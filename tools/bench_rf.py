#!/usr/bin/env python3
"""Times random_forest.RandomForestClassifier / random_forest.grid_search_cv on the GPU beside scikit-learn on the host.

    python tools/bench_rf.py [--out FILE] [--no-sklearn] [--n N] [--trees T] [--only single|grid]

Shapes, on seeded two-class data (y uniform, X = randn + 0.5 y on the first three features):

* single: one default fit -- n rows of d = 100 features, 100 trees, no depth limit, max_features "sqrt", bootstrap: wall time behind a
  device synchronise, the median of three, after a small warm-up fit.
* grid: the reference's classifier grid -- n rows of d = 100 PCA features, n_estimators in {50, 100, 200, 300} (scaled by --trees / 300),
  max_depth in {None, 10, 20, 30}, min_samples_split in {2, 5, 10}, min_samples_leaf in {1, 2, 4}, five stratified folds: 144 points, one
  forest per fold and min_samples_leaf (15 forests of the largest n_estimators), every other point scored through the predict kernel's
  limits, then the refit.  Wall time of random_forest.grid_search_cv behind a device synchronise.
* sklearn: on the host's CPUs, one job -- the single shape in full, and of the grid a stated subset: one fit of SKLEARN_TREES trees on
  one fold (4/5 of the rows) at each (max_depth, min_samples_leaf) with min_samples_split = 2, as seconds per tree.  The grid's
  scikit-learn time is NOT measured; ``sklearn_grid_s_extrapolated`` is 5 folds x sum over the 144 points of n_estimators x the measured
  seconds per tree at the point's (max_depth, min_samples_leaf) -- min_samples_split 5 and 10 are charged as 2, which overstates them --
  and says so in its name.

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

LIMIT_S = {"single": 300, "grid": 400}
SKLEARN_TREES = 8
DEPTHS, LEAVES, SPLITS = [None, 10, 20, 30], [1, 2, 4], [2, 5, 10]


def grid_of(trees):
    return {"n_estimators": sorted({max(1, trees // 6), max(1, trees // 3), max(1, 2 * trees // 3), trees}), "max_depth": DEPTHS,
            "min_samples_split": SPLITS, "min_samples_leaf": LEAVES}


def synth(n, d, sep=0.5, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 2, n)
    X = rs.randn(n, d)
    X[:, :3] += sep * (2.0 * y[:, None] - 1.0)
    return X, y


def _shape(trees):
    import numpy as np
    root = trees["root"]
    depth = 0
    for t in range(min(len(root) - 1, 10)):                # depth of the first trees, level by level numbering: walk the leftmost-deepest
        lo, hi = int(root[t]), int(root[t + 1])
        level, dpt = np.array([lo]), 0
        while True:
            kids = np.concatenate([trees["left"][level], trees["right"][level]])
            kids = kids[kids >= 0]
            if not len(kids):
                break
            level, dpt = kids, dpt + 1
        depth = max(depth, dpt)
    return {"nodes_per_tree": float(root[-1]) / (len(root) - 1), "max_depth_first_trees": depth}


def step_single(n, trees):
    import torch
    from bbbp_amd import random_forest as rf
    X, y = synth(n, 100)
    rf.RandomForestClassifier(3).fit(X[:500], y[:500])           # load the library, warm the allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        clf = rf.RandomForestClassifier(100).fit(X, y)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    fit_s = sorted(times)[1]
    acc = float((clf.predict(X) == y).mean())
    return {"n": n, "d": 100, "n_estimators": 100, "fit_s": fit_s, "fit_s_all": times, "trees_per_s": 100 / fit_s, "train_accuracy": acc, **_shape(clf.trees_)}


def step_grid(n, trees):
    import torch
    from bbbp_amd import random_forest as rf
    X, y = synth(n, 100)
    rf.RandomForestClassifier(3).fit(X[:500], y[:500])
    torch.cuda.synchronize()
    grid = grid_of(trees)
    before = rf._GROWN["trees"]
    t0 = time.perf_counter()
    best, scores, fitted = rf.grid_search_cv(X, y, grid, cv=5)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    grown = rf._GROWN["trees"] - before
    return {"n": n, "d": 100, "grid": grid, "points": len(scores), "forests": 5 * len(LEAVES), "trees_grown": grown, "grid_search_cv_s": dt,
            "trees_per_s": grown / dt, "best": best, "best_f1": max(scores), "worst_f1": min(scores)}


def sklearn_rows(n, trees):
    from sklearn.ensemble import RandomForestClassifier
    X, y = synth(n, 100)
    t0 = time.perf_counter()
    sk = RandomForestClassifier(n_estimators=100, random_state=0).fit(X, y)
    single = {"fit_s": time.perf_counter() - t0, "train_accuracy": float((sk.predict(X) == y).mean()),
              "nodes_per_tree": float(sum(e.tree_.node_count for e in sk.estimators_)) / 100, "max_depth": max(e.tree_.max_depth for e in sk.estimators_)}
    m = n * 4 // 5
    per_tree = {}
    for depth in DEPTHS:
        for msl in LEAVES:
            t0 = time.perf_counter()
            RandomForestClassifier(n_estimators=SKLEARN_TREES, max_depth=depth, min_samples_leaf=msl, random_state=0).fit(X[:m], y[:m])
            per_tree[f"{depth}/{msl}"] = (time.perf_counter() - t0) / SKLEARN_TREES
    grid = grid_of(trees)
    total = 5 * len(SPLITS) * sum(T * per_tree[f"{depth}/{msl}"] for T in grid["n_estimators"] for depth in DEPTHS for msl in LEAVES)
    n_trees = 5 * len(SPLITS) * len(DEPTHS) * len(LEAVES) * sum(grid["n_estimators"])
    return {"single": single, "grid_subset": {"rows": m, "d": 100, "trees_timed": SKLEARN_TREES, "min_samples_split": 2,
                                              "s_per_tree_by_depth_and_leaf": per_tree},
            "sklearn_grid_trees": n_trees, "sklearn_grid_s_extrapolated": total, "host_cpus": os.cpu_count(), "n_jobs": 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--n", type=int, default=6400)
    ap.add_argument("--trees", type=int, default=300, help="the grid's largest n_estimators (the reference's: 300)")
    ap.add_argument("--only", choices=["single", "grid"], help="run one GPU step only")
    ap.add_argument("--step", help=argparse.SUPPRESS)                 # child mode: run one GPU step and print its JSON line
    a = ap.parse_args()
    if not 100 <= a.n <= 8192 or a.trees < 6:
        ap.error("--n must be within 100..8192 and --trees at least 6")
    if a.step:
        res = step_grid(a.n, a.trees) if a.step == "grid" else step_single(a.n, a.trees)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    result = {"bench": "rf"}
    rc = 0
    for name in ("single", "grid"):
        if a.only and a.only != name:
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(a.n), "--trees", str(a.trees)],
                               capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"[bench_rf] {name}: no result within {LIMIT_S[name]} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_rf] {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
            break
        result[name] = json.loads(got[-1])
        print(f"[bench_rf] {name}: done", file=sys.stderr, flush=True)
    if rc == 0 and not a.no_sklearn:
        result["sklearn"] = sklearn_rows(a.n, a.trees)
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
