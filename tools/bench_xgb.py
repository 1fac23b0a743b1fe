#!/usr/bin/env python3
"""Times xgb.XGBRegressor / xgb.fit_regressors on the GPU beside scikit-learn's histogram booster on one core of the host.

    python tools/bench_xgb.py [--out FILE] [--workload a|b|both] [--no-sklearn] [--reps R] [--sklearn-trees T]

Two seeded synthetic workloads at the reference's shapes (five folds of ``KFold(5, shuffle=True, random_state=42)`` plus the refit, six
problems in one ``fit_regressors`` batch over one matrix):

* a: ``XGBRegressor(n_estimators=300, learning_rate=0.01, max_depth=30)`` (Models/multi_input_data_regression_opt_transformer_cnn_20250108.py:
  186-189) on 1 058 x 49 319: 167 binary columns and 49 152 pixel-like columns, most of them constant (the white border), the rest with
  2-16 distinct values.
* b: ``XGBRegressor(n_estimators=200, max_depth=10, learning_rate=0.1)`` on 1 058 x 192 continuous columns.

Per workload: wall time of the batch behind a device synchronise (upload, cuts, bins, fit and the read-back of the trees included), warm-up
call first, the median of ``--reps`` calls, measured twice, both medians reported; trees per second; launches enqueued per tree; and from
one more fit with the events of ``bbbp_xgb_fit_profile`` on, the split kernel's time alone and the share of (node, feature) pairs that took
the small-node form (nodes of at most 64 rows).  The batch's models are compared with single fits bit for bit (workload b only: six more fits).

The baseline is ``HistGradientBoostingRegressor(loss="squared_error", l2_regularization=1.0, max_bins=255, min_samples_leaf=1,
max_leaf_nodes=None, early_stopping=False)`` with the same depth, rate and tree count in a child process held to one thread: a stand-in
with the same gain and leaf weight, NOT the reference's library (xgboost is not installed).  For workload a, where one of its trees
over 49 319 columns takes seconds, it fits the refit problem alone twice, with 2 and with ``--sklearn-trees`` trees (default 6); the time per
tree and the fixed cost (binning) follow from the two, and the time of six fits of 300 trees is extrapolated from them and marked so.

The GPU step runs in a child process of its own under a time limit; if it fails or runs out of time nothing more is started on the GPU.
Nothing outside this repository is read.  Prints one JSON line.
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

LIMIT_S = 900
PARAMS = {"a": dict(n_estimators=300, learning_rate=0.01, max_depth=30), "b": dict(n_estimators=200, learning_rate=0.1, max_depth=10)}


def synth(which, n=1058, seed=1):
    import numpy as np
    rs = np.random.default_rng(seed)
    if which == "b":
        X = rs.standard_normal((n, 192)).astype(np.float32)
        y = np.sin(2 * X[:, 0].astype(np.float64)) + X[:, 1].astype(np.float64) * X[:, 2] + 0.1 * rs.standard_normal(n)
        return X, y
    fp = (rs.random((n, 167)) < 0.2).astype(np.float32)
    img = np.ones((n, 3, 128, 128), np.float32)                      # white; a drawing in the middle 48 x 48, the same in the three channels
    levels = rs.integers(2, 17, size=(48, 48))
    ink = rs.random((n, 48, 48)) < 0.15
    shade = np.floor(rs.random((n, 48, 48)) * levels) / levels
    img[:, :, 40:88, 40:88] = np.where(ink, shade, 1.0).astype(np.float32)[:, None]
    X = np.hstack([fp, img.reshape(n, -1)])
    y = fp[:, :8].sum(axis=1) - 2.0 * X[:, 167 + 64 * 128 + 64] + X[:, 167 + 60 * 128 + 70] * fp[:, 9] + 0.1 * rs.standard_normal(n)
    return X, y


def problems_of(X, y):
    from sklearn.model_selection import KFold
    return [(X, y, tr) for tr, _ in KFold(5, shuffle=True, random_state=42).split(X)] + [(X, y)]


def _median(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2], times, out


def small_share(regs, max_depth):
    """The share of (searched node, live feature) pairs whose node has at most 64 rows; a searched node has two rows at least and lies above max_depth."""
    import numpy as np
    small = total = 0
    for reg in regs:
        t = reg.trees_
        depth = np.zeros(len(t["left"]), np.int64)
        frontier = t["root"][:-1].astype(np.int64)
        while frontier.size:
            inner = frontier[t["left"][frontier] >= 0]
            for side in ("left", "right"):
                depth[t[side][inner]] = depth[inner] + 1
            frontier = np.concatenate([t["left"][inner], t["right"][inner]]).astype(np.int64)
        searched = (t["sum_hessian"] >= 2) & (depth < max_depth)
        total += int(searched.sum()); small += int((searched & (t["sum_hessian"] <= 64)).sum())
    return small / max(total, 1)


def step_gpu(which, reps):
    import ctypes
    import numpy as np
    import torch
    from bbbp_amd import _lib, xgb
    X, y = synth(which)
    problems, kw = problems_of(X, y), PARAMS[which]
    xgb.XGBRegressor(n_estimators=3, max_depth=4).fit(X[:200, :200], y[:200])            # load the library, warm the allocator
    xgb.fit_regressors(problems, **{**kw, "n_estimators": 2})
    torch.cuda.synchronize()
    first_s, first_all, _ = _median(lambda: xgb.fit_regressors(problems, **kw), reps)
    second_s, second_all, batch = _median(lambda: xgb.fit_regressors(problems, **kw), reps)
    L = _lib.lib()
    L.bbbp_xgb_fit_profile(1)
    xgb.fit_regressors(problems, **kw)
    L.bbbp_xgb_fit_profile(0)
    split_ms, launches = ctypes.c_double(), ctypes.c_long()
    L.bbbp_xgb_fit_last(ctypes.byref(split_ms), ctypes.byref(launches))
    n_trees = len(problems) * kw["n_estimators"]
    out = {"workload": which, "n": X.shape[0], "d": X.shape[1], "problems": len(problems), **kw, "batch_ms": [1e3 * first_s, 1e3 * second_s],
           "batch_s_all": [first_all, second_all], "trees_per_s": [n_trees / first_s, n_trees / second_s],
           "launches_per_tree": launches.value / kw["n_estimators"], "split_kernel_ms": split_ms.value,
           "small_node_share": small_share(batch, kw["max_depth"]), "nodes_per_tree": sum(len(r.trees_["left"]) for r in batch) / n_trees,
           "deepest_tree": max(r.booster_.max_depth for r in batch), "refit_train_mse": float(np.mean((batch[-1].train_margin_ - y) ** 2))}
    if which == "b":
        alone = [xgb.XGBRegressor(**kw).fit(X[p[2]] if len(p) == 3 else X, y[p[2]] if len(p) == 3 else y) for p in problems]
        out["batch_equals_single_fits"] = bool(all(np.array_equal(a.trees_[k], b.trees_[k]) for a, b in zip(alone, batch) for k in a.trees_))
    return out


def step_sklearn(which, sk_trees):
    import numpy as np
    from sklearn.ensemble import HistGradientBoostingRegressor
    X, y = synth(which)
    kw = PARAMS[which]
    trees = kw["n_estimators"] if which == "b" else min(max(sk_trees, 3), kw["n_estimators"])
    problems = problems_of(X, y) if which == "b" else [(X, y)]

    def fits(T):
        t0 = time.perf_counter()
        fitted = [HistGradientBoostingRegressor(loss="squared_error", l2_regularization=1.0, max_bins=255, min_samples_leaf=1, max_leaf_nodes=None,
                                                max_depth=kw["max_depth"], learning_rate=kw["learning_rate"], max_iter=T, early_stopping=False)
                  .fit(X[p[2]] if len(p) == 3 else X, y[p[2]] if len(p) == 3 else y) for p in problems]
        return time.perf_counter() - t0, fitted

    fit_s, fitted = fits(trees)
    out = {"fits": len(problems), "trees_per_fit": trees, "fit_s": fit_s, "threads": 1, "refit_train_mse": float(np.mean((fitted[-1].predict(X) - y) ** 2))}
    if which == "a":
        short_s, _ = fits(2)
        per_tree = (fit_s - short_s) / (trees - 2)
        out.update(fit_s_2_trees=short_s, s_per_tree=per_tree, fixed_s=short_s - 2 * per_tree,
                   batch_ms_extrapolated=1e3 * 6 * (short_s - 2 * per_tree + kw["n_estimators"] * per_tree))
    else:
        out.update(batch_ms=1e3 * fit_s, trees_per_s=len(problems) * trees / fit_s)
    return out


def _child(args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=LIMIT_S, env=env)
    got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print(f"[bench_xgb] {' '.join(args)}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return r.returncode or 1, None
    return 0, json.loads(got[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--workload", choices=("a", "b", "both"), default="both")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sklearn-trees", type=int, default=6)
    ap.add_argument("--step", choices=("gpu", "sklearn"), help=argparse.SUPPRESS)      # child mode: run one step and print its JSON line
    a = ap.parse_args()
    if a.reps < 1 or a.sklearn_trees < 1:
        ap.error("--reps and --sklearn-trees at least 1")
    if a.step:
        res = step_gpu(a.workload, a.reps) if a.step == "gpu" else step_sklearn(a.workload, a.sklearn_trees)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    result, rc = {"bench": "xgb"}, 0
    one_thread = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for which in (("a", "b") if a.workload == "both" else (a.workload,)):
        try:
            rc, gpu = _child(["--step", "gpu", "--workload", which, "--reps", str(a.reps)])
            if rc:
                break
            result[which] = {"gpu": gpu}
            if not a.no_sklearn:
                rc, sk = _child(["--step", "sklearn", "--workload", which, "--sklearn-trees", str(a.sklearn_trees)], env=one_thread)
                if rc:
                    break
                result[which]["sklearn_hist"] = sk
        except subprocess.TimeoutExpired:
            print(f"[bench_xgb] workload {which}: no result within {LIMIT_S} s; stopping", file=sys.stderr)
            rc = 124
            break
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
