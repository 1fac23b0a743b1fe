#!/usr/bin/env python3
"""Times random_forest.RandomForestRegressor / random_forest.fit_regressors on the GPU beside scikit-learn on the host.

    python tools/bench_rfr.py [--out FILE] [--no-sklearn] [--n N] [--d D] [--trees T] [--depth DEPTH] [--jobs J]

The shape is the logBB stack's forest (Models/multi_input_data_regression_opt_transformer_cnn_opt.py:163-165): five folds (KFold(5) without
shuffling) of ``RandomForestRegressor(n_estimators=300, max_depth=15, random_state=42)`` on an [846, 192] float32 matrix, here seeded
synthetic data (X standard normal, y = sin(2 x0) + x1 x2 + 0.1 noise).

* alone: the five folds fitted one after the other, ``RandomForestRegressor.fit`` per fold.
* batch: the same five folds through ``fit_regressors``, every tree of every fold in one call.
* predict: every fold's forest on its held-out rows.
  Each is wall time behind a device synchronise, the median of three, after a small warm-up fit; the presort, the copies and the read-back
  of the node arrays are included.  The batch's forests are compared with the single fits bit for bit.
* sklearn: the same five fits and predictions on the host's CPUs with ``n_jobs`` = --jobs (default 16), once.

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

LIMIT_S = 300


def synth(n, d, seed=1):
    import numpy as np
    rs = np.random.default_rng(seed)
    X = rs.standard_normal((n, d)).astype(np.float32)
    y = np.sin(2 * X[:, 0].astype(np.float64)) + X[:, 1].astype(np.float64) * X[:, 2] + 0.1 * rs.standard_normal(n)
    return X, y


def folds_of(n, k=5):
    import numpy as np
    sizes = np.full(k, n // k)
    sizes[: n % k] += 1
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    return [(np.concatenate([np.arange(0, bounds[f]), np.arange(bounds[f + 1], n)]), np.arange(bounds[f], bounds[f + 1])) for f in range(k)]


def _median3(fn):
    import torch
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)[1], times, out


def step_gpu(n, d, trees, depth):
    import numpy as np
    import torch
    from bbbp_amd import random_forest as rf
    X, y = synth(n, d)
    folds = folds_of(n)
    kw = dict(n_estimators=trees, max_depth=depth, random_state=42)
    rf.RandomForestRegressor(3, max_depth=4).fit(X[:200], y[:200])          # load the library, warm the allocator
    torch.cuda.synchronize()
    alone_s, alone_all, alone = _median3(lambda: [rf.RandomForestRegressor(**kw).fit(X[tr], y[tr]) for tr, _ in folds])
    batch_s, batch_all, batch = _median3(lambda: rf.fit_regressors([(X[tr], y[tr]) for tr, _ in folds], **kw))
    same = all(np.array_equal(a.trees_[k], b.trees_[k]) for a, b in zip(alone, batch) for k in a.trees_)
    predict_s, predict_all, preds = _median3(lambda: [reg.predict(X[te]) for reg, (_, te) in zip(batch, folds)])
    mse = float(np.mean(np.concatenate([p - y[te] for p, (_, te) in zip(preds, folds)]) ** 2))
    return {"n": n, "d": d, "folds": len(folds), "n_estimators": trees, "max_depth": depth, "alone_s": alone_s, "alone_s_all": alone_all,
            "batch_s": batch_s, "batch_s_all": batch_all, "batch_equals_single_fits": bool(same), "predict_s": predict_s,
            "predict_s_all": predict_all, "trees_per_s_batch": len(folds) * trees / batch_s,
            "nodes_per_tree": float(sum(len(r.trees_["left"]) for r in batch)) / (len(folds) * trees), "out_of_fold_mse": mse}


def sklearn_rows(n, d, trees, depth, jobs):
    import numpy as np
    from sklearn.ensemble import RandomForestRegressor
    X, y = synth(n, d)
    folds = folds_of(n)
    t0 = time.perf_counter()
    fitted = [RandomForestRegressor(n_estimators=trees, max_depth=depth, random_state=42, n_jobs=jobs).fit(X[tr], y[tr]) for tr, _ in folds]
    fit_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    preds = [sk.predict(X[te]) for sk, (_, te) in zip(fitted, folds)]
    predict_s = time.perf_counter() - t0
    mse = float(np.mean(np.concatenate([p - y[te] for p, (_, te) in zip(preds, folds)]) ** 2))
    return {"fit_s": fit_s, "predict_s": predict_s, "n_jobs": jobs, "host_cpus": os.cpu_count(), "out_of_fold_mse": mse,
            "nodes_per_tree": float(sum(e.tree_.node_count for sk in fitted for e in sk.estimators_)) / (len(folds) * trees)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--n", type=int, default=846)
    ap.add_argument("--d", type=int, default=192)
    ap.add_argument("--trees", type=int, default=300)
    ap.add_argument("--depth", type=int, default=15)
    ap.add_argument("--jobs", type=int, default=16, help="scikit-learn's n_jobs")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)      # child mode: run the GPU step and print its JSON line
    a = ap.parse_args()
    if not 50 <= a.n <= 8192 or not 3 <= a.d <= 1024 or a.trees < 1 or a.depth < 1 or a.jobs < 1:
        ap.error("--n within 50..8192, --d within 3..1024, --trees, --depth and --jobs at least 1")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.n, a.d, a.trees, a.depth)), flush=True)
        return 0
    result = {"bench": "rfr"}
    rc = 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--n", str(a.n), "--d", str(a.d), "--trees", str(a.trees),
                            "--depth", str(a.depth)], capture_output=True, text=True, timeout=LIMIT_S)
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_rfr] gpu: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
        else:
            result["gpu"] = json.loads(got[-1])
    except subprocess.TimeoutExpired:
        print(f"[bench_rfr] gpu: no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    if rc == 0 and not a.no_sklearn:
        result["sklearn"] = sklearn_rows(a.n, a.d, a.trees, a.depth, a.jobs)
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
