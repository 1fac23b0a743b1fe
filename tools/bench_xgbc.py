#!/usr/bin/env python3
"""Times xgb.XGBClassifier / xgb.fit_classifiers on the GPU beside scikit-learn's histogram booster on one core of the host.

    python tools/bench_xgbc.py [--out FILE] [--no-sklearn] [--reps R]

One seeded synthetic workload at the reference's shape (Models/model_opt_20250130.py: about 1 600 training rows of 50 PCA components):
1 600 rows x 50 PCA-like columns (independent normals with a decaying scale), labels from a noisy nonlinear score, and the reference's
``XGBClassifier(learning_rate=0.02, n_estimators=500, max_depth=7, colsample_bytree=0.8, subsample=0.8, reg_lambda=3)``: the five folds of
``StratifiedKFold(5)`` plus the refit, six problems in one ``fit_classifiers`` batch over one matrix.

Reported: wall time of the batch behind a device synchronise (upload, cuts, bins, column masks, fit and the read-back of the trees
included), warm-up call first, the median of ``--reps`` calls, measured twice, both medians; trees per second; nodes per tree; the refit's
training accuracy; the time of ``predict_proba`` on the 1 600 rows; whether the batch's models equal single fits bit for bit.

The baseline is ``HistGradientBoostingClassifier(max_iter=500, max_depth=7, learning_rate=0.02, l2_regularization=3, max_leaf_nodes=None,
min_samples_leaf=1, early_stopping=False)`` on the same six problems in a child process held to one thread: a stand-in with the same gain and
leaf weight but no row or column sampling, NOT the reference's library (xgboost is not installed).

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
PARAMS = dict(learning_rate=0.02, n_estimators=500, max_depth=7, colsample_bytree=0.8, subsample=0.8, reg_lambda=3)


def synth(n=1600, d=50, seed=1):
    import numpy as np
    rs = np.random.default_rng(seed)
    X = (rs.standard_normal((n, d)) * np.linspace(3.0, 0.3, d)).astype(np.float32)
    score = 0.8 * X[:, 0] - 0.6 * X[:, 1] * np.sign(X[:, 2]) + np.sin(X[:, 3]) + 0.5 * X[:, 10] + 1.5 * rs.standard_normal(n)
    return X, (score > 0).astype(np.int64)


def problems_of(X, y):
    from sklearn.model_selection import StratifiedKFold
    return [(X, y, tr) for tr, _ in StratifiedKFold(5).split(X, y)] + [(X, y)]


def _median(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2], times, out


def step_gpu(reps):
    import numpy as np
    import torch
    from bbbp_amd import xgb
    X, y = synth()
    problems = problems_of(X, y)
    xgb.XGBClassifier(n_estimators=3, max_depth=4).fit(X[:200], y[:200])                 # load the library, warm the allocator
    xgb.fit_classifiers(problems, **{**PARAMS, "n_estimators": 2})
    torch.cuda.synchronize()
    first_s, first_all, _ = _median(lambda: xgb.fit_classifiers(problems, **PARAMS), reps)
    second_s, second_all, batch = _median(lambda: xgb.fit_classifiers(problems, **PARAMS), reps)
    refit = batch[-1]
    proba_s, _, proba = _median(lambda: refit.predict_proba(X), 5)
    n_trees = len(problems) * PARAMS["n_estimators"]
    alone = [xgb.XGBClassifier(**PARAMS).fit(X[p[2]] if len(p) == 3 else X, y[p[2]] if len(p) == 3 else y) for p in problems[:1] + problems[-1:]]
    same = all(np.array_equal(a.trees_[k], b.trees_[k]) for a, b in zip(alone, batch[:1] + batch[-1:]) for k in a.trees_)
    return {"n": X.shape[0], "d": X.shape[1], "problems": len(problems), **PARAMS, "batch_ms": [1e3 * first_s, 1e3 * second_s],
            "batch_s_all": [first_all, second_all], "trees_per_s": [n_trees / first_s, n_trees / second_s],
            "nodes_per_tree": sum(len(c.trees_["left"]) for c in batch) / n_trees, "deepest_tree": max(c.booster_.max_depth for c in batch),
            "refit_train_accuracy": float(((proba[:, 1] > 0.5) == (y == 1)).mean()), "predict_proba_ms": 1e3 * proba_s,
            "fold_and_refit_equal_single_fits": bool(same)}


def step_sklearn():
    from sklearn.ensemble import HistGradientBoostingClassifier
    X, y = synth()
    t0 = time.perf_counter()
    fitted = [HistGradientBoostingClassifier(max_iter=PARAMS["n_estimators"], max_depth=PARAMS["max_depth"], learning_rate=PARAMS["learning_rate"],
                                             l2_regularization=float(PARAMS["reg_lambda"]), max_leaf_nodes=None, min_samples_leaf=1, early_stopping=False)
              .fit(X[p[2]] if len(p) == 3 else X, y[p[2]] if len(p) == 3 else y) for p in problems_of(X, y)]
    fit_s = time.perf_counter() - t0
    return {"fits": len(fitted), "threads": 1, "batch_ms": 1e3 * fit_s, "trees_per_s": len(fitted) * PARAMS["n_estimators"] / fit_s,
            "refit_train_accuracy": float((fitted[-1].predict(X) == y).mean())}


def _child(args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=LIMIT_S, env=env)
    got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print(f"[bench_xgbc] {' '.join(args)}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return r.returncode or 1, None
    return 0, json.loads(got[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step", choices=("gpu", "sklearn"), help=argparse.SUPPRESS)      # child mode: run one step and print its JSON line
    a = ap.parse_args()
    if a.reps < 1:
        ap.error("--reps at least 1")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.reps) if a.step == "gpu" else step_sklearn()), flush=True)
        return 0
    result, rc = {"bench": "xgbc"}, 0
    one_thread = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    try:
        rc, gpu = _child(["--step", "gpu", "--reps", str(a.reps)])
        if not rc:
            result["gpu"] = gpu
            if not a.no_sklearn:
                rc, sk = _child(["--step", "sklearn"], env=one_thread)
                if not rc:
                    result["sklearn_hist"] = sk
    except subprocess.TimeoutExpired:
        print(f"[bench_xgbc] no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
