#!/usr/bin/env python3
"""Times gradient_boosting.GradientBoostingRegressor / gradient_boosting.fit_regressors on the GPU beside scikit-learn on the host.

    python tools/bench_gbr.py [--out FILE] [--no-sklearn] [--n N] [--d D] [--trees T] [--depth DEPTH]

The shape is the logBB stack's bake-off (Models/multi_input_data_regression_opt_transformer_cnn_opt_more.py:118-125):
``GradientBoostingRegressor(n_estimators=200, learning_rate=0.1, max_depth=5, random_state=42)`` on five folds
(``KFold(5, shuffle=True, random_state=42)``) of 1 058 rows, plus the refit on all rows, here on seeded synthetic data of tools/bench_rfr.py's
width (X standard normal [1 058, 192] float32, y = sin(2 x0) + x1 x2 + 0.1 noise).

* batch: the five folds and the refit through ``fit_regressors``, six chains in one ``bbbp_gbr_fit`` call.
* alone: the same six problems fitted one after the other, ``GradientBoostingRegressor.fit`` each.
* predict: every fold's model on its held-out rows.
  Each is wall time behind a device synchronise, the median of three, after a small warm-up fit; the presort, the copies and the read-back
  of the node arrays are included.  The batch's models are compared with the single fits bit for bit.
* sklearn: the same six fits and five predictions on the host's CPUs, once (the learner has no ``n_jobs``: one core).

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


def problems_of(X, y):
    """The five folds' (train, test) rows and the six training problems: the folds, then all rows."""
    from sklearn.model_selection import KFold
    folds = list(KFold(5, shuffle=True, random_state=42).split(X))
    return folds, [(X[tr], y[tr]) for tr, _ in folds] + [(X, y)]


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
    from bbbp_amd import gradient_boosting as gb
    X, y = synth(n, d)
    folds, problems = problems_of(X, y)
    kw = dict(n_estimators=trees, learning_rate=0.1, max_depth=depth, random_state=42)
    gb.GradientBoostingRegressor(3, max_depth=4).fit(X[:200], y[:200])          # load the library, warm the allocator
    torch.cuda.synchronize()
    batch_s, batch_all, batch = _median3(lambda: gb.fit_regressors(problems, **kw))
    alone_s, alone_all, alone = _median3(lambda: [gb.GradientBoostingRegressor(**kw).fit(Xp, yp) for Xp, yp in problems])
    same = all(np.array_equal(a.trees_[k], b.trees_[k]) for a, b in zip(alone, batch) for k in a.trees_)
    predict_s, predict_all, preds = _median3(lambda: [reg.predict(X[te]) for reg, (_, te) in zip(batch, folds)])
    mse = float(np.mean(np.concatenate([p - y[te] for p, (_, te) in zip(preds, folds)]) ** 2))
    n_trees = len(problems) * trees
    return {"n": n, "d": d, "problems": len(problems), "n_estimators": trees, "max_depth": depth, "batch_s": batch_s, "batch_s_all": batch_all,
            "batch_ms": 1e3 * batch_s, "trees_per_s_batch": n_trees / batch_s, "alone_s": alone_s, "alone_s_all": alone_all,
            "batch_equals_single_fits": bool(same), "predict_s": predict_s, "predict_s_all": predict_all,
            "nodes_per_tree": float(sum(len(r.trees_["left"]) for r in batch)) / n_trees, "out_of_fold_mse": mse,
            "refit_train_score": float(batch[-1].train_score_[-1])}


def sklearn_rows(n, d, trees, depth):
    import numpy as np
    from sklearn.ensemble import GradientBoostingRegressor
    X, y = synth(n, d)
    folds, problems = problems_of(X, y)
    t0 = time.perf_counter()
    fitted = [GradientBoostingRegressor(n_estimators=trees, learning_rate=0.1, max_depth=depth, random_state=42).fit(Xp, yp) for Xp, yp in problems]
    fit_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    preds = [sk.predict(X[te]) for sk, (_, te) in zip(fitted, folds)]
    predict_s = time.perf_counter() - t0
    mse = float(np.mean(np.concatenate([p - y[te] for p, (_, te) in zip(preds, folds)]) ** 2))
    n_trees = len(problems) * trees
    return {"fit_s": fit_s, "batch_ms": 1e3 * fit_s, "trees_per_s": n_trees / fit_s, "predict_s": predict_s, "n_jobs": 1, "host_cpus": os.cpu_count(),
            "out_of_fold_mse": mse, "refit_train_score": float(fitted[-1].train_score_[-1]),
            "nodes_per_tree": float(sum(e.tree_.node_count for sk in fitted for e in sk.estimators_[:, 0])) / n_trees}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--n", type=int, default=1058)
    ap.add_argument("--d", type=int, default=192)
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)      # child mode: run the GPU step and print its JSON line
    a = ap.parse_args()
    if not 50 <= a.n <= 8192 or not 3 <= a.d <= 1024 or a.trees < 1 or not 1 <= a.depth <= 7:
        ap.error("--n within 50..8192, --d within 3..1024, --trees at least 1, --depth within 1..7")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.n, a.d, a.trees, a.depth)), flush=True)
        return 0
    result = {"bench": "gbr"}
    rc = 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--n", str(a.n), "--d", str(a.d), "--trees", str(a.trees),
                            "--depth", str(a.depth)], capture_output=True, text=True, timeout=LIMIT_S)
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_gbr] gpu: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
        else:
            result["gpu"] = json.loads(got[-1])
    except subprocess.TimeoutExpired:
        print(f"[bench_gbr] gpu: no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    if rc == 0 and not a.no_sklearn:
        result["sklearn"] = sklearn_rows(a.n, a.d, a.trees, a.depth)
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
