#!/usr/bin/env python3
"""Times cat.CatBoostRegressor / cat.fit_regressors on the GPU.

    python tools/bench_cat.py [--out FILE] [--workload a|b|both] [--reps R] [--iterations T]

Two seeded synthetic workloads at the reference's shapes (five folds of ``KFold(5, shuffle=True, random_state=42)`` plus the refit, six
problems in one ``fit_regressors`` batch over one matrix), both with the reference's ``CatBoostRegressor(iterations=300, learning_rate=0.01,
depth=10)`` (Models/multi_input_data_regression_opt_transformer_cnn_20250108.py:192-195):

* a: 1 058 x 49 319, the matrix of ``tools/bench_xgb.py``'s workload a (167 binary columns and 49 152 pixel-like columns, most of them
  constant, the rest with 2-16 distinct values): the same data, the same bins, the same rows.
* b: the stacker's shape, 1 058 x 4 continuous columns (the out-of-fold matrix ``[nn, rf, xgb, cat]``).

Per workload: wall time of the batch behind a device synchronise (upload, cuts, bins, fit, borders and the read-back of the trees
included), warm-up call first, the median of ``--reps`` calls, measured twice, both medians reported; milliseconds per tree of the batch
(six problems side by side); launches enqueued per tree; and from one more fit with the events of ``bbbp_cat_fit_profile`` on, the split
kernel's time alone.  The batch's models are compared with single fits bit for bit (workload b only: six more fits).  ``--iterations``
shortens the fits (the time per tree does not depend on the tree count).

There is no library baseline: catboost is not installed and scikit-learn has no symmetric trees.  The yardstick is workload a of
``tools/bench_xgb.py`` run in the same session on the same box: its ``batch_ms / n_estimators`` beside this tool's ``ms_per_tree``.

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
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

LIMIT_S = 900
PARAMS = dict(iterations=300, learning_rate=0.01, depth=10)


def synth(which, n=1058, seed=1):
    import numpy as np
    if which == "a":
        import bench_xgb
        return bench_xgb.synth("a", n, seed)
    rs = np.random.default_rng(seed)
    y = rs.standard_normal(n)
    X = (y[:, None] + 0.4 * rs.standard_normal((n, 4))).astype(np.float32)
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


def step_gpu(which, reps, iterations):
    import ctypes
    import numpy as np
    import torch
    from bbbp_amd import _lib, cat
    X, y = synth(which)
    problems, kw = problems_of(X, y), {**PARAMS, "iterations": iterations}
    cat.CatBoostRegressor(iterations=3, depth=4).fit(X[:200, :200], y[:200])             # load the library, warm the allocator
    cat.fit_regressors(problems, **{**kw, "iterations": 2})
    torch.cuda.synchronize()
    first_s, first_all, _ = _median(lambda: cat.fit_regressors(problems, **kw), reps)
    second_s, second_all, batch = _median(lambda: cat.fit_regressors(problems, **kw), reps)
    L = _lib.lib()
    L.bbbp_cat_fit_profile(1)
    cat.fit_regressors(problems, **kw)
    L.bbbp_cat_fit_profile(0)
    split_ms, launches = ctypes.c_double(), ctypes.c_long()
    L.bbbp_cat_fit_last(ctypes.byref(split_ms), ctypes.byref(launches))
    out = {"workload": which, "n": X.shape[0], "d": X.shape[1], "problems": len(problems), **kw, "batch_ms": [1e3 * first_s, 1e3 * second_s], "batch_s_all": [first_all, second_all],
           "ms_per_tree": [1e3 * first_s / iterations, 1e3 * second_s / iterations], "launches_per_tree": (launches.value - 1) / iterations,
           "split_kernel_ms": split_ms.value, "split_kernel_ms_per_tree": split_ms.value / iterations,
           "refit_train_mse": float(np.mean((batch[-1].train_approx_ - y) ** 2)), "y_variance": float(np.var(y))}
    if which == "b":
        alone = [cat.CatBoostRegressor(**kw).fit(X[p[2]] if len(p) == 3 else X, y[p[2]] if len(p) == 3 else y) for p in problems]
        out["batch_equals_single_fits"] = bool(all(np.array_equal(a.trees_[k], b.trees_[k]) for a, b in zip(alone, batch) for k in a.trees_))
    return out


def _child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=LIMIT_S)
    got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print(f"[bench_cat] {' '.join(args)}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return r.returncode or 1, None
    return 0, json.loads(got[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--workload", choices=("a", "b", "both"), default="both")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=PARAMS["iterations"])
    ap.add_argument("--step", choices=("gpu",), help=argparse.SUPPRESS)                   # child mode: run one step and print its JSON line
    a = ap.parse_args()
    if a.reps < 1 or a.iterations < 1:
        ap.error("--reps and --iterations at least 1")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.workload, a.reps, a.iterations)), flush=True)
        return 0
    result, rc = {"bench": "cat"}, 0
    for which in (("a", "b") if a.workload == "both" else (a.workload,)):
        try:
            rc, gpu = _child(["--step", "gpu", "--workload", which, "--reps", str(a.reps), "--iterations", str(a.iterations)])
            if rc:
                break
            result[which] = {"gpu": gpu}
        except subprocess.TimeoutExpired:
            print(f"[bench_cat] workload {which}: no result within {LIMIT_S} s; stopping", file=sys.stderr)
            rc = 124
            break
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
