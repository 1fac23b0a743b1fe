#!/usr/bin/env python3
"""Times cat.CatBoostClassifier / cat.fit_classifiers on the GPU, beside cat.CatBoostRegressor on the same matrix.

    python tools/bench_catc.py [--out FILE] [--reps R] [--iterations T]

One seeded synthetic workload at the shape of the reference's classification scripts behind PCA, 6 246 x 100 float64 rows with two
classes, and the reference's ``CatBoostClassifier(iterations=500, learning_rate=0.03, depth=10, l2_leaf_reg=5, bagging_temperature=0.5,
loss_function="Logloss", random_seed=42)`` (Models/model_opt_20250130.py:413-457): the five folds of ``StratifiedKFold(5)`` and the refit,
six problems in one ``fit_classifiers`` batch over one matrix.  Three variants, in the same process:

* ``classifier_no_bootstrap``: ``bootstrap_type="No"`` (no weight table);
* ``classifier_bayesian``: the reference's temperature 0.5;
* ``regressor``: ``cat.fit_regressors`` on the same matrix with the 0 / 1 labels as targets and the same trees, depth, rate,
  ``l2_leaf_reg`` and ``border_count``.

Per variant: wall time of the batch behind a device synchronise (upload, cuts, bins, weight table, fit, borders and the read-back of the
trees included), warm-up call first, the median of ``--reps`` calls, measured twice, both medians reported; milliseconds per tree of the
batch; and from one more fit with the events of ``bbbp_catc_fit_profile`` / ``bbbp_cat_fit_profile`` on, the split kernel's time alone and
its share of that fit.  The host time to build the weight table ``[iterations, 6 246]`` is reported on its own.  ``--iterations`` shortens
the fits (the time per tree does not depend on the tree count).

There is no library baseline: catboost is not installed and scikit-learn has no symmetric trees.  The yardstick is the regressor of the
same session: ``ratio_no_bootstrap`` and ``ratio_bayesian`` are the classifier's time per tree over the regressor's.  The classifier's split
kernel differs from the regressor's by one 64-bit LDS atomic where that has a 32-bit one and one more lane read per row in the small
form; a ratio much above 1.25 means that something other than the loss changed.  The ratio is reported, not gated.

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
PARAMS = dict(iterations=500, learning_rate=0.03, depth=10, l2_leaf_reg=5, border_count=254)
TEMPERATURE, SEED = 0.5, 42


def synth(n=6246, d=100, seed=1):
    """Principal-component-like columns (decreasing scale) and a label that needs several of them."""
    import numpy as np
    rs = np.random.default_rng(seed)
    X = rs.standard_normal((n, d)) * (1.0 / np.sqrt(1.0 + np.arange(d)))[None, :]
    z = 2.0 * X[:, 0] - 1.5 * X[:, 1] + np.sin(3.0 * X[:, 2]) + X[:, 3] * X[:, 4] + 0.5 * rs.logistic(size=n)
    return X, (z > np.quantile(z, 0.6)).astype(np.int64)


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


def _variant(fit, warm, profile, last, reps, iterations):
    import ctypes
    import torch
    warm()
    torch.cuda.synchronize()
    first_s, first_all, _ = _median(fit, reps)
    second_s, second_all, batch = _median(fit, reps)
    profile(1)
    t0 = time.perf_counter()
    fit()
    torch.cuda.synchronize()
    profiled_s = time.perf_counter() - t0
    profile(0)
    split_ms, launches = ctypes.c_double(), ctypes.c_long()
    last(ctypes.byref(split_ms), ctypes.byref(launches))
    return batch, {"batch_ms": [1e3 * first_s, 1e3 * second_s], "batch_s_all": [first_all, second_all],
                   "ms_per_tree": [1e3 * first_s / iterations, 1e3 * second_s / iterations], "launches_per_tree": (launches.value - 1) / iterations,
                   "split_kernel_ms_per_tree": split_ms.value / iterations, "split_kernel_share_of_profiled_fit": split_ms.value / (1e3 * profiled_s)}


def step_gpu(reps, iterations):
    import numpy as np
    import torch
    from bbbp_amd import _lib, cat
    X, y = synth()
    problems, kw = problems_of(X, y), {**PARAMS, "iterations": iterations}
    targets = [(p[0], p[1].astype(np.float64), *p[2:]) for p in problems]
    L = _lib.lib()
    cat.CatBoostClassifier(iterations=3, depth=4).fit(X[:200], y[:200])                  # load the library, warm the allocator
    t0 = time.perf_counter()
    table = cat.weight_table(SEED, TEMPERATURE, iterations, X.shape[0])
    table_s = time.perf_counter() - t0
    out = {"n": X.shape[0], "d": X.shape[1], "problems": len(problems), **kw, "bagging_temperature": TEMPERATURE,
           "weight_table_host_ms": 1e3 * table_s, "weight_table_bytes": int(table.nbytes)}
    variants = {
        "regressor": (lambda k: cat.fit_regressors(targets, **k), L.bbbp_cat_fit_profile, L.bbbp_cat_fit_last),
        "classifier_no_bootstrap": (lambda k: cat.fit_classifiers(problems, bootstrap_type="No", **k), L.bbbp_catc_fit_profile, L.bbbp_catc_fit_last),
        "classifier_bayesian": (lambda k: cat.fit_classifiers(problems, bagging_temperature=TEMPERATURE, random_seed=SEED, **k), L.bbbp_catc_fit_profile,
                                L.bbbp_catc_fit_last),
    }
    for name, (fit, profile, last) in variants.items():
        batch, out[name] = _variant(lambda: fit(kw), lambda: fit({**kw, "iterations": 2}), profile, last, reps, iterations)
        if name != "regressor":
            refit = batch[-1]
            out[name]["refit_train_accuracy"] = float((refit.predict(X) == y).mean())
            out[name]["refit_train_logloss"] = float(np.mean(np.log1p(np.exp(-np.where(y > 0, refit.train_approx_, -refit.train_approx_)))))
    torch.cuda.synchronize()
    base = out["regressor"]["ms_per_tree"][1]
    out["ratio_no_bootstrap"] = out["classifier_no_bootstrap"]["ms_per_tree"][1] / base
    out["ratio_bayesian"] = out["classifier_bayesian"]["ms_per_tree"][1] / base
    return out


def _child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=LIMIT_S)
    got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print(f"[bench_catc] {' '.join(args)}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return r.returncode or 1, None
    return 0, json.loads(got[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=PARAMS["iterations"])
    ap.add_argument("--step", choices=("gpu",), help=argparse.SUPPRESS)                   # child mode: run the step and print its JSON line
    a = ap.parse_args()
    if a.reps < 1 or a.iterations < 1:
        ap.error("--reps and --iterations at least 1")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.reps, a.iterations)), flush=True)
        return 0
    result, rc = {"bench": "catc"}, 0
    try:
        rc, gpu = _child(["--step", "gpu", "--reps", str(a.reps), "--iterations", str(a.iterations)])
        if not rc:
            result["gpu"] = gpu
    except subprocess.TimeoutExpired:
        print(f"[bench_catc] no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
