#!/usr/bin/env python3
"""Times naive_bayes.grid_search_cv and naive_bayes.learning_curve on the GPU beside scikit-learn on one core of the host.

    python tools/bench_bnb.py [--out FILE] [--no-sklearn] [--reps R]

The workload is the reference's BernoulliNB step (Models/model_maccs.py:257-267) on seeded synthetic [6 246, 100] float64 data
(Bernoulli fingerprints with bit rates in [0.05, 0.65] that differ a little between the classes, standardised, PCA(100)):

* grid: ``GridSearchCV(BernoulliNB(), {alpha: 5 values, binarize: 3 values}, cv=5, scoring='f1')`` with the refit -- 75 fits, 75 scoring
  passes and the refit.  ``naive_bayes.grid_search_cv(X, y, grid)`` from a host array: the upload, one pack, one count launch, the read
  of the counts, the tables in numpy, one jll launch, the read of the scores' inputs, F1 on the host.
* curve: ``learning_curve(best, cv=6, train_sizes=np.linspace(.1, 1, 5))`` -- 30 fits, 60 scoring passes -- with ``scoring="accuracy"``
  (the script's default, ``estimator.score``).
  Each is an end-to-end call time: wall time behind a device synchronise, after two warm-up calls, the median of --reps calls (default
  15) with the fastest, the slowest and the quartiles, so that the spread is on record.  The calls are latency-bound: three launches and
  a handful of copies.  ``launches`` counts the three kernels' launches per call.
* sklearn: the same two calls with scikit-learn, ``n_jobs=1``, on one core: the median of five after one warm-up.

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
N, D, BITS = 6246, 100, 167
GRID = {"alpha": [0.01, 0.1, 0.5, 1.0, 2.0], "binarize": [0.0, 0.5, 1.0]}
CURVE_CV = 6                                       # train_sizes=np.linspace(.1, 1, 5)


def synth(seed=1):
    import numpy as np
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    rs = np.random.default_rng(seed)
    y = (rs.random(N) < 0.45).astype(np.int64)
    base = rs.uniform(0.05, 0.65, size=BITS)
    rates = np.clip(np.stack([base, base + rs.normal(0.0, 0.03, BITS)]), 0.05, 0.65)          # close classes: the scores are not all 1
    F = (rs.random((N, BITS)) < rates[y]).astype(np.float64)
    return PCA(n_components=D, svd_solver="full").fit_transform(StandardScaler().fit_transform(F)), y


def _spread(times):
    import numpy as np
    q = np.percentile(times, [0, 25, 50, 75, 100])
    return {"median_s": float(q[2]), "min_s": float(q[0]), "q1_s": float(q[1]), "q3_s": float(q[3]), "max_s": float(q[4]), "reps": len(times)}


def _timed(fn, reps, warmup, sync):
    out = None
    for _ in range(warmup):
        out = fn()
    sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append(time.perf_counter() - t0)
    return _spread(times), out


def step_gpu(reps):
    import numpy as np
    import torch
    from bbbp_amd import naive_bayes as NB
    X, y = synth()
    sizes = np.linspace(.1, 1, 5)

    def launches(fn):
        before = dict(NB._LAUNCHES)
        fn()
        return {k: NB._LAUNCHES[k] - before[k] for k in before}

    grid_fn = lambda: NB.grid_search_cv(X, y, GRID, cv=5)  # noqa: E731
    grid_launches = launches(grid_fn)
    grid, (best, scores, _) = _timed(grid_fn, reps, 2, torch.cuda.synchronize)
    curve_fn = lambda: NB.learning_curve(best, X, y, cv=CURVE_CV, train_sizes=sizes, scoring="accuracy")  # noqa: E731
    curve_launches = launches(curve_fn)
    curve, (abs_sizes, train, test) = _timed(curve_fn, reps, 2, torch.cuda.synchronize)
    return {"device": torch.cuda.get_device_name(0), "n": N, "d": D,
            "grid": {**grid, "launches": grid_launches, "best_params": best, "best_f1": max(scores), "points": len(scores)},
            "curve": {**curve, "launches": curve_launches, "sizes": [int(s) for s in abs_sizes], "test_mean": [float(v) for v in test.mean(axis=1)],
                      "train_mean": [float(v) for v in train.mean(axis=1)]}}


def sklearn_rows():
    import numpy as np
    import sklearn
    from sklearn.model_selection import GridSearchCV, learning_curve
    from sklearn.naive_bayes import BernoulliNB
    X, y = synth()
    grid, gs = _timed(lambda: GridSearchCV(BernoulliNB(), GRID, cv=5, scoring="f1", n_jobs=1).fit(X, y), 5, 1, lambda: None)
    curve, (abs_sizes, train, test) = _timed(lambda: learning_curve(gs.best_estimator_, X, y, cv=CURVE_CV, train_sizes=np.linspace(.1, 1, 5),
                                                                    n_jobs=1), 5, 1, lambda: None)
    return {"version": sklearn.__version__, "n_jobs": 1, "host_cpus": os.cpu_count(),
            "grid": {**grid, "best_params": gs.best_params_, "best_f1": float(gs.best_score_)},
            "curve": {**curve, "sizes": [int(s) for s in abs_sizes], "test_mean": [float(v) for v in test.mean(axis=1)],
                      "train_mean": [float(v) for v in train.mean(axis=1)]}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--reps", type=int, default=15, help="timed calls per GPU figure")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)      # child mode: run the GPU step and print its JSON line
    a = ap.parse_args()
    if not 3 <= a.reps <= 1000:
        ap.error("--reps within 3..1000")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.reps)), flush=True)
        return 0
    result = {"bench": "bnb"}
    rc = 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(a.reps)], capture_output=True, text=True, timeout=LIMIT_S)
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_bnb] gpu: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
        else:
            result["gpu"] = json.loads(got[-1])
    except subprocess.TimeoutExpired:
        print(f"[bench_bnb] gpu: no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    if rc == 0 and not a.no_sklearn:
        result["sklearn"] = sklearn_rows()
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
