#!/usr/bin/env python3
"""Times isolation_forest.IsolationForest on the GPU beside scikit-learn on one core of the host.

    python tools/bench_iforest.py [--out FILE] [--no-sklearn] [--reps R]

The workloads are the reference's outlier step behind PCA (Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest*.py):
``IsolationForest(contamination=0.05, random_state=42)`` -- 100 trees of 256 rows -- on the 30 + 30 PCA columns of 1 058 and of 7 807
molecules, here seeded synthetic data (standard normal, 5 % of the rows spread four times wider).

* fit: ``fit(X)`` with X resident on the device, as ``decomposition.PCA`` leaves it: the one fit launch, the read-back of the node arrays,
  the path terms on the host, the upload and the scoring pass over the training rows that gives ``offset_``.
* fit_numpy: the same from a host array (adds the upload of X).
* score: ``score_samples(X)`` of the fitted model on the device-resident rows: one launch, m doubles read back, the last step in numpy.
  Each is wall time behind a device synchronise, after two warm-up calls: the median of --reps calls (default 15), with the fastest, the
  slowest and the quartiles, so that the spread is on record.  The workload is small and latency-bound: a call is a handful of launches
  and copies.  ``fit_launches`` counts the fit kernel's launches per ``fit``.
* sklearn: the same fit and scoring with scikit-learn on one core (``n_jobs=None``), the median of five after one warm-up.

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
SHAPES = ((1058, 60), (7807, 60))
PARAMS = dict(n_estimators=100, max_samples=256, contamination=0.05, random_state=42)


def synth(n, d, seed=1):
    import numpy as np
    rs = np.random.default_rng(seed)
    X = rs.standard_normal((n, d))
    X[: n // 20] *= 4.0
    return X.astype(np.float32)


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
    import torch
    from bbbp_amd import isolation_forest as F
    rows = []
    for n, d in SHAPES:
        X = synth(n, d)
        Xd = torch.from_numpy(X).cuda()
        make = lambda: F.IsolationForest(**PARAMS)  # noqa: E731
        before = F._GROWN["launches"]
        make().fit(Xd)
        launches = F._GROWN["launches"] - before
        fit, est = _timed(lambda: make().fit(Xd), reps, 2, torch.cuda.synchronize)
        fit_numpy, _ = _timed(lambda: make().fit(X), reps, 2, torch.cuda.synchronize)
        score, s = _timed(lambda: est.score_samples(Xd), reps, 2, torch.cuda.synchronize)
        flags = est.predict(Xd)
        rows.append({"n": n, "d": d, **PARAMS, "fit_launches": launches, "fit": fit, "fit_numpy": fit_numpy, "score": score,
                     "nodes_per_tree": len(est.trees_["left"]) / est.n_estimators_, "outliers": int((flags == -1).sum()),
                     "planted_found": int((flags[: n // 20] == -1).sum())})
    return {"device": torch.cuda.get_device_name(0), "workloads": rows}


def sklearn_rows():
    from sklearn.ensemble import IsolationForest
    rows = []
    for n, d in SHAPES:
        X = synth(n, d)
        fit, sk = _timed(lambda: IsolationForest(**PARAMS).fit(X), 5, 1, lambda: None)
        score, _ = _timed(lambda: sk.score_samples(X), 5, 1, lambda: None)
        flags = sk.predict(X)
        rows.append({"n": n, "d": d, "fit": fit, "score": score, "n_jobs": None, "host_cpus": os.cpu_count(),
                     "nodes_per_tree": sum(e.tree_.node_count for e in sk.estimators_) / len(sk.estimators_), "outliers": int((flags == -1).sum()),
                     "planted_found": int((flags[: n // 20] == -1).sum())})
    import sklearn
    return {"version": sklearn.__version__, "workloads": rows}


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
    result = {"bench": "iforest"}
    rc = 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(a.reps)], capture_output=True, text=True, timeout=LIMIT_S)
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_iforest] gpu: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
        else:
            result["gpu"] = json.loads(got[-1])
    except subprocess.TimeoutExpired:
        print(f"[bench_iforest] gpu: no result within {LIMIT_S} s; stopping", file=sys.stderr)
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
