#!/usr/bin/env python3
"""Times imbalance.SMOTE and imbalance.SMOTETomek on the GPU beside their numpy restatement on one core of the host.

    python tools/bench_smote.py [--out FILE] [--no-host] [--reps R]

The workload is the reference's resampling step (Models/model_opt_maccs.py: ``SMOTE(random_state=42).fit_resample(X_reduced, y)``;
model_opt_20250130.py: ``SMOTETomek(random_state=42)``) at B3DB's shape: a seeded synthetic [7 807, 100] float64 matrix
(``tests/knn_oracle.make_points``) with 2 851 minority rows shifted by +0.5, so 2 105 synthetic rows are made.

* gpu: ``SMOTE(random_state=42).fit_resample`` and ``SMOTETomek(random_state=42).fit_resample`` from a host array (upload, the calls,
  download) and from a device tensor (``X_res`` stays on the device; ``y_res`` is a host array either way).  Each is an end-to-end call
  time: wall time behind a device synchronise, after two warm-up calls, the median of --reps calls (default 15) with the fastest, the
  slowest and the quartiles, and the whole measurement is run twice, so that the spread is on record.  ``launches`` counts the library's
  entry points per call: fits (column mean + row norms: the NaN check and the search's set-up), searches (two or three kernels each), the
  synthesis and the Tomek kernel.  ``synth_bytes`` is what the synthesis kernel moves: per synthetic row two rows read, one written, plus
  its index, step and neighbour entry.
* host: the same two calls as the numpy restatement -- imbalanced-learn's algorithm, which is not installed here -- with
  ``sklearn.neighbors.NearestNeighbors`` for the searches, on one core: the median of five after one warm-up.  The GPU results are
  compared with it: equal row counts and labels; rows equal bit for bit when both searches pick the same neighbours.

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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LIMIT_S = 300
N, D, N_MIN, SEED, K, RANDOM_STATE = 7807, 100, 2851, 1, 5, 42


def synth():
    import numpy as np
    import knn_oracle
    X = knn_oracle.make_points(N, D, SEED)
    y = np.zeros(N, dtype=np.int64)
    y[np.random.RandomState(SEED + 5).permutation(N)[:N_MIN]] = 1
    X[y == 1] += 0.5
    return X.astype(np.float32).astype(np.float64), y


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


def _digest(X_res, y_res):
    import hashlib
    import numpy as np
    X_res = np.ascontiguousarray(X_res)
    return {"rows": int(len(y_res)), "counts": [int(c) for c in np.bincount(y_res)], "sha1": hashlib.sha1(X_res.tobytes()).hexdigest()}


def step_gpu(reps):
    import torch
    from bbbp_amd import imbalance as IM
    X, y = synth()
    Xt = torch.from_numpy(X).cuda()
    n_new = N - 2 * N_MIN
    out = {"device": torch.cuda.get_device_name(0), "n": N, "d": D, "n_min": N_MIN, "n_new": n_new,
           "synth_bytes": n_new * (3 * D * 8 + 8 + 8 + 8)}
    makers = {"smote": lambda: IM.SMOTE(random_state=RANDOM_STATE), "smote_tomek": lambda: IM.SMOTETomek(random_state=RANDOM_STATE)}
    for name, make in makers.items():
        before = dict(IM._LAUNCHES)
        make().fit_resample(X, y)
        launches = {k: IM._LAUNCHES[k] - before[k] for k in before}
        runs = []
        for _ in range(2):                                   # the whole measurement twice
            host, res = _timed(lambda: make().fit_resample(X, y), reps, 2, torch.cuda.synchronize)
            device, res_t = _timed(lambda: make().fit_resample(Xt, y), reps, 2, torch.cuda.synchronize)
            runs.append({"from_host_array": host, "from_device_tensor": device})
        assert _digest(res_t[0].cpu().numpy(), res_t[1]) == _digest(*res)
        out[name] = {"launches": launches, "runs": runs, "result": _digest(*res)}
    return out


def restated_smote(X, y):
    import numpy as np
    from sklearn.neighbors import NearestNeighbors
    Xc = X[y == 1]
    nn = NearestNeighbors(n_neighbors=K + 1, algorithm="brute").fit(Xc).kneighbors(Xc, return_distance=False)[:, 1:]
    rs = np.random.RandomState(RANDOM_STATE)
    n_new = int((y == 0).sum() - (y == 1).sum())
    idx = rs.randint(0, len(Xc) * K, size=n_new)
    steps = rs.uniform(size=n_new)
    rows, cols = idx // K, idx % K
    X_new = Xc[rows] + steps[:, None] * (Xc[nn[rows, cols]] - Xc[rows])
    return np.vstack([X, X_new]), np.concatenate([y, np.ones(n_new, dtype=y.dtype)])


def restated_smote_tomek(X, y):
    import numpy as np
    from sklearn.neighbors import NearestNeighbors
    X_res, y_res = restated_smote(X, y)
    nn1 = NearestNeighbors(n_neighbors=2, algorithm="brute").fit(X_res).kneighbors(X_res, return_distance=False)[:, 1]
    member = (y_res[nn1] != y_res) & (nn1[nn1] == np.arange(len(y_res)))
    return X_res[~member], y_res[~member]


def host_rows():
    import numpy
    import sklearn
    from threadpoolctl import threadpool_limits              # scikit-learn's own dependency: BLAS and OpenMP pools down to one thread
    X, y = synth()
    out = {"numpy": numpy.__version__, "sklearn": sklearn.__version__, "threads": 1, "host_cpus": os.cpu_count()}
    with threadpool_limits(limits=1):
        for name, fn in (("smote", restated_smote), ("smote_tomek", restated_smote_tomek)):
            t, res = _timed(lambda: fn(X, y), 5, 1, lambda: None)
            out[name] = {**t, "result": _digest(*res)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement on the host")
    ap.add_argument("--reps", type=int, default=15, help="timed calls per GPU figure")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)      # child mode: run the GPU step and print its JSON line
    a = ap.parse_args()
    if not 3 <= a.reps <= 1000:
        ap.error("--reps within 3..1000")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.reps)), flush=True)
        return 0
    result = {"bench": "smote"}
    rc = 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(a.reps)], capture_output=True, text=True, timeout=LIMIT_S)
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_smote] gpu: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
        else:
            result["gpu"] = json.loads(got[-1])
    except subprocess.TimeoutExpired:
        print(f"[bench_smote] gpu: no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    if rc == 0 and not a.no_host:
        result["host"] = host_rows()
        result["equal_results"] = {k: result["host"][k]["result"] == result["gpu"][k]["result"] for k in ("smote", "smote_tomek")}
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
