#!/usr/bin/env python3
"""Times preprocessing.StandardScaler and preprocessing.PolynomialFeatures on the GPU beside scikit-learn on the host.

    python tools/bench_preprocessing.py [--out FILE] [--no-host] [--reps R]

The workloads are the reference's: ``StandardScaler().fit_transform`` on the fingerprint table (7 807 x 167, Models/model_opt_maccs.py), on
a 2 048-bit fingerprint table (7 807 x 2 048) and on the fused fingerprint + image table of the regression scripts (1 058 x 49 319); and
``PolynomialFeatures(2, interaction_only=True, include_bias=False)`` on the 60 joined components (1 058 x 60 -> 1 830 columns,
Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest_fixed_1.py) and ``PolynomialFeatures(2, include_bias=False)`` on
7 807 x 100 -> 5 150 columns.  The matrices are seeded normal float64.

* gpu: every call from a host array (upload, the calls, download) and from a device tensor (the result stays on the device).  Each is an
  end-to-end call time: wall time behind a device synchronise, after two warm-up calls, the median of --reps calls (default 15) with the
  fastest, the slowest and the quartiles; the whole measurement is run twice, so that the spread is on record.  ``launches`` counts the
  library's entry points per call.
* kernels: ``bbbp_scaler_apply`` and ``bbbp_poly_expand`` alone, between device events, 20 launches per window, the median of --reps
  windows; the bytes each moves (input read once, output written once, the table for the expansion) over that time, beside a
  ``torch`` device-to-device copy that moves the same number of bytes (half read, half written), measured the same way in the same run.
  Outputs of more than the Infinity Cache (256 MiB) run from HBM; smaller ones may not.
* host: scikit-learn's two estimators on the same matrices on this machine's CPU, the median of five after one warm-up.  The GPU results
  are compared with them bit for bit.

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

LIMIT_S = 400
SCALER_SHAPES = [(7807, 167), (7807, 2048), (1058, 49319)]
# (n, d, interaction_only): degree 2, no bias
POLY_SHAPES = [(1058, 60, True), (7807, 100, False)]
KERNEL_LAUNCHES = 20


def matrix(n, d):
    import numpy as np
    rng = np.random.RandomState(n + d)
    return rng.standard_normal((n, d)) * 3.0 + rng.uniform(-5, 5, size=d)


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


def _sha1(a):
    import hashlib
    import numpy as np
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _event_windows(fn, reps):
    """Seconds per call of ``fn`` between device events: the median over ``reps`` windows of KERNEL_LAUNCHES calls, after one window."""
    import torch
    times = []
    for w in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(KERNEL_LAUNCHES):
            fn()
        b.record()
        b.synchronize()
        if w:
            times.append(a.elapsed_time(b) * 1e-3 / KERNEL_LAUNCHES)
    return _spread(times)


def _beside_a_copy(kernel, nbytes, reps):
    """The kernel's seconds and bytes per second beside a device copy that moves the same number of bytes."""
    import torch
    src = torch.empty(nbytes // 16, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    out = {"bytes": int(nbytes), "kernel": _event_windows(kernel, reps), "torch_copy": _event_windows(lambda: dst.copy_(src), reps)}
    out["kernel_bytes_per_s"] = nbytes / out["kernel"]["median_s"]
    out["torch_copy_bytes_per_s"] = (nbytes // 16) * 16 / out["torch_copy"]["median_s"]
    return out


def step_gpu(reps):
    import torch
    from bbbp_amd import _dense, _lib, preprocessing as PP
    L = _lib.lib()
    out = {"device": torch.cuda.get_device_name(0), "scaler": {}, "poly": {}}
    sync = torch.cuda.synchronize
    for n, d in SCALER_SHAPES:
        X = matrix(n, d)
        Xt = torch.from_numpy(X).cuda()
        before = dict(PP._LAUNCHES)
        s = PP.StandardScaler()
        s.fit_transform(Xt)
        launches = {k: PP._LAUNCHES[k] - before[k] for k in before}
        runs = []
        for _ in range(2):                                   # the whole measurement twice
            host, res = _timed(lambda: PP.StandardScaler().fit_transform(X), reps, 2, sync)
            device, res_t = _timed(lambda: PP.StandardScaler().fit_transform(Xt), reps, 2, sync)
            fit_only, _ = _timed(lambda: PP.StandardScaler().fit(Xt), reps, 2, sync)
            runs.append({"from_host_array": host, "from_device_tensor": device, "fit_from_device_tensor": fit_only})
        assert _sha1(res) == _sha1(res_t.cpu().numpy())
        dst = torch.empty_like(Xt)
        apply = lambda: _lib.check(L.bbbp_scaler_apply(_dense.stream(), Xt.data_ptr(), d, n, d, s._mean_d.data_ptr(), s._scale_d.data_ptr(), 0,  # noqa: E731
                                                       dst.data_ptr(), d, None), "bbbp_scaler_apply")
        out["scaler"][f"{n}x{d}"] = {"launches": launches, "runs": runs, "sha1": _sha1(res), "apply_kernel": _beside_a_copy(apply, 2 * n * d * 8, reps)}
    for n, d, interaction_only in POLY_SHAPES:
        X = matrix(n, d)
        Xt = torch.from_numpy(X).cuda()
        make = lambda: PP.PolynomialFeatures(2, interaction_only=interaction_only, include_bias=False)  # noqa: E731
        before = dict(PP._LAUNCHES)
        p = make()
        first = p.fit_transform(Xt)
        launches = {k: PP._LAUNCHES[k] - before[k] for k in before}
        P = p.n_output_features_
        runs = []
        for _ in range(2):
            host, res = _timed(lambda: make().fit_transform(X), reps, 2, sync)
            device, res_t = _timed(lambda: make().fit_transform(Xt), reps, 2, sync)
            transform_only, _ = _timed(lambda: p.transform(Xt), reps, 2, sync)
            runs.append({"from_host_array": host, "from_device_tensor": device, "transform_from_device_tensor": transform_only})
        assert _sha1(res) == _sha1(res_t.cpu().numpy())
        expand = lambda: _lib.check(L.bbbp_poly_expand(_dense.stream(), Xt.data_ptr(), d, n, d, p._table_d.data_ptr(), P, first.data_ptr(), P, None),  # noqa: E731
                                    "bbbp_poly_expand")
        out["poly"][f"{n}x{d}"] = {"columns": P, "launches": launches, "runs": runs, "sha1": _sha1(res),
                                   "expand_kernel": _beside_a_copy(expand, n * d * 8 + n * P * 8 + P * 12, reps)}
    return out


def host_rows():
    import numpy
    import sklearn
    from sklearn.preprocessing import PolynomialFeatures, StandardScaler
    out = {"numpy": numpy.__version__, "sklearn": sklearn.__version__, "host_cpus": os.cpu_count(), "scaler": {}, "poly": {}}
    for n, d in SCALER_SHAPES:
        X = matrix(n, d)
        t, res = _timed(lambda: StandardScaler().fit_transform(X), 5, 1, lambda: None)
        out["scaler"][f"{n}x{d}"] = {**t, "sha1": _sha1(res)}
    for n, d, interaction_only in POLY_SHAPES:
        X = matrix(n, d)
        t, res = _timed(lambda: PolynomialFeatures(2, interaction_only=interaction_only, include_bias=False).fit_transform(X), 5, 1, lambda: None)
        out["poly"][f"{n}x{d}"] = {**t, "columns": int(res.shape[1]), "sha1": _sha1(res)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-host", action="store_true", help="skip scikit-learn on the host")
    ap.add_argument("--reps", type=int, default=15, help="timed calls per GPU figure")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)      # child mode: run the GPU step and print its JSON line
    a = ap.parse_args()
    if not 3 <= a.reps <= 1000:
        ap.error("--reps within 3..1000")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.reps)), flush=True)
        return 0
    result = {"bench": "preprocessing"}
    rc = 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(a.reps)], capture_output=True, text=True, timeout=LIMIT_S)
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_preprocessing] gpu: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
        else:
            result["gpu"] = json.loads(got[-1])
    except subprocess.TimeoutExpired:
        print(f"[bench_preprocessing] gpu: no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    if rc == 0 and not a.no_host:
        result["host"] = host_rows()
        result["equal_results"] = {kind: {k: result["host"][kind][k]["sha1"] == result["gpu"][kind][k]["sha1"] for k in result["host"][kind]}
                                   for kind in ("scaler", "poly")}
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
