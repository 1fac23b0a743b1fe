#!/usr/bin/env python3
"""Times decomposition.PCA on the GPU, phase by phase, beside scikit-learn on the same host.

    python tools/bench_pca.py [--out FILE] [--no-sklearn] [--repeat R]

Fits: [1058, 49152] -> 128 (the image matrix), [1058, 167] -> 64 (fingerprints), [7807, 167] -> 100 (the MLP grid's input);
transform: [4096, 49152] -> 128.  Per fit the phases are timed separately: column means, Gram / covariance product, device-to-host copy +
numpy.linalg.eigh, components product (Gram regime).  Device phases are timed with HIP events around R back-to-back calls after a warm-up;
the host phase with a host clock around work that ends in a synchronise.  Beside each time: the HBM floor of the product (bytes of X read
once at 6.29 TB/s measured / 8.0 TB/s spec copy bandwidth) and the float64 operations.

Every GPU step runs in a child process of its own under a time limit; after a step that fails or runs out of time nothing more is started
on the GPU.  Data is seeded and generated on the device; nothing outside this repository is read.  Prints one JSON line per step.
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

FITS = {"fit_image": (1058, 49152, 128), "fit_fingerprint": (1058, 167, 64), "fit_mlp_grid": (7807, 167, 100)}
TRANSFORMS = {"transform_image": (4096, 49152, 128)}
LIMIT_S = {"fit_image": 240, "fit_fingerprint": 120, "fit_mlp_grid": 120, "transform_image": 240}
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def synth(n, d, seed, device):
    """Seeded float32 [n, d]: 64 decaying directions + noise + a per-column offset (the shape of the tests' matrices)."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    r = min(64, n, d)
    s = 10.0 * 0.9 ** torch.arange(r, device=device, dtype=torch.float32)
    X = (torch.randn(n, r, generator=g, device=device) * s) @ torch.randn(r, d, generator=g, device=device) / r ** 0.5
    return X + 1e-3 * torch.randn(n, d, generator=g, device=device) + 3.0 * torch.randn(d, generator=g, device=device)


def event_ms(fn, repeat, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeat


def step_fit(name, repeat):
    import numpy as np
    import torch
    from bbbp_amd import _lib
    from bbbp_amd import decomposition as D
    n, d, k = FITS[name]
    dev = torch.device("cuda:0")
    X = synth(n, d, 1, dev)
    L = _lib.lib()
    small = min(n, d)
    mean_d = torch.empty(d, dtype=torch.float64, device=dev)
    S = torch.empty((small, small), dtype=torch.float64, device=dev)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    mean = lambda: _lib.check(L.bbbp_pca_col_mean(st(), X.data_ptr(), 0, n, d, d, mean_d.data_ptr()), "col_mean")  # noqa: E731
    if d <= n:
        prod = lambda: D._gemm_f64c(D._TN, d, d, n, X, d, X, d, S, mean_d, mean_d, symmetric=True)  # noqa: E731
    else:
        prod = lambda: D._gemm_f64c(D._NT, n, n, d, X, d, X, d, S, mean_d, mean_d, symmetric=True)  # noqa: E731
    res = {"step": name, "n": n, "d": d, "k": k, "regime": "covariance" if d <= n else "gram", "repeat": repeat}
    res["mean_ms"] = event_ms(mean, repeat)
    res["product_ms"] = event_ms(prod, repeat)
    torch.cuda.synchronize()
    host = []
    for _ in range(max(2, repeat // 2)):
        t0 = time.perf_counter()
        lam, vec = np.linalg.eigh(S.cpu().numpy())
        host.append((time.perf_counter() - t0) * 1e3)
    res["copy_eigh_ms"] = sorted(host)[len(host) // 2]
    if d > n:
        lam, vec = lam[::-1][:k], vec[:, ::-1][:, :k]
        U = torch.from_numpy(np.ascontiguousarray(vec)).to(dev)
        inv = torch.from_numpy(1.0 / np.sqrt(np.maximum(lam, 1e-300))).to(dev)
        comp = torch.empty((k, d), dtype=torch.float64, device=dev)
        res["components_ms"] = event_ms(lambda: D._gemm_f64c(D._TN, k, d, n, U, k, X, d, comp, None, mean_d, row_scale=inv), repeat)
    else:
        res["components_ms"] = 0.0
    # whole fit through the public interface (includes the small copies and the sign pass), host clock around synchronised work
    whole = []
    for _ in range(max(3, repeat // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.PCA(k).fit(X)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    res["fit_wall_ms"] = sorted(whole)[len(whole) // 2]
    x_bytes = 4.0 * n * d
    res["x_bytes"] = x_bytes
    res["hbm_floor_ms_measured_bw"] = x_bytes / HBM_MEASURED * 1e3
    res["hbm_floor_ms_spec_bw"] = x_bytes / HBM_SPEC * 1e3
    res["product_fraction_of_hbm_floor"] = res["hbm_floor_ms_measured_bw"] / res["product_ms"]
    res["product_f64_flop"] = 1.0 * small * (small + 1) * max(n, d)            # lower triangle only
    res["product_tflops"] = res["product_f64_flop"] / res["product_ms"] / 1e9
    res["eigh_share_of_fit"] = res["copy_eigh_ms"] / res["fit_wall_ms"]
    return res


def step_transform(name, repeat):
    import torch
    from bbbp_amd import decomposition as D
    m, d, k = TRANSFORMS[name]
    dev = torch.device("cuda:0")
    X = synth(m, d, 2, dev)
    p = D.PCA(k).fit(X[:1058])
    ms = event_ms(lambda: p.transform(X), repeat)
    x_bytes = 4.0 * m * d
    floor = x_bytes / HBM_MEASURED * 1e3
    return {"step": name, "m": m, "d": d, "k": k, "repeat": repeat, "transform_ms": ms, "x_bytes": x_bytes, "hbm_floor_ms_measured_bw": floor,
            "hbm_floor_ms_spec_bw": x_bytes / HBM_SPEC * 1e3, "fraction_of_hbm_floor": floor / ms, "tflops": 2.0 * m * d * k / ms / 1e9}


def sklearn_times():
    """scikit-learn on this host, same shapes, float64 input as the reference feeds it; `randomized` seeded so the run is repeatable."""
    import numpy as np
    from sklearn.decomposition import PCA
    out = []
    for name, (n, d, k) in FITS.items():
        rs = np.random.RandomState(1)
        r = min(64, n, d)
        X = (rs.randn(n, r) * (10.0 * 0.9 ** np.arange(r))) @ rs.randn(r, d) / r ** 0.5 + 1e-3 * rs.randn(n, d) + 3.0 * rs.randn(d)
        row = {"step": "sklearn_" + name, "n": n, "d": d, "k": k}
        for solver in ("randomized", "full"):
            t0 = time.perf_counter()
            est = PCA(k, svd_solver=solver, random_state=0).fit(X)
            row[solver + "_fit_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        est.transform(X)
        row["transform_ms"] = (time.perf_counter() - t0) * 1e3
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--step", help=argparse.SUPPRESS)                 # child mode: run one GPU step and print its JSON line
    a = ap.parse_args()
    if a.step:
        res = step_fit(a.step, a.repeat) if a.step in FITS else step_transform(a.step, a.repeat)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    lines = []
    rc = 0
    for name in list(FITS) + list(TRANSFORMS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--repeat", str(a.repeat)],
                               capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"[bench_pca] {name}: no result within {LIMIT_S[name]} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_pca] {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
            break
        lines.append(json.loads(got[-1]))
        print(got[-1], flush=True)
    if rc == 0 and not a.no_sklearn:
        for row in sklearn_times():
            lines.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
