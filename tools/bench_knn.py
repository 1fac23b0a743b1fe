#!/usr/bin/env python3
"""Times neighbors.NearestNeighbors.kneighbors on the GPU beside what the project could do without it, and scikit-learn on the host.

    python tools/bench_knn.py [--out FILE] [--no-sklearn] [--repeat R]

Shapes: `fold` -- the reference's cross-validation fold, train [8000, 100], 2000 queries, k = 7; `screen` -- train [10000, 100], 2^20
queries in chunks of 2^17, k = 7.  Float64 throughout (the PCA features the classifier stack feeds its learners).  Per shape:

* fused: bbbp_knn_row_norms of the queries + bbbp_knn_f64 (search, merge, refine), the lists of one chunk written in place;
* unfused: decomposition.gemm_f64c of the centred operands into a materialised [chunk, n] float64 matrix, the norms added, torch.topk --
  what the parent of this feature could do.  Its matrix is written once and read twice (8 m n bytes each way);
* scikit-learn NearestNeighbors(algorithm="brute") on the host's CPUs (on at most 2^15 of the screen queries, scaled to the full count).

Device times: HIP events around one whole pass over the queries, after a warm-up pass, the median of R passes.  Beside each time:
2 m n d / t as a fraction of the float64 matrix peak (78.6 TFLOP/s, the MI355X specification), and the HBM bytes the plan moves: operands
once per (query tile, slice), norms, lists -- against 8 m n bytes each way for the unfused matrix.

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

SHAPES = {"fold": (8000, 2000, 100, 7, 2000), "screen": (10000, 1 << 20, 100, 7, 1 << 17)}      # n, m, d, k, queries per chunk
LIMIT_S = {"fold": 180, "screen": 420}
F64_MFMA_PEAK = 78.6e12


def synth(n, d, seed, device):
    """Seeded float64 [n, d]: anisotropic Gaussian (column scales 3 .. 0.3) plus a per-column offset, the shape of the tests' point sets."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    off = torch.randn(d, generator=torch.Generator(device=device).manual_seed(99), device=device, dtype=torch.float64)
    return torch.randn(n, d, generator=g, device=device, dtype=torch.float64) * torch.linspace(3.0, 0.3, d, device=device, dtype=torch.float64) + off


def median_pass_ms(fn, repeat):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def plan_bytes(n, m, d, k, chunk, slices):
    """HBM bytes of the fused path from its plan: both operands once per (query tile, slice) pair at worst (the training rows of a slice
    are shared through L2 by the tiles that run together, so this is an upper bound), norms, partial lists, final lists twice (refine)."""
    tiles = -(-chunk // 64) * (m // chunk)
    operands = 8.0 * d * (tiles * slices * 64 + tiles * n)
    lists = 12.0 * m * k * (slices if slices > 1 else 0) * 2 + 16.0 * m * k * 3
    return operands + 8.0 * (m + tiles * n) + lists + 8.0 * m * d          # + the norm pass reading the queries once more


def step(name, repeat):
    import ctypes
    import torch
    from bbbp_amd import _lib
    from bbbp_amd import decomposition as D
    from bbbp_amd.neighbors import NearestNeighbors
    n, m, d, k, chunk = SHAPES[name]
    dev = torch.device("cuda:0")
    T, Q = synth(n, d, 1, dev), synth(m, d, 2, dev)
    nn = NearestNeighbors(k).fit(T)
    desc = _lib.KnnDesc(m=chunk, n=n, d=d, k=k, q_dtype=1, t_dtype=1, ldq=d, ldt=d)
    ws = _lib.lib().bbbp_knn_workspace_bytes(ctypes.byref(desc))
    slices = ws // (chunk * k * 12) if ws else 1
    keep = {}

    def fused():
        for c in range(0, m, chunk):
            keep["fused"] = nn._search(Q[c:c + chunk], k)

    tn = nn._norms_d
    mu = nn._mean_d

    def unfused():
        for c in range(0, m, chunk):
            Qc = Q[c:c + chunk]
            G = D.gemm_f64c(Qc, T, a_shift=mu, b_shift=mu)
            qn = ((Qc - mu) ** 2).sum(dim=1)
            G.mul_(-2.0).add_(qn[:, None]).add_(tn[None, :])
            keep["unfused"] = torch.topk(G, k, dim=1, largest=False, sorted=True)

    res = {"step": name, "n": n, "m": m, "d": d, "k": k, "chunk": chunk, "slices": int(slices), "repeat": repeat}
    res["fused_ms"] = median_pass_ms(fused, repeat)
    res["unfused_ms"] = median_pass_ms(unfused, repeat)
    # same neighbours from both paths on the last chunk (the unfused order among exact ties is torch.topk's)
    res["indices_equal_fraction"] = float((keep["fused"][1] == keep["unfused"][1]).double().mean().item())
    flop = 2.0 * m * n * d
    res["fused_fraction_of_f64_mfma_peak"] = flop / (res["fused_ms"] * 1e-3) / F64_MFMA_PEAK
    res["unfused_fraction_of_f64_mfma_peak"] = flop / (res["unfused_ms"] * 1e-3) / F64_MFMA_PEAK
    res["fused_hbm_bytes_plan"] = plan_bytes(n, m, d, k, chunk, int(slices))
    res["unfused_matrix_bytes"] = 8.0 * m * n * 3            # written by the product, read and rewritten by the norm pass, read by topk
    res["fused_over_unfused"] = res["unfused_ms"] / res["fused_ms"]
    return res


def sklearn_times():
    import numpy as np
    from sklearn.neighbors import NearestNeighbors as SkNN
    out = []
    for name, (n, m, d, k, _) in SHAPES.items():
        rs = np.random.RandomState(1)
        scale, off = np.linspace(3.0, 0.3, d), rs.randn(d)
        T = rs.randn(n, d) * scale + off
        mq = min(m, 1 << 15)
        Q = rs.randn(mq, d) * scale + off
        est = SkNN(n_neighbors=k, algorithm="brute").fit(T)
        t0 = time.perf_counter()
        est.kneighbors(Q)
        ms = (time.perf_counter() - t0) * 1e3
        out.append({"step": "sklearn_" + name, "n": n, "m": m, "d": d, "k": k, "queries_timed": mq, "kneighbors_ms_scaled_to_m": ms * m / mq,
                    "host_cpus": os.cpu_count()})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--step", help=argparse.SUPPRESS)                 # child mode: run one GPU step and print its JSON line
    a = ap.parse_args()
    if a.repeat < 5:
        ap.error("--repeat must be at least 5 (the median of fewer passes is not reported)")
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.repeat)), flush=True)
        return 0
    lines = []
    rc = 0
    for name in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--repeat", str(a.repeat)],
                               capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"[bench_knn] {name}: no result within {LIMIT_S[name]} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_knn] {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
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
