#!/usr/bin/env python3
"""Times one RMSE curve over all boosting iterations from a staged prediction beside the same curve from truncated models.

    python tools/bench_staged.py [--out FILE] [--family gbt|oblivious|both] [--d 192,49319] [--reps R] [--trees T] [--rows N]

Synthetic trees, no fit: ``T = 300`` trees and ``n = 1 058`` query rows at ``d = 192`` and ``d = 49 319`` features, for both families.
gbt trees are grown as the reference's are (``max_depth=30`` on 1 058 rows: a node splits its rows at a drawn point until a row is alone:
about 2 100 nodes a tree); oblivious trees have depth 10.  The two sides, per (family, d):

* staged: what ``eval_curves`` does per eval set -- ``staged_predict_device(X)`` (two launches) and ``boosters.rmse_curve`` on the ``[T, n]``
  matrix (one ``bbbp_metrics_sq_sums`` launch, one host read).
* truncated: what the API offered before -- for k = 1 .. T, ``truncated(0, k).predict_device(X)`` and ``metrics.regression_scores(y, p)``:
  ``3 T`` launches and ``T`` host reads.  The ``T`` truncated models are built and uploaded before the clock starts; their build time is
  reported on its own.

Both sides are warmed up, then timed alternately: ``--reps`` windows each, a window being ``--calls`` curves behind a device synchronise on a
host clock; the median window per curve and all windows are reported.  The two curves are compared bit for bit.  The launch counts are
those of the code paths (``metrics._LAUNCHES`` counts the ``sq_sums`` launches; the predict entry points launch two kernels per row chunk).

The GPU step of each (family, d) runs in a child process of its own under a time limit; if one fails or runs out of time nothing more is
started on the GPU.  Nothing outside this repository is read.  Prints one JSON line.
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

LIMIT_S = 420


def synth_gbt(T, d, rows, seed):
    """``boosters.XGBTrees`` arrays: every tree splits ``rows`` rows at drawn points until a row is alone."""
    import numpy as np
    rs = np.random.default_rng(seed)
    left, right, feature, cond, root = [], [], [], [], [0]
    for _ in range(T):
        base = len(left)
        counts = [rows]
        i = 0
        while i < len(counts):
            m = counts[i]
            if m > 1:
                a = int(rs.integers(1, m))
                left.append(base + len(counts)); right.append(base + len(counts) + 1)
                counts += [a, m - a]
            else:
                left.append(-1); right.append(-1)
            i += 1
        k = len(counts)
        feature.append(rs.integers(0, d, size=k)); cond.append(rs.standard_normal(k).astype(np.float32))
        root.append(base + k)
    left, right = np.asarray(left, np.int32), np.asarray(right, np.int32)
    feature = np.where(left >= 0, np.concatenate(feature), 0).astype(np.int32)
    cond = np.concatenate(cond)
    cond[left < 0] *= 0.01                                        # leaf values of a learning rate's size
    return left, right, feature, cond, np.zeros(len(left), np.uint8), np.asarray(root, np.int32)


def synth_oblivious(T, d, depth, seed):
    import numpy as np
    rs = np.random.default_rng(seed)
    return (rs.integers(0, d, size=T * depth).astype(np.int32), rs.standard_normal(T * depth).astype(np.float32), np.zeros(d, np.uint8),
            (np.arange(T + 1) * depth).astype(np.int32), (np.arange(T, dtype=np.int64) << depth), 0.01 * rs.standard_normal(T << depth))


def step_gpu(family, d, T, n, reps, calls):
    import numpy as np
    import torch
    from bbbp_amd import boosters, metrics
    rs = np.random.default_rng(7)
    X = torch.from_numpy(rs.standard_normal((n, d)).astype(np.float32)).cuda()
    y = rs.standard_normal(n)
    t0 = time.perf_counter()
    if family == "gbt":
        trees = boosters.XGBTrees(*synth_gbt(T, d, n, seed=3), d, 0.5)
    else:
        trees = boosters.CatBoostTrees(*synth_oblivious(T, d, 10, seed=3), d, 1.0, 0.5)
    synth_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    parts = [trees.truncated(0, k) for k in range(1, T + 1)]
    for p in parts:
        p._on_device()
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    def staged():
        return boosters.rmse_curve(trees.staged_predict_device(X), y)

    def truncated():
        return [float(np.sqrt(metrics.regression_scores(y, p.predict_device(X))["MSE"][0, 0])) for p in parts]

    def window(fn, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / count, out

    before = metrics._LAUNCHES["sq_sums"]
    a = staged()
    staged_sq = metrics._LAUNCHES["sq_sums"] - before
    before = metrics._LAUNCHES["sq_sums"]
    b = truncated()
    truncated_sq = metrics._LAUNCHES["sq_sums"] - before
    same = bool(np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)))
    staged_s, truncated_s = [], []
    for _ in range(reps):                                         # alternating: other work shares the machine
        staged_s.append(window(staged, calls)[0])
        truncated_s.append(window(truncated, 1)[0])
    walk_s = window(lambda: trees.staged_predict_device(X), calls)[0]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"family": family, "d": d, "T": T, "n": n, "K": len(a), "nodes": int(len(trees.arrays.get("left", ()))), "curves_equal_bit_for_bit": same,
            "staged_ms": 1e3 * med(staged_s), "staged_ms_all": [1e3 * v for v in staged_s], "staged_predict_only_ms": 1e3 * walk_s,
            "truncated_ms": 1e3 * med(truncated_s), "truncated_ms_all": [1e3 * v for v in truncated_s], "ratio": med(truncated_s) / med(staged_s),
            "launches": {"staged": 2 + staged_sq, "truncated": 2 * T + truncated_sq}, "host_reads": {"staged": 1, "truncated": T},
            "truncated_models_build_s": build_s, "synth_s": synth_s, "calls_per_window": calls, "rmse_first_last": [a[0], a[-1]]}


def _child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=LIMIT_S)
    got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print(f"[bench_staged] {' '.join(args)}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return r.returncode or 1, None
    return 0, json.loads(got[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--family", choices=("gbt", "oblivious", "both"), default="both")
    ap.add_argument("--d", default="192,49319", help="feature counts, comma separated")
    ap.add_argument("--trees", type=int, default=300)
    ap.add_argument("--rows", type=int, default=1058)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50, help="staged curves per timed window")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)      # child mode: one (family, d) and its JSON line
    a = ap.parse_args()
    widths = [int(v) for v in a.d.split(",")]
    if a.reps < 1 or a.calls < 1 or a.trees < 1 or a.rows < 2 or min(widths) < 1:
        ap.error("--reps, --calls, --trees and --d at least 1, --rows at least 2")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.family, widths[0], a.trees, a.rows, a.reps, a.calls)), flush=True)
        return 0
    result, rc = {"bench": "staged", "runs": []}, 0
    for family in (("gbt", "oblivious") if a.family == "both" else (a.family,)):
        for d in widths:
            try:
                rc, got = _child(["--step", "--family", family, "--d", str(d), "--trees", str(a.trees), "--rows", str(a.rows), "--reps", str(a.reps),
                                  "--calls", str(a.calls)])
            except subprocess.TimeoutExpired:
                print(f"[bench_staged] {family} d = {d}: no result within {LIMIT_S} s; stopping", file=sys.stderr)
                rc = 124
            if rc:
                break
            result["runs"].append(got)
        if rc:
            break
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
