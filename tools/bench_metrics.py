#!/usr/bin/env python3
"""Times bbbp_amd.metrics on the GPU beside scikit-learn's functions on one core of the host.

    python tools/bench_metrics.py [--out FILE] [--no-sklearn] [--reps R]

Seeded synthetic predictions at the reference's shapes (7 807 molecules in the classification table, 20 % held out; 6 246 training rows
under five folds; 1 058 rows in the regression table):

* table: ``evaluate_model``'s eight scores for 10 models on 1 562 test rows -- ``metrics.classification_scores(y, pred[10, n],
  proba[10, n])``: one confusion launch, one pair launch and its sum pass, one host read.
* grid_f1 / grid_all: a grid's worth of cross-validated predictions, 144 columns x 5 folds on 6 246 rows (row i carries the prediction of
  the fold that held it out): F1 only (``confusion_counts`` with ``groups`` and ``scores_from_counts``: one launch) and all eight
  (three launches).
* regression: MSE and R2 for 5 folds on 1 058 rows, ``metrics.regression_scores``: one launch.
  Each is an end-to-end call time: wall time behind a device synchronise, after two warm-up calls, the median of --reps calls (default
  15) with the fastest, the slowest and the quartiles; once from host arrays (uploads included) and once from device tensors.  The whole
  GPU step runs twice, in two child processes, so that the run-to-run spread is on record.  The calls are latency-bound; ``launches``
  counts the kernels' launches per call.
* pair_kernel: the pair kernel and its sum pass alone on grid_all's scores, 20 back-to-back calls between two device events:
  ``visits`` counts every (row, staged row) comparison slot, ``pairs`` the (positive, negative) pairs of one segment that count.
* sklearn: the same scores with scikit-learn's functions called in the loop the reference uses (per model; per grid point and fold), on
  one core: the median of five after one warm-up.

Each GPU step runs in a child process of its own under a time limit; if it fails or runs out of time nothing more is started on the GPU.
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
TABLE = (10, 1562)
GRID = (144, 6246, 5)
REG = (1, 1058, 5)


def synth(M, n, folds, seed):
    """(y, pred [M, n], proba [M, n] float64, groups): columns of differing quality, probabilities rounded to 3 decimals so that ties occur."""
    import numpy as np
    rs = np.random.default_rng(seed)
    y = (rs.random(n) < 0.45).astype(np.int64)
    skill = rs.uniform(0.5, 2.5, size=(M, 1))
    proba = np.round(1.0 / (1.0 + np.exp(-(skill * (2 * y - 1) + rs.normal(0.0, 1.5, (M, n))))), 3)
    groups = rs.permutation(np.arange(n) % folds).astype(np.int64) if folds > 1 else None
    return y, (proba > 0.5).astype(np.int64), proba, groups


def synth_regression(seed=3):
    import numpy as np
    M, n, folds = REG
    rs = np.random.default_rng(seed)
    y = rs.normal(0.0, 1.0, n)
    return y, y[None, :] + rs.normal(0.0, 0.6, (M, n)), rs.permutation(np.arange(n) % folds).astype(np.int64)


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
    from bbbp_amd import _dense, _lib, metrics as MT
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize

    def launches(fn):
        before = dict(MT._LAUNCHES)
        fn()
        return {k: MT._LAUNCHES[k] - before[k] for k in before}

    def both(make):
        """make(on_device) -> callable; times it from host arrays and from device tensors."""
        row = {}
        for name, on_device in (("host", False), ("device", True)):
            fn = make(on_device)
            row["launches"] = launches(fn)
            row[name], out = _timed(fn, reps, 2, sync)
        return row, out

    def put(a, on_device):
        return torch.from_numpy(a).to(dev) if on_device else a

    out = {"device": torch.cuda.get_device_name(0)}
    y, pred, proba, _ = synth(*TABLE, 1, seed=1)
    out["table"], got = both(lambda d: (lambda p=put(pred, d), s=put(proba, d): MT.classification_scores(y, p, s, device=dev)))
    out["table"].update(columns=TABLE[0], rows=TABLE[1], mean_auc=float(got["ROC AUC"].mean()), mean_f1=float(got["F1 Score"].mean()))
    y, pred, proba, groups = synth(*GRID, seed=2)
    out["grid_f1"], got = both(lambda d: (lambda p=put(pred, d): MT.scores_from_counts(MT.confusion_counts(y, p, groups=groups, device=dev))["F1 Score"]))
    out["grid_f1"].update(columns=GRID[0], rows=GRID[1], folds=GRID[2], mean_f1=float(got.mean()))
    out["grid_all"], got = both(lambda d: (lambda p=put(pred, d), s=put(proba, d): MT.classification_scores(y, p, s, groups=groups, device=dev)))
    out["grid_all"].update(columns=GRID[0], rows=GRID[1], folds=GRID[2], mean_auc=float(got["ROC AUC"].mean()), mean_f1=float(got["F1 Score"].mean()))
    # the pair kernel and its sum pass alone, on the same scores
    M, n, G = GRID
    prob = MT._Problem(y == 1, groups.astype(np.int32), G, dev)
    scores = torch.from_numpy(proba).to(dev)
    L = _lib.lib()
    res = torch.empty(M * G * 4, dtype=torch.int64, device=dev)
    work = torch.empty(L.bbbp_metrics_work_bytes(1, M, n, G) // 8, dtype=torch.int64, device=dev)
    call = lambda: _lib.check(L.bbbp_metrics_auc_pairs(_dense.stream(), scores.data_ptr(), 1, n, M, n, prob.y01.data_ptr(), prob.seg_ptr(), G,  # noqa: E731
                                                       res.data_ptr(), work.data_ptr()), "bbbp_metrics_auc_pairs")
    call()
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call()
    e1.record()
    sync()
    ms = e0.elapsed_time(e1) / 20
    r = res.cpu().numpy().reshape(M, G, 4)
    pairs = int((r[..., 1] * r[..., 2]).sum())
    out["pair_kernel"] = {"ms_per_call": ms, "calls": 20, "visits": M * n * n, "pairs": pairs, "visits_per_s": M * n * n / (ms * 1e-3),
                          "pairs_per_s": pairs / (ms * 1e-3)}
    y, pred, groups = synth_regression()
    out["regression"], got = both(lambda d: (lambda p=put(pred, d): MT.regression_scores(y, p, groups=groups, device=dev)))
    out["regression"].update(rows=REG[1], folds=REG[2], mean_mse=float(got["MSE"].mean()), mean_r2=float(got["R2"].mean()))
    return out


def sklearn_rows():
    import numpy as np
    import sklearn
    import sklearn.metrics as skm
    eight = [skm.accuracy_score, skm.balanced_accuracy_score, skm.precision_score, skm.recall_score, skm.f1_score, skm.matthews_corrcoef,
             skm.cohen_kappa_score]

    def evaluate(y, p, s):
        return [f(y, p) for f in eight] + [skm.roc_auc_score(y, s)]

    out = {"version": sklearn.__version__, "n_jobs": 1, "host_cpus": os.cpu_count()}
    y, pred, proba, _ = synth(*TABLE, 1, seed=1)
    out["table"], got = _timed(lambda: [evaluate(y, pred[m], proba[m]) for m in range(TABLE[0])], 5, 1, lambda: None)
    out["table"].update(mean_auc=float(np.mean([g[7] for g in got])), mean_f1=float(np.mean([g[4] for g in got])))
    y, pred, proba, groups = synth(*GRID, seed=2)
    rows = [np.flatnonzero(groups == g) for g in range(GRID[2])]
    out["grid_f1"], got = _timed(lambda: [[skm.f1_score(y[r], pred[m][r]) for r in rows] for m in range(GRID[0])], 5, 1, lambda: None)
    out["grid_f1"].update(mean_f1=float(np.mean(got)))
    out["grid_all"], got = _timed(lambda: [[evaluate(y[r], pred[m][r], proba[m][r]) for r in rows] for m in range(GRID[0])], 5, 1, lambda: None)
    out["grid_all"].update(mean_auc=float(np.mean([g[7] for col in got for g in col])), mean_f1=float(np.mean([g[4] for col in got for g in col])))
    y, pred, groups = synth_regression()
    rows = [np.flatnonzero(groups == g) for g in range(REG[2])]
    out["regression"], got = _timed(lambda: [(skm.mean_squared_error(y[r], pred[0][r]), skm.r2_score(y[r], pred[0][r])) for r in rows], 5, 1, lambda: None)
    out["regression"].update(mean_mse=float(np.mean([g[0] for g in got])), mean_r2=float(np.mean([g[1] for g in got])))
    return out


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
    result = {"bench": "metrics"}
    rc = 0
    for run in ("run1", "run2"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(a.reps)], capture_output=True, text=True, timeout=LIMIT_S)
            got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not got:
                print(f"[bench_metrics] gpu {run}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
                rc = r.returncode or 1
            else:
                result[run] = json.loads(got[-1])
        except subprocess.TimeoutExpired:
            print(f"[bench_metrics] gpu {run}: no result within {LIMIT_S} s; stopping", file=sys.stderr)
            rc = 124
        if rc:
            break
    if rc == 0 and not a.no_sklearn:
        result["sklearn"] = sklearn_rows()
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
