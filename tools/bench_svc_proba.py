#!/usr/bin/env python3
"""Times svm.PlattSVC on the GPU beside the work libsvm's probability scheme implies without the shared matrix and batch.

    python tools/bench_svc_proba.py [--out FILE] [--rows N [N ...]] [--d D]

Shape: SVC(probability=True) of the reference's classification scripts (Models/model_opt_maccs.py:128) -- five internal folds and the fit on
all rows -- on seeded two-class data of --rows rows (default 850 and 6400) and --d features (default 100), float64, RBF, C = 1:
y uniform in {-1, +1}, X = randn + 0.5 y on the first three features.  Per row count, in one child process under a time limit:

* plattsvc_fit_s: wall time of PlattSVC().fit behind a device synchronise -- one kernel matrix, six problems in one solver batch, the
  out-of-fold decision kernel, the sigmoid fit (median of three after a warm-up call);
* six_svc_fits_s: six SVC().fit one after the other on the same five training parts and on all rows, each forming its own matrix: what the
  scheme costs with the classifier alone;
* oof_decision_us / platt_fit_us: the two new kernels alone on the solved fold problems, device events around the launch (median of five);
* iteration counts of the six problems, and whether (A, B) and the out-of-fold values are the same bits on every repeat.

Nothing outside this repository is read.  Prints one JSON line per row count.
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

LIMIT_S = 240


def synth(n, d, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    y = np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0)
    X = rs.randn(n, d)
    X[:, :min(3, d)] += 0.5 * y[:, None]
    return X, y


def step(n, d):
    import numpy as np
    import torch
    from bbbp_amd import svm
    X, y = synth(n, d)
    held = svm.platt_folds(n, 5, 0)
    trains = [np.setdiff1d(np.arange(n), te) for te in held]

    def median(f, reps):
        f()                                                                      # warm-up: every shape the timed calls use
        times, out = [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return out, sorted(times)[reps // 2], times

    fits = []
    clf, together, together_all = median(lambda: fits.append(svm.PlattSVC().fit(X, y)) or fits[-1], 3)
    singles, alone, alone_all = median(lambda: [svm.SVC().fit(X[tr], y[tr]) for tr in trains] + [svm.SVC().fit(X, y)], 3)
    same = all(np.array_equal(f.oof_decision_, clf.oof_decision_) and f.probA_[0] == clf.probA_[0] and f.probB_[0] == clf.probB_[0] for f in fits)

    # the two kernels alone, on the fold problems solved once more
    dev = torch.device("cuda:0")
    Xd = torch.from_numpy(X).to(dev)
    K = svm.kernel_matrix(Xd, "rbf", svm._resolve_gamma("scale", Xd))[0]
    ys = np.where(y == clf.classes_[0], 1.0, -1.0)
    y_d = torch.from_numpy(ys).to(dev)
    oof = torch.empty(n, dtype=torch.float64, device=dev)
    parts = svm._platt_problems(K, y_d, ys, held, 1.0, 1e-3, oof)
    svm._solve([pr for pr, _ in parts])
    ab = torch.empty((1, 2), dtype=torch.float64, device=dev)
    info = torch.empty((1, 2), dtype=torch.int32, device=dev)

    def events(f):
        f()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) * 1e3)
        return sorted(ms)[2], ms

    oof_us, oof_all = events(lambda: svm._oof_launch(K, parts, oof))
    platt_us, platt_all = events(lambda: svm._platt_launch([oof], [y_d], ab, info))
    assert np.array_equal(oof.cpu().numpy(), clf.oof_decision_) and ab[0, 0].item() == clf.probA_[0]
    return {"rows": n, "d": d, "plattsvc_fit_s": together, "plattsvc_fit_s_all": together_all, "six_svc_fits_s": alone, "six_svc_fits_s_all": alone_all,
            "oof_decision_us": oof_us, "oof_decision_us_all": oof_all, "platt_fit_us": platt_us, "platt_fit_us_all": platt_all,
            "platt_iterations": clf.platt_n_iter_, "platt_status": clf.platt_status_, "probA": clf.probA_[0], "probB": clf.probB_[0],
            "iterations_all_rows": clf.n_iter_, "iterations_single": [m.n_iter_ for m in singles], "same_bits_on_every_repeat": bool(same)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--rows", type=int, nargs="+", default=[850, 6400])
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--step", type=int, help=argparse.SUPPRESS)       # child mode: one row count, one JSON line
    a = ap.parse_args()
    if min(a.rows) < 10 or a.d < 1:
        ap.error("--rows must be at least 10 and --d positive")
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.d)), flush=True)
        return 0
    lines, rc = [], 0
    for n in a.rows:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(n), "--d", str(a.d)], capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"[bench_svc_proba] rows {n}: no result within {LIMIT_S} s; stopping", file=sys.stderr)
            rc = 124
            break
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"[bench_svc_proba] rows {n}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            rc = r.returncode or 1
            break
        lines.append(json.loads(got[-1]))
        print(got[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
