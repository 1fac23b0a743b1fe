#!/usr/bin/env python3
"""Times ensemble.fit_classifier_stack and the two models' predict_proba on the GPU beside scikit-learn on one core of the host.

    python tools/bench_stacking.py [--out FILE] [--no-sklearn] [--sklearn-only] [--reps R]

The workload is the classifier stack of the reference's scripts (Models/model_opt.py:208-222) on a seeded synthetic [6 246, 100] float64
matrix with two classes: the eight learners with their defaults (kNN, LogisticRegression, PlattSVC, BernoulliNB, DecisionTree,
RandomForest, GradientBoosting, MLP), ``StackingClassifier(estimators, final_estimator=GradientBoostingClassifier(100, 0.1, 3), cv=5)`` and
``VotingClassifier(estimators, voting='soft')``.

* fit: ``ensemble.fit_classifier_stack(estimators, X, y, final)`` from a host array -- the upload, 8 x 6 base fits (one ``_fit_rows``
  call per learner), the out-of-fold matrix in one launch, the final estimator's fit.
* predict: ``predict_proba`` of both models on 1 562 held-out rows from a host array.
  Both are end-to-end call times dominated by the base learners' fits and predictions: wall time behind a device synchronise, after one
  warm-up call, the median of --reps calls (default 5) with the fastest and the slowest, measured twice.
* kernels: the three entries of csrc/ensemble.hip alone at the workload's shapes (8 x 5 fold entries over 6 246 rows; votes of 8 learners
  over 1 562 rows), between device events, the median of 50 calls after 5.
* ``launches`` counts the three entries' launches per fit and per predict; ``fit_paths`` names the learners whose fits looped.
* sklearn: scikit-learn's ``StackingClassifier`` and ``VotingClassifier`` (``SVC(probability=True)`` in PlattSVC's place) with
  ``n_jobs=1`` on one core: one run each.  It is long.

The GPU step and the baseline each run in a child process of their own under a time limit, the GPU step with the environment as it is, the
baseline with one thread; if the GPU step fails or runs out of time nothing more is started on the GPU.
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

LIMIT_S = 1000
N, N_TEST, D, CV = 6246, 1562, 100, 5


def synth(seed=1):
    import numpy as np
    rs = np.random.default_rng(seed)
    X = rs.normal(size=(N + N_TEST, D))
    score = X[:, :6] @ rs.normal(size=6) + 0.6 * X[:, 6] * X[:, 7] + 1.2 * rs.normal(size=N + N_TEST)
    y = (score > 0.3).astype(np.int64)
    return X[:N], y[:N], X[N:], y[N:]


def _spread(times):
    import numpy as np
    return {"median_s": float(np.median(times)), "min_s": float(min(times)), "max_s": float(max(times)), "reps": len(times)}


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


def _event_ms(fn, reps=50, warmup=5):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)), "reps": reps}


def step_gpu(reps):
    import warnings

    import numpy as np
    import torch
    from bbbp_amd import ensemble as E, gradient_boosting, linear_model, mlp, naive_bayes, neighbors, random_forest, svm
    warnings.simplefilter("ignore")
    X, y, Xt, yt = synth()
    learners = lambda: [("knn", neighbors.KNeighborsClassifier()), ("lr", linear_model.LogisticRegression()), ("svc", svm.PlattSVC()),  # noqa: E731
                        ("bnb", naive_bayes.BernoulliNB()), ("tree", random_forest.DecisionTreeClassifier()),
                        ("rf", random_forest.RandomForestClassifier()), ("gbc", gradient_boosting.GradientBoostingClassifier()),
                        ("mlp", mlp.MLPClassifier())]
    final = gradient_boosting.GradientBoostingClassifier(100, 0.1, 3)
    fit_fn = lambda: E.fit_classifier_stack(learners(), X, y, final, cv=CV)  # noqa: E731

    def launches(fn):
        before = dict(E._LAUNCHES)
        out = fn()
        return {k: E._LAUNCHES[k] - before[k] for k in before}, out

    fit_launches, (stacking, vote) = launches(fit_fn)
    predict_fn = lambda: (stacking.predict_proba(Xt), vote.predict_proba(Xt))  # noqa: E731
    predict_launches, (ps, pv) = launches(predict_fn)
    fits, predicts = [], []
    for _ in range(2):                                 # measured twice: both medians are reported
        fits.append(_timed(fit_fn, reps, 0, torch.cuda.synchronize)[0])
        predicts.append(_timed(predict_fn, reps, 0, torch.cuda.synchronize)[0])
    # the three entries alone, at the workload's shapes
    dev = torch.device("cuda:0")
    rs = np.random.default_rng(2)
    from sklearn.model_selection import StratifiedKFold
    parts = [te for _, te in StratifiedKFold(CV).split(X, y)]
    entries = [(torch.from_numpy(rs.random((len(te), 2))).to(dev), 1, te, j) for j in range(8) for te in parts]
    meta = torch.empty((N, 8), dtype=torch.float64, device=dev)
    probas = [torch.from_numpy(rs.random((N_TEST, 2))).to(dev) for _ in range(8)]
    preds = [torch.from_numpy(rs.integers(0, 2, N_TEST).astype(np.uint8)).to(dev) for _ in range(8)]
    w = rs.uniform(0.1, 2.0, 8)
    # the tables are built and uploaded once: between the events stands the entry's call alone (its host-side checks and its one launch)
    import ctypes
    from bbbp_amd import _dense, _lib, _tree_host
    L, st = _lib.lib(), _dense.stream()
    rows_d = [torch.from_numpy(te).to(dev) for _, _, te, _ in entries]
    table = (_lib.EnsSource * len(entries))(*[_lib.EnsSource(src.data_ptr(), 2, col, r.data_ptr(), len(te), j)
                                              for (src, col, te, j), r in zip(entries, rows_d)])
    table_d = _tree_host.upload(table, dev)
    ids = np.ascontiguousarray(np.concatenate([te for _, _, te, _ in entries]), dtype=np.int64)
    ids_p = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_long))
    soft_t, soft_d, _ = E._columns_table([(p, 0) for p in probas], 2, dev)
    hard_t, hard_d, _ = E._columns_table([(p, 0) for p in preds], 1, dev)
    w_d = torch.from_numpy(w).to(dev)
    avg, cnt = (torch.empty((N_TEST, 2), dtype=torch.float64, device=dev) for _ in range(2))
    lab = torch.empty(N_TEST, dtype=torch.uint8, device=dev)
    calls = {"meta_scatter": lambda: L.bbbp_ens_meta_scatter(st, table, table_d.data_ptr(), len(entries), ids_p, N, 8, meta.data_ptr(), 8),
             "soft_vote": lambda: L.bbbp_ens_soft_vote(st, soft_t, soft_d.data_ptr(), 8, w_d.data_ptr(), float(w.sum()), N_TEST, avg.data_ptr(), lab.data_ptr()),
             "hard_vote": lambda: L.bbbp_ens_hard_vote(st, hard_t, hard_d.data_ptr(), 8, w_d.data_ptr(), N_TEST, cnt.data_ptr(), lab.data_ptr())}
    kernels = {}
    for name, call in calls.items():
        _lib.check(call(), name)
        kernels[name] = _event_ms(call)
    acc = lambda p: float(np.mean((p[:, 1] > p[:, 0]).astype(np.int64) == yt))  # noqa: E731
    return {"device": torch.cuda.get_device_name(0), "n": N, "n_test": N_TEST, "d": D, "cv": CV, "fit": fits, "predict_proba": predicts,
            "launches": {"fit": fit_launches, "predict_proba": predict_launches}, "fit_paths": stacking.fit_paths_,
            "looped": sorted(k for k, v in stacking.fit_paths_.items() if v == "looped"), "kernels": kernels,
            "accuracy": {"stacking": acc(ps), "voting": acc(pv)}}


def sklearn_rows():
    import warnings

    import numpy as np
    import sklearn
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier, StackingClassifier, VotingClassifier
    from sklearn.linear_model import LogisticRegression
    from sklearn.naive_bayes import BernoulliNB
    from sklearn.neighbors import KNeighborsClassifier
    from sklearn.neural_network import MLPClassifier
    from sklearn.svm import SVC
    from sklearn.tree import DecisionTreeClassifier
    warnings.simplefilter("ignore")
    X, y, Xt, yt = synth()
    learners = [("knn", KNeighborsClassifier()), ("lr", LogisticRegression()), ("svc", SVC(probability=True, random_state=0)), ("bnb", BernoulliNB()),
                ("tree", DecisionTreeClassifier(random_state=0)), ("rf", RandomForestClassifier(random_state=0)),
                ("gbc", GradientBoostingClassifier(random_state=0)), ("mlp", MLPClassifier(random_state=0))]
    t0 = time.perf_counter()
    stacking = StackingClassifier(learners, final_estimator=GradientBoostingClassifier(n_estimators=100, learning_rate=0.1, max_depth=3, random_state=0),
                                  cv=CV, n_jobs=1).fit(X, y)
    t1 = time.perf_counter()
    vote = VotingClassifier(learners, voting="soft", n_jobs=1).fit(X, y)
    t2 = time.perf_counter()
    ps, pv = stacking.predict_proba(Xt), vote.predict_proba(Xt)
    t3 = time.perf_counter()
    acc = lambda p: float(np.mean((p[:, 1] > p[:, 0]).astype(np.int64) == yt))  # noqa: E731
    return {"version": sklearn.__version__, "n_jobs": 1, "host_cpus": os.cpu_count(), "runs": 1, "fit_stacking_s": t1 - t0, "fit_voting_s": t2 - t1,
            "fit_s": t2 - t0, "predict_proba_s": t3 - t2, "accuracy": {"stacking": acc(ps), "voting": acc(pv)}}


def _child(args, env=None):
    """One step in a process of its own under the time limit: (exit status, its JSON result or None)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=LIMIT_S, env=env)
    got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print(f"[bench_stacking] {' '.join(args)}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return r.returncode or 1, None
    return 0, json.loads(got[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-only", action="store_true", help="only the scikit-learn baseline: no GPU is touched")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per GPU figure")
    ap.add_argument("--step", choices=("gpu", "sklearn"), help=argparse.SUPPRESS)      # child mode: run one step and print its JSON line
    a = ap.parse_args()
    if not 1 <= a.reps <= 1000:
        ap.error("--reps within 1..1000")
    if a.step:
        print("RESULT " + json.dumps(step_gpu(a.reps) if a.step == "gpu" else sklearn_rows()), flush=True)
        return 0
    result, rc = {"bench": "stacking"}, 0
    # the GPU step keeps the environment it was given; the baseline's one core is set for the baseline's process alone
    one_thread = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    try:
        if not a.sklearn_only:
            rc, result["gpu"] = _child(["--step", "gpu", "--reps", str(a.reps)])
        if rc == 0 and not a.no_sklearn:
            rc, result["sklearn"] = _child(["--step", "sklearn"], env=one_thread)
    except subprocess.TimeoutExpired:
        print(f"[bench_stacking] no result within {LIMIT_S} s; stopping", file=sys.stderr)
        rc = 124
    result = {k: v for k, v in result.items() if v is not None}
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
