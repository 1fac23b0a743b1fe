"""Numpy restatement of Bernoulli naive Bayes as bbbp_amd.naive_bayes computes it: the binarise rule, integer counts per (rows, class),
the host table expressions, the joint log-likelihood in its fixed order, and the grid / learning-curve bookkeeping as plain loops of
single fits.  tests/test_bnb_cpu.py pins it to scikit-learn; tests/test_gpu_bnb.py holds the GPU to it bit for bit.

Nothing here shares code with the module under test: ``backend`` is the pair of callables its bookkeeping accepts in place of the device."""
import functools
import itertools

import numpy as np


def binarise(X, threshold):
    """bool [n, d]: ``X > threshold``, strict.  The threshold takes the array's dtype first (numpy's rule for an array compared with a
    Python float, which is what ``sklearn.preprocessing.binarize`` does): for float32 X, 0.1 becomes ``np.float32(0.1)``."""
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    return X > X.dtype.type(threshold)


def counts(B, y01, rows):
    """(feature_count int64 [2, d], class_count int64 [2]) of the rows ``rows`` of the binarised matrix."""
    Br, yr = B[rows], y01[rows]
    fc = np.stack([Br[yr == c].sum(axis=0, dtype=np.int64) for c in (0, 1)])
    cc = np.array([np.count_nonzero(yr == c) for c in (0, 1)], dtype=np.int64)
    return fc, cc


def tables(fc, cc, alpha, fit_prior=True, class_prior=None):
    """(feature_log_prob_, class_log_prior_, w, c): scikit-learn's expressions (naive_bayes.py, ``_update_feature_log_prob``,
    ``_update_class_log_prior``, ``_joint_log_likelihood``) on float64 copies of the integer counts."""
    fc, cc = fc.astype(np.float64), cc.astype(np.float64)
    smoothed_fc = fc + alpha
    smoothed_cc = cc + alpha * 2
    flp = np.log(smoothed_fc) - np.log(smoothed_cc.reshape(-1, 1))
    if class_prior is not None:
        prior = np.log(np.asarray(class_prior, dtype=np.float64))
    elif fit_prior:
        prior = np.log(cc) - np.log(cc.sum())
    else:
        prior = np.full(2, -np.log(2))
    neg = np.log(1 - np.exp(flp))
    return flp, prior, flp - neg, prior + neg.sum(axis=1)


def jll(B, w, c):
    """float64 [m, 2]: per row and class, start from 0.0, add ``w[k, j]`` for the set features j in ascending order, then ``c[k]``; one
    float64 addition each (the loop over j adds one term to the rows that have the bit, nothing is summed pairwise)."""
    B = np.asarray(B, dtype=bool)
    s = np.zeros((B.shape[0], 2), dtype=np.float64)
    for j in range(B.shape[1]):
        on = B[:, j]
        s[on, 0] = s[on, 0] + w[0, j]
        s[on, 1] = s[on, 1] + w[1, j]
    s[:, 0] = s[:, 0] + c[0]
    s[:, 1] = s[:, 1] + c[1]
    return s


def jll_bound(B, w, c):
    """The per-entry bound between two float64 summations of the same terms in any order: ``2 (d + 2) 2^-53 (sum over set j of |w_kj| +
    |c_k|)`` (tests/test_bnb_cpu.py derives it)."""
    d = B.shape[1]
    mass = np.asarray(B, dtype=np.float64) @ np.abs(w).T + np.abs(c)
    return 2 * (d + 2) * 2.0 ** -53 * mass * (1 + 2.0 ** -40)          # the bound's own evaluation rounds too


class Fit:
    """One fitted model of the restatement."""

    def __init__(self, X, y, alpha=1.0, binarize=0.0, fit_prior=True, class_prior=None, rows=None):
        X, y = np.asarray(X), np.asarray(y)
        self.classes = np.unique(y)
        assert len(self.classes) == 2
        y01 = (y == self.classes[1]).astype(np.uint8)
        rows = np.arange(len(y)) if rows is None else np.asarray(rows)
        self.binarize = binarize
        self.fc, self.cc = counts(binarise(X, binarize), y01, rows)
        self.flp, self.prior, self.w, self.c = tables(self.fc, self.cc, alpha, fit_prior, class_prior)

    def jll(self, Q):
        return jll(binarise(Q, self.binarize), self.w, self.c)

    def predict01(self, Q):
        return np.argmax(self.jll(Q), axis=1)

    def predict(self, Q):
        return self.classes[self.predict01(Q)]


def backend(X, thresholds):
    """(count, jll) over X binarised at every threshold: what bbbp_amd.naive_bayes' bookkeeping takes in place of the device."""
    planes = [binarise(X, t) for t in thresholds]

    def count(row_lists, y01, pairs):
        got = [counts(planes[t], y01, row_lists[m]) for m, t in pairs]
        cc = np.stack([counts(planes[0], y01, r)[1] for r in row_lists])
        return np.stack([fc for fc, _ in got]), cc

    def jll_(w, c, threshold_of, row_lists):
        return [jll(planes[t] if r is None else planes[t][r], w[p], c[p]) for p, (t, r) in enumerate(zip(threshold_of, row_lists))]

    return count, jll_


def f1(truth01, pred01):
    tp = int(np.sum((truth01 == 1) & (pred01 == 1)))
    fp, fn = int(np.sum((truth01 == 0) & (pred01 == 1))), int(np.sum((truth01 == 1) & (pred01 == 0)))
    return 2 * tp / (2 * tp + fp + fn) if tp + fp + fn else 0.0


def grid_search(X, y, param_grid, cv=5):
    """(best_params, mean F1 per point, Fit on all rows): sorted keys, product order, StratifiedKFold(cv), the first maximum."""
    from sklearn.model_selection import StratifiedKFold
    X, y = np.asarray(X), np.asarray(y)
    points = []
    for sub in ([param_grid] if isinstance(param_grid, dict) else list(param_grid)):
        keys = sorted(sub)
        points += [dict(zip(keys, vals)) for vals in itertools.product(*(sub[k] for k in keys))]
    y01 = (y == np.unique(y)[1]).astype(np.uint8)
    folds = list(StratifiedKFold(n_splits=cv).split(X, y))
    scores = []
    for pt in points:
        per_fold = [f1(y01[te], Fit(X, y, rows=tr, **pt).predict01(X[te])) for tr, te in folds]
        scores.append(float(np.mean(per_fold)))
    best = int(np.argmax(scores))
    return points[best], scores, Fit(X, y, **points[best])


def learning_curve(params, X, y, cv=5, train_sizes=np.linspace(0.1, 1.0, 5), scoring="f1"):
    """(sizes, train_scores [sizes, folds], test_scores [sizes, folds]) without shuffling: prefixes of every fold's training rows."""
    from sklearn.model_selection import StratifiedKFold
    X, y = np.asarray(X), np.asarray(y)
    y01 = (y == np.unique(y)[1]).astype(np.uint8)
    folds = list(StratifiedKFold(n_splits=cv).split(X, y))
    n_max = len(folds[0][0])
    sizes = np.asarray(train_sizes)
    if np.issubdtype(sizes.dtype, np.floating):
        sizes = np.clip((sizes * n_max).astype(int), 1, n_max)
    sizes = np.unique(sizes)
    score = f1 if scoring == "f1" else (lambda t, p: float(np.mean(t == p)))
    train, test = np.zeros((len(sizes), len(folds))), np.zeros((len(sizes), len(folds)))
    for fi, (tr, te) in enumerate(folds):
        for si, size in enumerate(sizes):
            fit = Fit(X, y, rows=tr[:size], **params)
            train[si, fi] = score(y01[tr[:size]], fit.predict01(X[tr[:size]]))
            test[si, fi] = score(y01[te], fit.predict01(X[te]))
    return sizes, train, test


# ---- data ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fingerprint_problem(n, d, seed=0, bits=167, dtype="float64"):
    """Bernoulli fingerprints with class-dependent bit rates in [0.05, 0.65], standardised, then PCA(d): the reference's pipeline in small.
    Labels 0 / 1 in random order.  Read-only arrays, shared by the tests."""
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(20261020 + seed)
    y = (rng.random(n) < 0.45).astype(np.int64)
    y[:2] = (0, 1)
    rates = rng.uniform(0.05, 0.65, size=(2, bits))
    F = (rng.random((n, bits)) < rates[y]).astype(np.float64)
    X = PCA(n_components=d, svd_solver="full").fit_transform(StandardScaler().fit_transform(F)).astype(dtype)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def gaussian_problem(n, d, seed=0, dtype="float64"):
    """n x d normal columns shifted by class, some columns rounded so that values meet the thresholds 0.0, 0.5 and 1.0 exactly, one
    column of -0.0 / 0.0; the first two rows are one of each class.  Read-only."""
    rng = np.random.default_rng(977 + 31 * n + d + seed)
    y = (rng.random(n) < 0.4).astype(np.int64)
    y[:2] = (0, 1)
    X = rng.standard_normal((n, d)) + 0.8 * y[:, None] * (rng.random(d) < 0.5)
    X[:, ::3] = np.round(X[:, ::3] * 2) / 2
    if d > 4:
        X[:, 4] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    X = X.astype(dtype)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y
