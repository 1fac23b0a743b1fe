"""``sklearn.naive_bayes.BernoulliNB`` for the GPU: the binarised matrix packed into bits once, every fit of a batch counted in one launch
and every joint log-likelihood of a batch computed in one more.

The reference's classification scripts search ``BernoulliNB()`` over ``alpha x binarize`` under five folds and draw its learning curve
(``Models/model_maccs.py:257-267``, ``model_opt_20250130.py:507-510``): 75 fits plus the refit, then 30 fits with 60 scoring passes, on
6 000 to 8 000 rows of 100 PCA columns.  A fit is counting and a prediction adds one table entry per set bit, so
(``csrc/bnb.hip``):

* ``bbbp_bnb_pack`` writes bit ``x > threshold`` (strict, as ``sklearn.preprocessing.binarize``; for float32 ``X`` the threshold is
  rounded to float32 first, numpy's rule) for every threshold of the batch, feature-major for counting and row-major for prediction,
  and flags NaN and infinity;
* ``bbbp_bnb_count`` counts every (row mask, threshold) pair of a batch: ``feature_count`` and ``class_count`` as exact integers.  A row
  mask is a bit vector over the rows of ``X``: a fold's training rows or a learning-curve prefix, intersected with either class;
* ``bbbp_bnb_jll`` adds, per (problem, query row), the problem's table entries of the row's set bits in ascending order in float64 and
  then the constant: a fixed order, so ``tests/bnb_numpy.py`` reproduces a result bit for bit.

The log tables are formed on the host, in numpy, with scikit-learn's own expressions on the integer counts (``tables``): a device ``log``
would not give numpy's bits and a table is 2 d doubles.  ``feature_count_``, ``class_count_``, ``feature_log_prob_`` and
``class_log_prior_`` are therefore scikit-learn 1.7's bit for bit, and ``alpha`` never reaches the device: the alphas of a grid share
their counts.  A joint log-likelihood differs from scikit-learn's only by the order of its at most d + 1 additions (BLAS there).

``fit_masks`` is the batch entry (row lists x thresholds x alphas: one pack, one count launch, one host read), ``grid_search_cv`` and
``learning_curve`` run the reference's searches on it.  Their bookkeeping is separate from the device: ``backend(X, thresholds)`` returns
the two callables ``count`` and ``jll`` (``device_backend`` here, the numpy restatement in the CPU tests).

Out of scope, each refused by name: more than two classes, ``sample_weight``, ``partial_fit``, ``binarize=None``, sparse input, NaN or
infinity in ``X``, a ``class_prior`` that is not two positive numbers, an ``alpha`` that is not one finite number >= 0, a row subset that
lacks one of the two classes (scikit-learn would fit a one-class model), a fit whose tables are not finite (a tiny alpha with a feature
set in every row of a class: scikit-learn's joint log-likelihood is NaN there), more than one GPU.  There is no CPU path.
"""
from __future__ import annotations

import itertools
import numbers

import numpy as np
import torch

from . import _dense, _lib

MAX_FEATURES, MAX_THRESHOLDS, MAX_PROBLEMS, MAX_ITEMS = 1048576, 1024, 65535, 2147483647      # BBBP_BNB_MAX_*
MAX_ROWS = 2147483647
_LAUNCHES = {"pack": 0, "count": 0, "jll": 0}      # launches of this process (tests and the bench tool count them)
_WHO = "naive_bayes"


# ---- argument checks: nothing here touches the GPU -----------------------------------------------------------------------------------
def _is_sparse(X):
    return hasattr(X, "tocsr") or (isinstance(X, torch.Tensor) and X.layout != torch.strided)


def _is_real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _check_alpha(alpha, who):
    if not _is_real(alpha) or not 0.0 <= float(alpha) < float("inf"):
        raise ValueError(f"{who}: alpha must be one finite number >= 0 (an array of alphas is not supported), got {alpha!r}")


def _check_binarize(binarize, who):
    if binarize is None:
        raise ValueError(f"{who}: binarize=None is not supported (X is always thresholded; pass a number)")
    if not _is_real(binarize) or not np.isfinite(float(binarize)):
        raise ValueError(f"{who}: binarize must be a finite number, got {binarize!r}")


def _check_class_prior(class_prior, who):
    if class_prior is None:
        return
    try:
        prior = np.asarray(class_prior, dtype=np.float64)
    except (TypeError, ValueError):
        prior = None
    if prior is None or prior.shape != (2,) or not np.all(np.isfinite(prior)) or not np.all(prior > 0.0):
        raise ValueError(f"{who}: class_prior must be two positive numbers, got {class_prior!r}")


def _check_device(device, who):
    if torch.device(device).type != "cuda":
        raise ValueError(f"{who}: device {device!r}: counting and prediction run on the GPU (no CPU fallback)")


def _check_input(X, who):
    """Shape (n, d) of a dense 2-D input within the limits."""
    if _is_sparse(X):
        raise ValueError(f"{who}: sparse input is not supported (X must be a dense numpy array or CUDA tensor)")
    shape = tuple(X.shape) if isinstance(X, torch.Tensor) else np.shape(X)
    if len(shape) != 2:
        raise ValueError(f"{who}: expected a 2-D [n, d] input, got shape {shape}")
    n, d = shape
    if n < 1 or d < 1:
        raise ValueError(f"{who}: X must have at least one row and one feature, got shape {shape}")
    if n > MAX_ROWS or d > MAX_FEATURES:
        raise ValueError(f"{who}: X is {n} x {d}, at most {MAX_ROWS} rows and {MAX_FEATURES} features (BBBP_BNB_MAX_D) are supported")
    return int(n), int(d)


def _binary_labels(y, n, who):
    """(classes, y01 uint8): labels of any sortable kind, exactly two of them."""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"{who}: y must be 1-D, got shape {y.shape}")
    if len(y) != n:
        raise ValueError(f"{who}: X has {n} rows, y has {len(y)}")
    classes = np.unique(y)
    if len(classes) != 2:
        raise ValueError(f"{who}: {len(classes)} classes in y, exactly two are supported")
    return classes, (y == classes[1]).astype(np.uint8)


def _row_lists(rows, n, y01, who):
    """Every row list as int64 indices into [0, n): no row twice (a mask holds a row once), both classes present."""
    out = []
    for k, r in enumerate(rows):
        r = np.arange(n, dtype=np.int64) if r is None else np.asarray(r)
        if r.ndim != 1 or r.dtype.kind not in "iu":
            raise ValueError(f"{who}: row list {k} must be a 1-D array of integer indices")
        r = r.astype(np.int64)
        if len(r) == 0 or r.min() < 0 or r.max() >= n:
            raise ValueError(f"{who}: row list {k} is empty or leaves [0, {n})")
        if len(np.unique(r)) != len(r):
            raise ValueError(f"{who}: row list {k} repeats a row (a row mask holds every row once)")
        seen = np.bincount(y01[r], minlength=2)
        if not seen.all():
            raise ValueError(f"{who}: row list {k} ({len(r)} rows) lacks one of the two classes (counts {seen.tolist()}); "
                             "scikit-learn would fit a one-class model there")
        out.append(r)
    return out


# ---- the host tables: scikit-learn's expressions on integer counts ---------------------------------------------------------------------
def tables(feature_count, class_count, alpha, fit_prior=True, class_prior=None, force_alpha=True):
    """(feature_log_prob_ [2, d], class_log_prior_ [2], w [2, d], c [2]) from integer counts, as ``BernoulliNB`` forms them in float64:
    ``flp = log(fc + alpha) - log((cc + 2 alpha).reshape(-1, 1))``, the prior ``log(cc) - log(cc.sum())`` (or ``-log(2)``, or
    ``log(class_prior)``), ``neg = log(1 - exp(flp))``, ``w = flp - neg``, ``c = prior + neg.sum(axis=1)``."""
    fc, cc = np.asarray(feature_count, dtype=np.float64), np.asarray(class_count, dtype=np.float64)
    alpha = alpha if force_alpha else max(alpha, 1e-10)
    with np.errstate(divide="ignore", invalid="ignore"):
        flp = np.log(fc + alpha) - np.log((cc + alpha * 2).reshape(-1, 1))
        if class_prior is not None:
            prior = np.log(np.asarray(class_prior, dtype=np.float64))
        elif fit_prior:
            prior = np.log(cc) - np.log(cc.sum())
        else:
            prior = np.full(2, -np.log(2))
        neg = np.log(1 - np.exp(flp))
        w = flp - neg
        c = prior + neg.sum(axis=1)
    return flp, prior, w, c


def f1_binary(truth01, pred01):
    """``f1_score`` of class 1 as scikit-learn 1.7 forms it: ``2 tp / (positives + predicted positives)``, 0.0 without either."""
    truth01, pred01 = np.asarray(truth01, dtype=bool), np.asarray(pred01, dtype=bool)
    tp, denom = int(np.count_nonzero(truth01 & pred01)), int(np.count_nonzero(truth01)) + int(np.count_nonzero(pred01))
    return 2 * tp / denom if denom else 0.0


def _score(scoring, truth01, pred01):
    return f1_binary(truth01, pred01) if scoring == "f1" else float(np.mean(np.asarray(truth01) == np.asarray(pred01)))


# ---- the device backend ------------------------------------------------------------------------------------------------------------------
class _Bits:
    """X packed for a list of thresholds on the device: one ``bbbp_bnb_pack`` launch and one host read of its flag."""

    def __init__(self, X, thresholds, device, planes=True, who=_WHO):
        dev = torch.device(device)
        self.X, self.was_numpy = _dense.to_device_matrix(X, dev, who, allow_row_stride=True)
        self.n, self.d = (int(s) for s in self.X.shape)
        self.T = len(thresholds)
        if not 1 <= self.T <= MAX_THRESHOLDS:
            raise ValueError(f"{who}: {self.T} distinct thresholds, 1 .. {MAX_THRESHOLDS} are supported (BBBP_BNB_MAX_THRESHOLDS)")
        self.W, self.Wd = -(-self.n // 64), -(-self.d // 64)
        with torch.cuda.device(dev):
            thr = torch.from_numpy(np.asarray(thresholds, dtype=np.float64)).to(dev)
            self.planes = torch.empty((self.T, self.d, self.W), dtype=torch.int64, device=dev) if planes else None
            self.rowwords = torch.empty((self.T, self.n, self.Wd), dtype=torch.int64, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().bbbp_bnb_pack(_dense.stream(), self.X.data_ptr(), _dense.DT[self.X.dtype], _dense.ld(self.X), self.n, self.d,
                                                thr.data_ptr(), self.T, None if self.planes is None else self.planes.data_ptr(),
                                                self.rowwords.data_ptr(), flag.data_ptr()), "bbbp_bnb_pack")
            _LAUNCHES["pack"] += 1
            if int(flag.item()):
                raise ValueError(f"{who}: X contains NaN or infinity")

    def masks(self, row_lists, y01):
        """uint64 [M, 2, W] on the host: bit i of mask (m, c) is set when row i is in list m and of class c."""
        bits = np.zeros((len(row_lists), 2, self.W * 64), dtype=bool)
        for m, r in enumerate(row_lists):
            bits[m, y01[r], r] = True
        return np.packbits(bits, axis=-1, bitorder="little").view("<u8")

    def count(self, row_lists, y01, pairs):
        """(feature_count int64 [len(pairs), 2, d], class_count int64 [len(row_lists), 2]): one launch, one host read."""
        M, P = len(row_lists), len(pairs)
        if not (1 <= M <= MAX_PROBLEMS and 1 <= P <= MAX_PROBLEMS and 2 * self.d * P + 2 * M <= MAX_ITEMS):
            raise ValueError(f"{_WHO}: a batch of {M} row lists and {P} (rows, threshold) pairs over {self.d} features exceeds one launch "
                             f"(BBBP_BNB_MAX_PROBLEMS {MAX_PROBLEMS}, BBBP_BNB_MAX_ITEMS {MAX_ITEMS})")
        pairs = np.asarray(pairs, dtype=np.int32).reshape(P, 2)
        if pairs[:, 0].min() < 0 or pairs[:, 0].max() >= M or pairs[:, 1].min() < 0 or pairs[:, 1].max() >= self.T:
            raise ValueError(f"{_WHO}: a (rows, threshold) pair names a row list or a threshold outside the batch")
        dev = self.X.device
        with torch.cuda.device(dev):
            masks = torch.from_numpy(self.masks(row_lists, y01).view(np.int64)).to(dev)
            pd = torch.from_numpy(np.ascontiguousarray(pairs.T)).to(dev)          # [2, P]: the masks' indices, then the thresholds'
            out = torch.empty(2 * self.d * P + 2 * M, dtype=torch.int32, device=dev)
            fc, cc = out[:2 * self.d * P], out[2 * self.d * P:]
            _lib.check(_lib.lib().bbbp_bnb_count(_dense.stream(), self.planes.data_ptr(), self.n, self.d, self.T, masks.data_ptr(), M, pd[0].data_ptr(),
                                                 pd[1].data_ptr(), P, fc.data_ptr(), cc.data_ptr()), "bbbp_bnb_count")
            _LAUNCHES["count"] += 1
            host = out.cpu().numpy().astype(np.int64)
        if (host < 0).any():
            raise RuntimeError(f"{_WHO}: the count kernel refused a pair (a defect of the host side, not of the data)")
        return host[:2 * self.d * P].reshape(P, 2, self.d), host[2 * self.d * P:].reshape(M, 2)

    def jll_device(self, w, c, threshold_of, row_lists):
        """The batch's joint log-likelihoods on the device, float64 [sum of rows, 2], and every problem's first row in it: one launch."""
        w, c = np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
        P = len(threshold_of)
        if w.shape != (P, 2, self.d) or c.shape != (P, 2) or len(row_lists) != P:
            raise ValueError(f"{_WHO}: jll: tables {w.shape} / {c.shape} do not fit {P} problems of {self.d} features")
        if not 1 <= P <= MAX_PROBLEMS:
            raise ValueError(f"{_WHO}: a batch of {P} scoring problems exceeds one launch (BBBP_BNB_MAX_PROBLEMS {MAX_PROBLEMS})")
        desc, rows, at, row_at = np.zeros((P, 4), dtype=np.int64), [], 0, 0
        for p, (t, r) in enumerate(zip(threshold_of, row_lists)):
            if not 0 <= int(t) < self.T:
                raise ValueError(f"{_WHO}: jll: threshold index {t} outside the batch")
            if r is None:
                desc[p] = (t, -1, self.n, at)
            else:
                r = np.asarray(r)
                if len(r) and (r.min() < 0 or r.max() >= self.n):
                    raise ValueError(f"{_WHO}: jll: a query row leaves [0, {self.n})")
                desc[p] = (t, row_at, len(r), at)
                rows.append(r.astype(np.int32))
                row_at += len(r)
            at += int(desc[p, 2])
        dev = self.X.device
        with torch.cuda.device(dev):
            out = torch.empty((at, 2), dtype=torch.float64, device=dev)
            if at:
                tab = torch.from_numpy(np.concatenate([w.ravel(), c.ravel()])).to(dev)
                dd = torch.from_numpy(desc).to(dev)
                rd = torch.from_numpy(np.concatenate(rows)).to(dev) if row_at else None
                _lib.check(_lib.lib().bbbp_bnb_jll(_dense.stream(), self.rowwords.data_ptr(), self.n, self.d, self.T, tab.data_ptr(),
                                                   tab[w.size:].data_ptr(), dd.data_ptr(), P, None if rd is None else rd.data_ptr(), row_at,
                                                   int(desc[:, 2].max()), at, out.data_ptr()), "bbbp_bnb_jll")
                _LAUNCHES["jll"] += 1
        return out, desc[:, 3], desc[:, 2]

    def jll(self, w, c, threshold_of, row_lists):
        """A list of float64 [rows, 2] numpy arrays, one per problem: one launch, one host read."""
        out, begin, m = self.jll_device(w, c, threshold_of, row_lists)
        host = out.cpu().numpy()
        return [host[b:b + k] for b, k in zip(begin, m)]


def device_backend(device="cuda"):
    """``backend(X, thresholds) -> (count, jll)`` on the GPU: ``count(row_lists, y01, pairs)`` gives the integer ``feature_count``
    [pairs, 2, d] and ``class_count`` [row lists, 2] of every (row list, threshold index) pair; ``jll(w, c, threshold_of, row_lists)``
    gives every problem's joint log-likelihoods [rows, 2] over its query rows (``None``: all rows of X)."""
    def backend(X, thresholds):
        bits = _Bits(X, thresholds, device)
        return bits.count, bits.jll
    return backend


# ---- the estimator -------------------------------------------------------------------------------------------------------------------
class BernoulliNB:
    """``BernoulliNB(alpha=1.0, binarize=0.0, fit_prior=True, class_prior=None, *, force_alpha=True, device="cuda")``: scikit-learn 1.7's
    names, two classes.

    ``fit`` takes a numpy array or a CUDA tensor [n, d] (float32 or float64, unit inner stride, any row stride) and labels of any sortable
    kind, and sets ``classes_``, ``class_count_``, ``feature_count_``, ``feature_log_prob_``, ``class_log_prior_`` (scikit-learn's, bit
    for bit) and ``n_features_in_``.  ``predict_joint_log_proba`` / ``predict_log_proba`` / ``predict_proba`` return float64 [m, 2], numpy
    for numpy queries and a CUDA tensor for a CUDA tensor; ``predict`` returns numpy labels, ties to ``classes_[0]``.  ``get_params`` /
    ``set_params`` make ``sklearn.base.clone`` work."""

    _who = "BernoulliNB"
    _params = ("alpha", "binarize", "fit_prior", "class_prior", "force_alpha", "device")

    def __init__(self, alpha=1.0, binarize=0.0, fit_prior=True, class_prior=None, *, force_alpha=True, device="cuda"):
        who = self._who
        _check_alpha(alpha, who)
        _check_binarize(binarize, who)
        _check_class_prior(class_prior, who)
        _check_device(device, who)
        # the parameters are kept as they were given: sklearn.base.clone compares them by identity
        self.alpha, self.binarize, self.fit_prior, self.class_prior, self.force_alpha, self.device = alpha, binarize, fit_prior, class_prior, force_alpha, device

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._params}

    def set_params(self, **params):
        unknown = set(params) - set(self._params)
        if unknown:
            raise ValueError(f"{self._who}: unknown parameters {sorted(unknown)}")
        type(self)(**{**self.get_params(), **params})          # the constructor's checks
        for name, value in params.items():
            setattr(self, name, value)
        return self

    # ---- fit ----
    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise ValueError(f"{self._who}: sample_weight is not supported")
        model = fit_masks(X, y, [None], [self.binarize], [self.alpha], fit_prior=self.fit_prior, class_prior=self.class_prior,
                          force_alpha=self.force_alpha, device=self.device, who=self._who)[0]
        self._adopt(model.classes_, model.feature_count_, model.class_count_, model.feature_log_prob_, model.class_log_prior_, model._w, model._c)
        return self

    def partial_fit(self, X, y, classes=None, sample_weight=None):
        raise ValueError(f"{self._who}: partial_fit is not supported (a fit is one pass over packed bits; fit again on all rows)")

    def _adopt(self, classes, fc, cc, flp, prior, w, c):
        if not (np.all(np.isfinite(w)) and np.all(np.isfinite(c))):
            raise ValueError(f"{self._who}: the fitted tables are not finite (alpha = {self.alpha!r}: a feature that is set in every row of a "
                             "class gives log(1 - 1); scikit-learn's joint log-likelihood is NaN there); use a larger alpha")
        self.classes_, self.feature_count_, self.class_count_ = classes, np.asarray(fc, dtype=np.float64), np.asarray(cc, dtype=np.float64)
        self.feature_log_prob_, self.class_log_prior_, self._w, self._c = flp, prior, w, c
        self.n_features_in_ = int(flp.shape[1])
        return self

    @classmethod
    def from_sklearn(cls, fitted, device="cuda"):
        """Adopt a fitted scikit-learn ``BernoulliNB`` of two classes and predict with its tables."""
        who = f"{cls.__name__}.from_sklearn"
        if not all(hasattr(fitted, a) for a in ("feature_log_prob_", "class_log_prior_", "classes_", "binarize")):
            raise ValueError(f"{who}: a fitted scikit-learn BernoulliNB is expected")
        if len(fitted.classes_) != 2:
            raise ValueError(f"{who}: {len(fitted.classes_)} classes, exactly two are supported")
        self = cls(alpha=fitted.alpha, binarize=fitted.binarize, fit_prior=fitted.fit_prior, class_prior=fitted.class_prior,
                   force_alpha=getattr(fitted, "force_alpha", True), device=device)
        flp, prior = np.asarray(fitted.feature_log_prob_, dtype=np.float64), np.asarray(fitted.class_log_prior_, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            neg = np.log(1 - np.exp(flp))
        return self._adopt(np.asarray(fitted.classes_), fitted.feature_count_, fitted.class_count_, flp, prior, flp - neg, prior + neg.sum(axis=1))

    # ---- prediction ----
    def _jll(self, X):
        """(float64 [m, 2] on the device, was_numpy): one pack of the query rows, one jll launch."""
        if not hasattr(self, "_w"):
            raise RuntimeError(f"{self._who}: not fitted")
        n, d = _check_input(X, self._who)
        if d != self.n_features_in_:
            raise ValueError(f"{self._who}: X has {d} features, the model was fitted on {self.n_features_in_}")
        bits = _Bits(X, [float(self.binarize)], self.device, planes=False, who=self._who)
        return bits.jll_device(self._w[None], self._c[None], [0], [None])[0], bits.was_numpy

    def predict_joint_log_proba(self, X):
        out, was_numpy = self._jll(X)
        return out.cpu().numpy() if was_numpy else out

    def predict_log_proba(self, X):
        """``jll - logsumexp(jll, axis=1)``, scikit-learn's expression, on the host whatever the input was."""
        from scipy.special import logsumexp
        out, was_numpy = self._jll(X)
        jll = out.cpu().numpy()
        logp = jll - np.atleast_2d(logsumexp(jll, axis=1)).T
        return logp if was_numpy else torch.from_numpy(logp).to(out.device)

    def predict_proba(self, X):
        logp = self.predict_log_proba(X)
        return np.exp(logp) if isinstance(logp, np.ndarray) else torch.from_numpy(np.exp(logp.cpu().numpy())).to(logp.device)

    def predict(self, X):
        """numpy labels of ``classes_``' dtype: the larger joint log-likelihood, ``classes_[0]`` on a tie."""
        jll = self._jll(X)[0].cpu().numpy()
        return self.classes_[np.argmax(jll, axis=1)]

    def score(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise ValueError(f"{self._who}: sample_weight is not supported")
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        return float(np.mean(self.predict(X) == y))


def _model(classes, fc, cc, alpha, binarize, fit_prior, class_prior, force_alpha, device):
    est = BernoulliNB(alpha, binarize, fit_prior, class_prior, force_alpha=force_alpha, device=device)
    return est._adopt(classes, fc, cc, *tables(fc, cc, alpha, fit_prior, class_prior, force_alpha))


def _thresholds(values):
    """(distinct thresholds in order of appearance, every value's index among them)."""
    distinct = list(dict.fromkeys(float(v) for v in values))
    return distinct, [distinct.index(float(v)) for v in values]


def fit_masks(X, y, rows, binarize, alpha, *, fit_prior=True, class_prior=None, force_alpha=True, device="cuda", backend=None, who="naive_bayes.fit_masks"):
    """Fit ``BernoulliNB(alpha=a, binarize=b).fit(X[r], y[r])`` for every r of ``rows`` (integer index arrays without repeats, ``None``:
    all rows), b of ``binarize`` and a of ``alpha``, in ``itertools.product(rows, binarize, alpha)`` order: one pack, one count launch
    and one host read of the counts for all of them.  Every model equals the single fit bit for bit."""
    binarize, alpha, rows = list(binarize), list(alpha), list(rows)
    for a in alpha:
        _check_alpha(a, who)
    for b in binarize:
        _check_binarize(b, who)
    _check_class_prior(class_prior, who)
    if backend is None:
        _check_device(device, who)
    if not (rows and binarize and alpha):
        raise ValueError(f"{who}: rows, binarize and alpha must each hold one entry at least")
    n, _ = _check_input(X, who)
    classes, y01 = _binary_labels(y, n, who)
    row_lists = _row_lists(rows, n, y01, who)
    distinct, index = _thresholds(binarize)
    count, _ = (backend or device_backend(device))(X, distinct)
    pairs = [(m, t) for m in range(len(row_lists)) for t in range(len(distinct))]
    fc, cc = count(row_lists, y01, pairs)
    return [_model(classes, fc[m * len(distinct) + index[bi]], cc[m], a, binarize[bi], fit_prior, class_prior, force_alpha, device)
            for m in range(len(row_lists)) for bi in range(len(binarize)) for a in alpha]


def _grid_points(param_grid, who):
    points = []
    for sub in ([param_grid] if isinstance(param_grid, dict) else list(param_grid)):      # a list of grids: one after the other, as ParameterGrid
        unknown = set(sub) - {"alpha", "binarize", "fit_prior"}
        if unknown:
            raise ValueError(f"{who}: unsupported grid keys {sorted(unknown)}")
        keys = sorted(sub)
        points += [dict(zip(keys, vals)) for vals in itertools.product(*(sub[k] for k in keys))]
    if not points:
        raise ValueError(f"{who}: the grid is empty")
    full = [(pt.get("alpha", 1.0), pt.get("binarize", 0.0), pt.get("fit_prior", True)) for pt in points]
    for a, b, _ in full:
        _check_alpha(a, who)
        _check_binarize(b, who)
    return points, full


def grid_search_cv(X, y, param_grid, cv: int = 5, device="cuda", *, backend=None):
    """The reference's ``GridSearchCV(BernoulliNB(), param_grid, cv=5, scoring='f1')`` (model_maccs.py:257-267) over ``alpha``,
    ``binarize`` and ``fit_prior``.

    Same conventions as ``svm.grid_search_cv``: sorted keys, ``itertools.product`` order, scikit-learn's ``StratifiedKFold(cv)``,
    ``f1_score`` of ``classes_[1]``, the first maximum wins; ``param_grid`` is a dict or a list of dicts.  X is packed once for the
    grid's distinct thresholds; the training rows of every fold and, for the refit, all rows are counted in one launch (alpha and
    ``fit_prior`` share counts); every (fold, point) scores its test rows in one more.
    Returns (best_params, mean F1 per point, the classifier refitted on all rows with best_params)."""
    from sklearn.model_selection import StratifiedKFold
    who = "naive_bayes.grid_search_cv"
    points, full = _grid_points(param_grid, who)
    if backend is None:
        _check_device(device, who)
    n, _ = _check_input(X, who)
    classes, y01 = _binary_labels(y, n, who)
    folds = list(StratifiedKFold(n_splits=cv).split(np.zeros((n, 1)), y01))
    row_lists = _row_lists([tr for tr, _ in folds] + [None], n, y01, who)
    distinct, index = _thresholds([b for _, b, _ in full])
    T = len(distinct)
    count, jll = (backend or device_backend(device))(X, distinct)
    fc, cc = count(row_lists, y01, [(m, t) for m in range(len(row_lists)) for t in range(T)])
    fits = [[_model(classes, fc[fi * T + index[pi]], cc[fi], a, b, fp, None, True, device) for pi, (a, b, fp) in enumerate(full)]
            for fi in range(len(folds))]
    flat = [(fi, pi) for fi in range(len(folds)) for pi in range(len(full))]
    got = jll(np.stack([fits[fi][pi]._w for fi, pi in flat]), np.stack([fits[fi][pi]._c for fi, pi in flat]), [index[pi] for _, pi in flat],
              [folds[fi][1] for fi, _ in flat])
    f1 = np.zeros((len(full), len(folds)))
    for (fi, pi), s in zip(flat, got):
        f1[pi, fi] = f1_binary(y01[folds[fi][1]], np.argmax(s, axis=1))
    scores = [float(v) for v in f1.mean(axis=1)]
    best = int(np.argmax(scores))
    a, b, fp = full[best]
    fitted = _model(classes, fc[len(folds) * T + index[best]], cc[len(folds)], a, b, fp, None, True, device)
    return points[best], scores, fitted


def learning_curve(params, X, y, cv: int = 5, train_sizes=np.linspace(0.1, 1.0, 5), scoring="f1", device="cuda", *, backend=None):
    """``sklearn.model_selection.learning_curve(BernoulliNB(**params), X, y, cv=cv, train_sizes=train_sizes, scoring=scoring)`` without
    shuffling (model_maccs.py draws it with ``cv=6`` and five sizes): folds of ``StratifiedKFold(cv)``, absolute sizes by scikit-learn's
    ``_translate_train_sizes`` on the first fold's training rows (as scikit-learn does; with stratified folds no training fold is
    larger), every fit on the prefix ``train[:size]`` of a fold's training rows, scored on that prefix and on the fold's test rows.
    ``scoring`` is "f1" (of ``classes_[1]``) or "accuracy".  All prefixes of all folds are one batch: one pack, one count launch, one
    jll launch.  Returns (train_sizes_abs, train_scores [sizes, folds], test_scores [sizes, folds])."""
    from sklearn.model_selection import StratifiedKFold
    from sklearn.model_selection._validation import _translate_train_sizes
    who = "naive_bayes.learning_curve"
    params = dict(params)
    unknown = set(params) - {"alpha", "binarize", "fit_prior", "class_prior", "force_alpha"}
    if unknown:
        raise ValueError(f"{who}: unsupported parameters {sorted(unknown)}")
    if scoring not in ("f1", "accuracy"):
        raise ValueError(f"{who}: scoring must be 'f1' or 'accuracy', got {scoring!r}")
    alpha, binarize = params.get("alpha", 1.0), params.get("binarize", 0.0)
    fit_prior, class_prior, force_alpha = params.get("fit_prior", True), params.get("class_prior"), params.get("force_alpha", True)
    _check_alpha(alpha, who)
    _check_binarize(binarize, who)
    _check_class_prior(class_prior, who)
    if backend is None:
        _check_device(device, who)
    n, _ = _check_input(X, who)
    classes, y01 = _binary_labels(y, n, who)
    folds = list(StratifiedKFold(n_splits=cv).split(np.zeros((n, 1)), y01))
    sizes = _translate_train_sizes(train_sizes, len(folds[0][0]))
    prefixes = [(fi, si, tr[:size]) for fi, (tr, _) in enumerate(folds) for si, size in enumerate(sizes)]
    row_lists = _row_lists([r for _, _, r in prefixes], n, y01, who)
    count, jll = (backend or device_backend(device))(X, [float(binarize)])
    fc, cc = count(row_lists, y01, [(m, 0) for m in range(len(row_lists))])
    fits = [_model(classes, fc[m], cc[m], alpha, binarize, fit_prior, class_prior, force_alpha, device) for m in range(len(row_lists))]
    w, c = np.stack([f._w for f in fits]), np.stack([f._c for f in fits])
    got = jll(np.concatenate([w, w]), np.concatenate([c, c]), [0] * (2 * len(fits)), row_lists + [folds[fi][1] for fi, _, _ in prefixes])
    train_scores, test_scores = np.zeros((len(sizes), len(folds))), np.zeros((len(sizes), len(folds)))
    for m, (fi, si, _) in enumerate(prefixes):
        train_scores[si, fi] = _score(scoring, y01[row_lists[m]], np.argmax(got[m], axis=1))
        test_scores[si, fi] = _score(scoring, y01[folds[fi][1]], np.argmax(got[len(fits) + m], axis=1))
    return sizes, train_scores, test_scores
