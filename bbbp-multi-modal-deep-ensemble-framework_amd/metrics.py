"""``sklearn.metrics`` for the GPU, batched: the scores of all columns (models, grid points) over all row segments (folds) in a fixed,
small number of launches.

Every classification script of the reference ends in ``evaluate_model`` (``Models/model_maccs.py``, ``model_opt*.py``): accuracy,
balanced accuracy, precision, recall, F1, Matthews' correlation, Cohen's kappa and ROC AUC per fitted model, the last from
``predict_proba(X)[:, 1]`` or, where a model has none, from the hard predictions; every regression script ends in
``mean_squared_error`` and ``r2_score``.  Seven of the eight classification scores are functions of the four confusion counts and the
AUC with ties is a pair count, so the device computes integers and the host a dozen float64 expressions (``csrc/metrics.hip``):

* ``bbbp_metrics_confusion``: (tn, fp, fn, tp) per (column, segment) as int64 from 0/1 bytes, or from scores with one strict threshold per
  column.  One launch up to 16 384 rows, two beyond.
* ``bbbp_metrics_auc_pairs``: ``U2 = sum over positives i of #{negatives < s_i} + #{negatives <= s_i}``, the class sizes P and N and the
  count of non-finite scores per (column, segment), by visiting every pair of rows: no sort, no row limit, exact for any n, and
  **quadratic** in n (n^2 / 256 LDS tile passes per column; 1.6e7 pairs per column at the reference's 7 807 rows).  Two launches.
  ``AUC = U2 / (2 P N)``, the exact value rounded once; scikit-learn sums a trapezoid rule in floating point and differs by a few ulp.
* ``bbbp_metrics_sq_sums``: ``sum (y - p)^2`` per (column, segment) and, once per segment, ``sum y``, ``sum (y - ybar)^2`` and the row
  count, in float64 in a fixed order that ``tests/metrics_numpy.py`` reproduces bit for bit.  One launch.

``scores_from_counts`` holds scikit-learn 1.7's expressions on the integer counts; on two-class problems its seven scores are
scikit-learn's bit for bit.  It, the AUC division and the MSE / R2 divisions run on the host and need no GPU.

The layout is that of cross-validated predictions: ``y_pred`` / ``y_score`` are ``[M, n]`` (or 1-D), ``groups`` gives every row a segment
id in ``[0, G)`` or -1 for "left out", results are ``[M, G]``.  A segment is scored as scikit-learn would score its rows alone; an empty
segment gives NaN in every score and zero counts.  The batched calls do not warn; the scalar drop-ins warn as scikit-learn does.

Not built, each refused by name: more than two classes, ``sample_weight``, ``average`` other than ``'binary'``, ``adjusted=True``,
``weights`` in kappa, ``max_fpr``, multi-output targets, ``roc_curve`` / ``precision_recall_curve``, ``log_loss``, more than 64 segments,
more than one GPU.  There is no CPU path for the counting.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _dense, _lib

MAX_COLUMNS, MAX_GROUPS, TILE_ROWS, PAIR_ROWS, MAX_ROWS = 65535, 64, 16384, 256, 2147483647      # BBBP_METRICS_*
_U8 = 2                                                                                          # BBBP_METRICS_DTYPE_U8
_LAUNCHES = {"confusion": 0, "pairs": 0, "sum": 0, "sq_sums": 0}      # launches of this process (tests and the bench tool count them)
KEYS = ("Accuracy", "Balanced Accuracy", "Precision", "Recall", "F1 Score", "MCC", "Cohen's Kappa", "ROC AUC")

try:
    from sklearn.exceptions import UndefinedMetricWarning
except ImportError:                                                   # scikit-learn is needed by the grid searches only
    class UndefinedMetricWarning(UserWarning):
        pass


# ---- the host expressions: scikit-learn's, on integer counts --------------------------------------------------------------------------
def _zero_division_value(zero_division, who="metrics"):
    if isinstance(zero_division, str):
        if zero_division == "warn":
            return 0.0
    elif zero_division in (0, 1) and not isinstance(zero_division, bool):
        return float(zero_division)
    raise ValueError(f"{who}: zero_division must be 0, 1 or 'warn', got {zero_division!r}")


def scores_from_counts(counts, zero_division="warn"):
    """The seven count scores as float64 arrays of ``counts.shape[:-1]`` from integer (tn, fp, fn, tp) in the last axis, with
    scikit-learn 1.7's float64 expressions: ``Accuracy`` (tp + tn) / n; ``Recall`` tp / (tp + fn); ``Precision`` tp / (tp + fp);
    ``F1 Score`` 2 tp / ((tp + fn) + (tp + fp)), the three with ``zero_division`` on a zero denominator; ``Balanced Accuracy`` the mean
    of the recalls of the classes present in ``y_true``; ``MCC`` (c s - t.p) / sqrt((s^2 - p.p) (s^2 - t.t)) or 0 when a factor is 0;
    ``Cohen's Kappa`` 1 - (fp + fn) / (expected[0, 1] + expected[1, 0]) (NaN when both are 0, as scikit-learn).  All zero: NaN."""
    zd = _zero_division_value(zero_division, "scores_from_counts")
    c = np.asarray(counts)
    if c.ndim < 1 or c.shape[-1] != 4 or c.dtype.kind not in "iu":
        raise ValueError(f"scores_from_counts: integer counts with (tn, fp, fn, tp) in the last axis are expected, got {c.dtype} {c.shape}")
    c = c.astype(np.int64)
    if c.size and c.min() < 0:
        raise ValueError("scores_from_counts: a count is negative")
    tn, fp, fn, tp = (c[..., k] for k in range(4))
    n = tn + fp + fn + tp
    empty = n == 0

    def ratio(num, den, on_zero):
        den = np.asarray(den, dtype=np.float64)
        zero = den == 0
        out = np.asarray(num, dtype=np.float64) / np.where(zero, 1.0, den)
        return np.where(zero, on_zero, out)

    out = {"Accuracy": ratio(tp + tn, n, np.nan)}
    recall, specificity = ratio(tp, tp + fn, np.nan), ratio(tn, tn + fp, np.nan)
    both = (recall + specificity) / 2
    out["Balanced Accuracy"] = np.where(np.isnan(recall), specificity, np.where(np.isnan(specificity), recall, both))
    out["Precision"] = ratio(tp, tp + fp, zd)
    out["Recall"] = ratio(tp, tp + fn, zd)
    out["F1 Score"] = ratio(2 * tp, (tp + fn) + (tp + fp), zd)
    # matthews_corrcoef: float64 throughout, as C.sum(dtype=float64), np.trace(dtype=float64) and np.dot give them
    t0, t1, p0, p1 = ((tn + fp).astype(np.float64), (fn + tp).astype(np.float64), (tn + fn).astype(np.float64), (fp + tp).astype(np.float64))
    s = p0 + p1
    cov_ytyp = (tn + tp).astype(np.float64) * s - (t0 * p0 + t1 * p1)
    cov_ypyp = s ** 2 - (p0 * p0 + p1 * p1)
    cov_ytyt = s ** 2 - (t0 * t0 + t1 * t1)
    prod = cov_ypyp * cov_ytyt
    with np.errstate(divide="ignore", invalid="ignore"):
        out["MCC"] = np.where(prod == 0, 0.0, cov_ytyp / np.sqrt(np.where(prod == 0, 1.0, prod)))
        # cohen_kappa_score: expected = outer(column sums, row sums) / n with integer products, k = (fp + fn) / (e01 + e10)
        nf = np.where(empty, 1, n)
        e01, e10 = ((tn + fn) * (fn + tp)) / nf, ((fp + tp) * (tn + fp)) / nf
        out["Cohen's Kappa"] = 1 - (fp + fn) / (e01 + e10)
    for k in out:
        out[k] = np.where(empty, np.nan, out[k]).astype(np.float64)
    return out


def auc_from_pairs(u2, pos, neg):
    """``U2 / (2 P N)`` per element, the exact rational rounded once (Python integer division); NaN where a class is absent."""
    u2, pos, neg = np.asarray(u2), np.asarray(pos), np.asarray(neg)
    out = np.full(u2.shape, np.nan)
    for at in np.ndindex(u2.shape):
        p, q = int(pos[at]), int(neg[at])
        if p and q:
            out[at] = int(u2[at]) / (2 * p * q)
    return out


def pairs_from_counts(counts):
    """(U2, P, N) of hard 0/1 predictions used as scores, from (tn, fp, fn, tp): a predicted positive lies above every predicted negative
    and ties with the others, so ``U2 = tp (2 tn + fp) + fn tn``."""
    c = np.asarray(counts).astype(object)
    tn, fp, fn, tp = (c[..., k] for k in range(4))
    return tp * (2 * tn + fp) + fn * tn, tp + fn, tn + fp


def regression_from_sums(sse, ystat):
    """``{"MSE": sse / count, "R2": 1 - sse / sum (y - ybar)^2}`` from the device's sums; R2 as scikit-learn with ``force_finite``: a zero
    denominator gives 1.0 for a zero numerator and 0.0 otherwise, fewer than two rows give NaN.  An empty segment: NaN in both."""
    sse, ystat = np.asarray(sse, dtype=np.float64), np.asarray(ystat, dtype=np.float64)
    count, den = ystat[:, 2][None, :], ystat[:, 1][None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = np.where(count > 0, sse / np.where(count > 0, count, 1.0), np.nan)
        r2 = np.where(den != 0, 1 - sse / np.where(den != 0, den, 1.0), np.where(sse == 0, 1.0, 0.0))
    return {"MSE": mse, "R2": np.where(count >= 2, r2, np.nan)}


# ---- argument checks: nothing here touches the GPU -----------------------------------------------------------------------------------
def _to_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _check_device(device, *inputs, who):
    for t in inputs:
        if isinstance(t, torch.Tensor) and t.is_cuda and device is None:
            device = t.device
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError(f"{who}: device {device!r}: the counting runs on the GPU (no CPU fallback)")
    return device


def _truth(y_true, who):
    y = _to_numpy(y_true)
    if y.ndim == 2 and y.shape[1] == 1:
        y = y[:, 0]
    if y.ndim != 1:
        raise NotImplementedError(f"{who}: multi-output targets are not supported (y_true has shape {y.shape})")
    if not 1 <= len(y) <= MAX_ROWS:
        raise ValueError(f"{who}: y_true has {len(y)} rows, 1 .. {MAX_ROWS} are supported")
    if y.dtype.kind == "f" and not np.all(np.isfinite(y)):
        raise ValueError(f"{who}: y_true contains NaN or infinity")
    return y


def _columns(a, n, who, name):
    """[M, n] view of a 1-D or 2-D numpy array or tensor."""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2:
        raise ValueError(f"{who}: {name} must be 1-D or [M, n], got shape {tuple(a.shape)}")
    if a.shape[1] != n:
        raise ValueError(f"{who}: y_true has {n} rows, {name} has {a.shape[1]} per column")
    if not 1 <= a.shape[0] <= MAX_COLUMNS:
        raise ValueError(f"{who}: {a.shape[0]} columns, 1 .. {MAX_COLUMNS} are supported (BBBP_METRICS_MAX_COLUMNS)")
    return a


def _groups(groups, n, who):
    """(int32 segment ids or None, G)."""
    if groups is None:
        return None, 1
    g = _to_numpy(groups)
    if g.ndim != 1 or len(g) != n or g.dtype.kind not in "iu":
        raise ValueError(f"{who}: groups must be {n} integer segment ids (-1: the row is left out)")
    if g.min() < -1:
        raise ValueError(f"{who}: a segment id is below -1")
    G = max(int(g.max()) + 1, 1)
    if G > MAX_GROUPS:
        raise ValueError(f"{who}: {G} segments, at most {MAX_GROUPS} are supported (BBBP_METRICS_MAX_GROUPS)")
    return g.astype(np.int32), G


def _distinct(a):
    """``np.unique(a)``, without the sort where a numeric array holds two values at most (a grid's predictions are a million labels)."""
    a = np.asarray(a)
    if a.size and a.dtype.kind in "iub":
        lo, hi = a.min(), a.max()
        if lo == hi or np.count_nonzero(a == lo) + np.count_nonzero(a == hi) == a.size:
            return np.unique(np.array([lo, hi]))
    return np.unique(a)


def _classes(y, pred_unique, pos_label, who):
    """The sorted union of the labels, checked as scikit-learn checks a binary problem."""
    classes = np.unique(np.concatenate([np.unique(y), np.asarray(pred_unique)])) if pred_unique is not None else np.unique(y)
    if classes.dtype.kind == "f" and not np.all(np.isfinite(classes)):
        raise ValueError(f"{who}: the labels contain NaN or infinity")
    if len(classes) > 2:
        raise ValueError(f"{who}: {len(classes)} classes ({classes[:5].tolist()} ...): more than two classes are not supported")
    if pos_label is not None and len(classes) == 2 and not np.any(classes == pos_label):
        raise ValueError(f"{who}: pos_label={pos_label!r} is not a valid label. It should be one of {classes.tolist()}")
    return classes


def _refuse(who, **given):
    """NotImplementedError for every argument that is not at its default."""
    for name, (value, default) in given.items():
        if not (value is default or (isinstance(default, (str, bool, int)) and type(value) is type(default) and value == default)):
            raise NotImplementedError(f"{who}: {name}={value!r} is not supported (only {name}={default!r} is built)")


# ---- the device calls ---------------------------------------------------------------------------------------------------------------------
class _Problem:
    """y_true as 0/1 bytes and the segment ids on the device."""

    def __init__(self, y01, seg, G, dev):
        self.dev, self.G, self.n = dev, G, len(y01)
        self.y01 = torch.from_numpy(np.ascontiguousarray(y01, dtype=np.uint8)).to(dev)
        self.seg = None if seg is None else torch.from_numpy(seg).to(dev)

    def seg_ptr(self):
        return None if self.seg is None else self.seg.data_ptr()


def _pred_bytes(y_pred, y, pos_label, dev, who):
    """Hard predictions [M, n] as 0/1 bytes on the device and the classes of the problem, checked before anything is copied."""
    if isinstance(y_pred, torch.Tensor):
        if not y_pred.is_cuda:
            raise RuntimeError(f"{who}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {y_pred.device} (no CPU fallback)")
        y_pred = y_pred.to(dev)
        uniq = torch.unique(y_pred).cpu().numpy()
        classes = _classes(y, uniq, pos_label, who)
        in_place = y_pred.dtype == torch.uint8 and pos_label == 1 and set(uniq.tolist()) <= {0, 1} and (y_pred.shape[1] == 1 or y_pred.stride(1) == 1) \
            and (y_pred.shape[0] == 1 or y_pred.stride(0) >= y_pred.shape[1])
        return (y_pred if in_place else (y_pred == pos_label).to(torch.uint8).contiguous()), classes
    classes = _classes(y, _distinct(y_pred), pos_label, who)
    return torch.from_numpy(np.ascontiguousarray(y_pred == pos_label).astype(np.uint8)).to(dev), classes


def _device_counts(prob, pred, thr, scores):
    """One host read for a batch: (counts [M, G, 4] or None, pairs [M, G, 4] or None) as int64 numpy; raises on a non-finite score.
    ``pred``: byte tensor, or a float tensor with ``thr``; ``scores``: a float or byte tensor for the pair counts."""
    dev, G, n = prob.dev, prob.G, prob.n
    L = _lib.lib()
    with torch.cuda.device(dev):
        Mc = 0 if pred is None else int(pred.shape[0])
        Ms = 0 if scores is None else int(scores.shape[0])
        wc, ws = Mc * G * 4, Ms * G * 4
        buf = torch.empty(wc + ws + 1, dtype=torch.int64, device=dev)
        flag = buf[wc + ws:]
        flag.zero_()
        if pred is not None:
            dtype = _U8 if pred.dtype == torch.uint8 else _dense.DT[pred.dtype]
            nbytes = L.bbbp_metrics_work_bytes(0, Mc, n, G)
            work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev) if nbytes else None
            thr_d = None if thr is None else torch.from_numpy(np.array(thr, dtype=np.float64)).to(dev)
            _lib.check(L.bbbp_metrics_confusion(_dense.stream(), pred.data_ptr(), dtype, _dense.ld(pred), Mc, n, None if thr_d is None else thr_d.data_ptr(),
                                                prob.y01.data_ptr(), prob.seg_ptr(), G, buf.data_ptr(), None if work is None else work.data_ptr(),
                                                flag.data_ptr()), "bbbp_metrics_confusion")
            _LAUNCHES["confusion"] += 1
            _LAUNCHES["sum"] += 1 if nbytes else 0
        if scores is not None:
            dtype = _U8 if scores.dtype == torch.uint8 else _dense.DT[scores.dtype]
            work = torch.empty(L.bbbp_metrics_work_bytes(1, Ms, n, G) // 8, dtype=torch.int64, device=dev)
            _lib.check(L.bbbp_metrics_auc_pairs(_dense.stream(), scores.data_ptr(), dtype, _dense.ld(scores), Ms, n, prob.y01.data_ptr(), prob.seg_ptr(),
                                                G, buf[wc:].data_ptr(), work.data_ptr()), "bbbp_metrics_auc_pairs")
            _LAUNCHES["pairs"] += 1
            _LAUNCHES["sum"] += 1
        host = buf.cpu().numpy()
    counts = host[:wc].reshape(Mc, G, 4) if pred is not None else None
    pairs = host[wc:wc + ws].reshape(Ms, G, 4) if scores is not None else None
    if host[-1] != 0 or (pairs is not None and pairs[..., 3].any()):
        raise ValueError("metrics: the scores contain NaN or infinity")
    return counts, pairs


def _score_matrix(a, n, dev, who, name):
    a = _columns(a, n, who, name)
    if not isinstance(a, torch.Tensor) and np.asarray(a).dtype.kind not in "fiub":
        raise ValueError(f"{who}: {name} must be numeric, got dtype {np.asarray(a).dtype}")
    if isinstance(a, np.ndarray) and not a.flags.writeable:
        a = a.copy()                                          # torch refuses to wrap a read-only array without a warning
    return _dense.to_device_matrix(a, dev, who, allow_row_stride=True)[0]


# ---- the batched entry points -------------------------------------------------------------------------------------------------------------
def confusion_counts(y_true, y_pred, *, pos_label=1, groups=None, threshold=None, device=None):
    """int64 ndarray ``[M, G, 4]`` of (tn, fp, fn, tp), positive = ``pos_label``.  ``y_pred``: hard labels 1-D or ``[M, n]``; with
    ``threshold`` (one number, or one per column) it holds scores instead and the prediction is ``score > threshold`` (strict, compared
    in float64), the classes then being those of ``y_true``."""
    who = "metrics.confusion_counts"
    dev = _check_device(device, y_pred, who=who)
    y = _truth(y_true, who)
    seg, G = _groups(groups, len(y), who)
    if threshold is None:
        pred, _ = _pred_bytes(_columns(y_pred, len(y), who, "y_pred"), y, pos_label, dev, who)
        thr = None
    else:
        _classes(y, None, pos_label, who)
        M = _columns(y_pred, len(y), who, "y_pred").shape[0]
        thr = np.asarray(threshold, dtype=np.float64)
        if thr.shape not in ((), (1,), (M,)) or not np.all(np.isfinite(thr)):
            raise ValueError(f"{who}: threshold must be one finite number, or one per column")
        thr = np.broadcast_to(thr, (M,))
        pred = _score_matrix(y_pred, len(y), dev, who, "y_pred")
    return _device_counts(_Problem(y == pos_label, seg, G, dev), pred, thr, None)[0]


def classification_scores(y_true, y_pred, y_score=None, *, pos_label=1, groups=None, zero_division="warn", device=None):
    """The reference's eight scores as float64 arrays ``[M, G]`` under ``KEYS``.  ``y_pred``: hard labels, 1-D or ``[M, n]``; ``y_score``:
    scores of the greater class (``predict_proba(X)[:, 1]``), same shape, float32 or float64; ``None``: the AUC is that of the hard
    predictions used as scores, as ``evaluate_model`` does for a model without ``predict_proba`` (then from the counts: no further
    launch).  The seven count scores take ``pos_label`` as the positive class, the AUC the greater label, as ``roc_auc_score`` does."""
    who = "metrics.classification_scores"
    _zero_division_value(zero_division, who)
    dev = _check_device(device, y_pred, y_score, who=who)
    y = _truth(y_true, who)
    seg, G = _groups(groups, len(y), who)
    pred, classes = _pred_bytes(_columns(y_pred, len(y), who, "y_pred"), y, pos_label, dev, who)
    scores = None if y_score is None else _score_matrix(y_score, len(y), dev, who, "y_score")
    if scores is not None and scores.shape[0] != pred.shape[0]:
        raise ValueError(f"{who}: y_pred has {pred.shape[0]} columns, y_score {scores.shape[0]}")
    prob = _Problem(y == pos_label, seg, G, dev)
    lesser = len(classes) == 2 and classes[0] == pos_label          # the AUC's positive class is classes[1] whatever pos_label says
    if scores is not None and lesser:
        counts = _device_counts(prob, pred, None, None)[0]
        pairs = _device_counts(_Problem(y != pos_label, seg, G, dev), None, None, scores)[1]
    else:
        counts, pairs = _device_counts(prob, pred, None, scores)
    out = scores_from_counts(counts, zero_division)
    if scores is None:
        c = counts[..., ::-1] if lesser else counts                  # (tp, fn, fp, tn) of the lesser class is (tn, fp, fn, tp) of the greater
        out["ROC AUC"] = auc_from_pairs(*pairs_from_counts(c))
    else:
        out["ROC AUC"] = auc_from_pairs(pairs[..., 0], pairs[..., 1], pairs[..., 2])
    return out


def auc_pair_counts(y_true, y_score, *, groups=None, device=None):
    """int64 ndarray ``[M, G, 3]`` of (U2, P, N) with the greater label of ``y_true`` as the positive class: ``AUC = U2 / (2 P N)``."""
    who = "metrics.auc_pair_counts"
    dev = _check_device(device, y_score, who=who)
    y = _truth(y_true, who)
    seg, G = _groups(groups, len(y), who)
    classes = _classes(y, None, None, who)
    scores = _score_matrix(y_score, len(y), dev, who, "y_score")
    return _device_counts(_Problem(y == classes[-1] if len(classes) == 2 else np.zeros(len(y), bool), seg, G, dev), None, None, scores)[1][..., :3]


def squared_error_sums(y_true, y_pred, *, groups=None, device=None):
    """(sse float64 ``[M, G]``, ystat float64 ``[G, 3]`` = (sum y, sum (y - ybar)^2, count)): the device's sums as they are."""
    who = "metrics.regression_scores"
    dev = _check_device(device, y_pred, who=who)
    y = _truth(y_true, who)
    if y.dtype.kind not in "fiub":
        raise ValueError(f"{who}: y_true must be numeric, got dtype {y.dtype}")
    seg, G = _groups(groups, len(y), who)
    a = y_pred if isinstance(y_pred, torch.Tensor) else np.asarray(y_pred)
    if a.ndim == 2 and a.shape[0] == len(y) and a.shape[1] == 1 and len(y) != 1:
        a = a[:, 0]
    pred = _score_matrix(a, len(y), dev, who, "y_pred")
    M, n = int(pred.shape[0]), len(y)
    with torch.cuda.device(dev):
        yd = torch.from_numpy(np.array(y, dtype=np.float64)).to(dev)
        sd = None if seg is None else torch.from_numpy(seg).to(dev)
        buf = torch.empty(M * G + 3 * G + 1, dtype=torch.float64, device=dev)
        flag = buf[M * G + 3 * G:]
        flag.zero_()
        _lib.check(_lib.lib().bbbp_metrics_sq_sums(_dense.stream(), pred.data_ptr(), _dense.DT[pred.dtype], _dense.ld(pred), M, n, yd.data_ptr(),
                                                   None if sd is None else sd.data_ptr(), G, buf.data_ptr(), buf[M * G:].data_ptr(), flag.data_ptr()),
                   "bbbp_metrics_sq_sums")
        _LAUNCHES["sq_sums"] += 1
        host = buf.cpu().numpy()
    if host[-1:].view(np.int64)[0] != 0:
        raise ValueError(f"{who}: y_true or y_pred contains NaN or infinity")
    return host[:M * G].reshape(M, G), host[M * G:M * G + 3 * G].reshape(G, 3)


def regression_scores(y_true, y_pred, *, groups=None, device=None):
    """``{"MSE": [M, G], "R2": [M, G]}`` of ``mean_squared_error`` and ``r2_score`` per (column, segment): one launch, one host read."""
    return regression_from_sums(*squared_error_sums(y_true, y_pred, groups=groups, device=device))


# ---- scikit-learn's scalar functions ----------------------------------------------------------------------------------------------------
def _scalar(key, who, y_true, y_pred, pos_label, zero_division="warn", device=None):
    _zero_division_value(zero_division, who)
    y = _truth(y_true, who)
    a = y_pred if isinstance(y_pred, torch.Tensor) else np.asarray(y_pred)
    if a.ndim != 1 and not (a.ndim == 2 and a.shape[1] == 1):
        raise NotImplementedError(f"{who}: multi-output targets are not supported (y_pred has shape {tuple(a.shape)})")
    counts = confusion_counts(y, a.reshape(-1), pos_label=pos_label, device=device)
    tn, fp, fn, tp = (int(v) for v in counts[0, 0])
    if zero_division == "warn":
        ill = {"Precision": (tp + fp == 0, "Precision is ill-defined and being set to 0.0 due to no predicted samples."),
               "Recall": (tp + fn == 0, "Recall is ill-defined and being set to 0.0 due to no true samples."),
               "F1 Score": (2 * tp + fp + fn == 0, "F-score is ill-defined and being set to 0.0 due to no true nor predicted samples.")}
        if key in ill and ill[key][0]:
            warnings.warn(ill[key][1] + " Use `zero_division` parameter to control this behavior.", UndefinedMetricWarning, stacklevel=3)
    if key == "Balanced Accuracy" and (tp + fn == 0 or tn + fp == 0):
        warnings.warn("y_pred contains classes not in y_true", stacklevel=3)
    return float(scores_from_counts(counts, zero_division)[key][0, 0])


def accuracy_score(y_true, y_pred, *, normalize=True, sample_weight=None, device=None):
    _refuse("metrics.accuracy_score", normalize=(normalize, True), sample_weight=(sample_weight, None))
    y = _truth(y_true, "metrics.accuracy_score")
    return _scalar("Accuracy", "metrics.accuracy_score", y, y_pred, np.unique(y)[-1], device=device)


def balanced_accuracy_score(y_true, y_pred, *, sample_weight=None, adjusted=False, device=None):
    _refuse("metrics.balanced_accuracy_score", sample_weight=(sample_weight, None), adjusted=(adjusted, False))
    y = _truth(y_true, "metrics.balanced_accuracy_score")
    return _scalar("Balanced Accuracy", "metrics.balanced_accuracy_score", y, y_pred, np.unique(y)[-1], device=device)


def precision_score(y_true, y_pred, *, labels=None, pos_label=1, average="binary", sample_weight=None, zero_division="warn", device=None):
    _refuse("metrics.precision_score", labels=(labels, None), average=(average, "binary"), sample_weight=(sample_weight, None))
    return _scalar("Precision", "metrics.precision_score", y_true, y_pred, pos_label, zero_division, device)


def recall_score(y_true, y_pred, *, labels=None, pos_label=1, average="binary", sample_weight=None, zero_division="warn", device=None):
    _refuse("metrics.recall_score", labels=(labels, None), average=(average, "binary"), sample_weight=(sample_weight, None))
    return _scalar("Recall", "metrics.recall_score", y_true, y_pred, pos_label, zero_division, device)


def f1_score(y_true, y_pred, *, labels=None, pos_label=1, average="binary", sample_weight=None, zero_division="warn", device=None):
    _refuse("metrics.f1_score", labels=(labels, None), average=(average, "binary"), sample_weight=(sample_weight, None))
    return _scalar("F1 Score", "metrics.f1_score", y_true, y_pred, pos_label, zero_division, device)


def matthews_corrcoef(y_true, y_pred, *, sample_weight=None, device=None):
    _refuse("metrics.matthews_corrcoef", sample_weight=(sample_weight, None))
    y = _truth(y_true, "metrics.matthews_corrcoef")
    return _scalar("MCC", "metrics.matthews_corrcoef", y, y_pred, np.unique(y)[-1], device=device)


def cohen_kappa_score(y1, y2, *, labels=None, weights=None, sample_weight=None, device=None):
    _refuse("metrics.cohen_kappa_score", labels=(labels, None), weights=(weights, None), sample_weight=(sample_weight, None))
    y = _truth(y1, "metrics.cohen_kappa_score")
    with np.errstate(invalid="ignore"):
        return _scalar("Cohen's Kappa", "metrics.cohen_kappa_score", y, y2, np.unique(y)[-1], device=device)


def confusion_matrix(y_true, y_pred, *, labels=None, sample_weight=None, normalize=None, device=None):
    """``[[tn, fp], [fn, tp]]`` over the sorted labels (int64); 1 x 1 when ``y_true`` and ``y_pred`` hold one label between them."""
    who = "metrics.confusion_matrix"
    _refuse(who, labels=(labels, None), sample_weight=(sample_weight, None), normalize=(normalize, None))
    y, p = _truth(y_true, who), _truth(y_pred, who)
    classes = _classes(y, np.unique(p), None, who)
    counts = confusion_counts(y, y_pred, pos_label=classes[-1], device=device)[0, 0]
    return counts.reshape(2, 2) if len(classes) == 2 else counts[3:].reshape(1, 1)


def roc_auc_score(y_true, y_score, *, average="macro", sample_weight=None, max_fpr=None, multi_class="raise", labels=None, device=None):
    """The area under the ROC curve with ties, ``U2 / (2 P N)``; one class in ``y_true``: a warning and NaN, as scikit-learn 1.7."""
    who = "metrics.roc_auc_score"
    _refuse(who, sample_weight=(sample_weight, None), max_fpr=(max_fpr, None), labels=(labels, None))
    if average not in ("macro", None, "binary"):
        raise NotImplementedError(f"{who}: average={average!r} is not supported (a binary target has one score)")
    y = _truth(y_true, who)
    s = y_score if isinstance(y_score, torch.Tensor) else np.asarray(y_score)
    if s.ndim != 1 and not (s.ndim == 2 and s.shape[1] == 1):
        raise NotImplementedError(f"{who}: multi-output or multi-class scores are not supported (y_score has shape {tuple(s.shape)})")
    if len(_classes(y, None, None, who)) != 2:
        if not isinstance(s, torch.Tensor) and not np.all(np.isfinite(s.astype(np.float64))):
            raise ValueError(f"{who}: the scores contain NaN or infinity")
        warnings.warn("Only one class is present in y_true. ROC AUC score is not defined in that case.", UndefinedMetricWarning, stacklevel=2)
        return float("nan")
    u2, pos, neg = auc_pair_counts(y, s.reshape(-1), device=device)[0, 0]
    return float(auc_from_pairs(u2, pos, neg))


def mean_squared_error(y_true, y_pred, *, sample_weight=None, multioutput="uniform_average", device=None):
    _refuse("metrics.mean_squared_error", sample_weight=(sample_weight, None), multioutput=(multioutput, "uniform_average"))
    return float(regression_scores(y_true, _one_column(y_pred, "metrics.mean_squared_error"), device=device)["MSE"][0, 0])


def r2_score(y_true, y_pred, *, sample_weight=None, multioutput="uniform_average", force_finite=True, device=None):
    _refuse("metrics.r2_score", sample_weight=(sample_weight, None), multioutput=(multioutput, "uniform_average"), force_finite=(force_finite, True))
    r2 = float(regression_scores(y_true, _one_column(y_pred, "metrics.r2_score"), device=device)["R2"][0, 0])
    if np.isnan(r2):
        warnings.warn("R^2 score is not well-defined with less than two samples.", UndefinedMetricWarning, stacklevel=2)
    return r2


def _one_column(y_pred, who):
    a = y_pred if isinstance(y_pred, torch.Tensor) else np.asarray(y_pred)
    if a.ndim != 1 and not (a.ndim == 2 and a.shape[1] == 1):
        raise NotImplementedError(f"{who}: multi-output targets are not supported (y_pred has shape {tuple(a.shape)})")
    return a.reshape(-1)


# ---- the reference's results table ---------------------------------------------------------------------------------------------------------
def evaluate_models(models, X_test, y_test, names=None):
    """``{name: {the eight keys: float}}`` for a dict or a list of fitted models: the reference's ``evaluate_model`` per model, with the
    scores of all models counted by two batched device calls' worth of launches (confusion counts, pair counts) and one host read.
    Every model's ``predict`` is called, and ``predict_proba(X_test)[:, 1]`` where it has one; a model without it contributes its hard
    predictions as scores.  The positive class is 1, as in the reference.  No plotting."""
    who = "metrics.evaluate_models"
    if isinstance(models, dict):
        if names is not None:
            raise ValueError(f"{who}: names are the keys of a dict of models")
        names, models = list(models), list(models.values())
    else:
        models = list(models)
        names = [f"{type(m).__name__}_{k}" for k, m in enumerate(models)] if names is None else list(names)
    if not models or len(names) != len(models) or len(set(names)) != len(names):
        raise ValueError(f"{who}: one distinct name per model and one model at least are needed")
    y = _truth(y_test, who)
    dev = _check_device(None, X_test, who=who)
    preds, scores = [], []
    for m in models:
        p = m.predict(X_test)
        p = p.to(dev) if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(_to_numpy(p))).to(dev)
        preds.append(p.reshape(-1))
        if hasattr(m, "predict_proba"):
            s = m.predict_proba(X_test)
            s = s if isinstance(s, torch.Tensor) else torch.from_numpy(np.asarray(s, dtype=np.float64))
            scores.append(s.to(dev)[:, 1].to(torch.float64))
        else:
            scores.append(preds[-1].to(torch.float64))
    got = classification_scores(y, torch.stack(preds), torch.stack(scores), pos_label=1, device=dev)
    return {name: {k: float(got[k][i, 0]) for k in KEYS} for i, name in enumerate(names)}
