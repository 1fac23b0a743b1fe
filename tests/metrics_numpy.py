"""numpy restatement of ``bbbp_amd.metrics``' device side: confusion counts by boolean masks, the AUC pair count ``U2`` by two
``searchsorted`` calls per segment, and the squared-error sums in the kernel's fixed order (a lane-strided sequential sum over 256 lanes,
the shuffle tree ``v[l] += v[l + off]`` for off = 32 .. 1 per wave of 64, then the four waves in ascending order), every product,
difference and sum rounded once.  The sums are finished with the package's own host expressions (``scores_from_counts``,
``auc_from_pairs``, ``regression_from_sums``), so a GPU result can be compared bit for bit."""
from fractions import Fraction

import numpy as np

from bbbp_amd import metrics

LANES, WAVE = 256, 64


def segments(groups, n):
    """(segment id per row, G) with every row in segment 0 for ``None``."""
    if groups is None:
        return np.zeros(n, dtype=np.int64), 1
    g = np.asarray(groups).astype(np.int64)
    return g, max(int(g.max()) + 1, 1)


def confusion_counts(y01, pred01, groups=None):
    """int64 [M, G, 4] of (tn, fp, fn, tp)."""
    y01, pred01 = np.asarray(y01).astype(bool), np.atleast_2d(np.asarray(pred01)).astype(bool)
    seg, G = segments(groups, len(y01))
    out = np.zeros((len(pred01), G, 4), dtype=np.int64)
    for m, p in enumerate(pred01):
        for g in range(G):
            s = seg == g
            out[m, g] = [np.count_nonzero(s & ~y01 & ~p), np.count_nonzero(s & ~y01 & p), np.count_nonzero(s & y01 & ~p), np.count_nonzero(s & y01 & p)]
    return out


def pair_counts(y01, scores, groups=None):
    """int64 [M, G, 3] of (U2, P, N): U2 = sum over positives of #{negatives < s} + #{negatives <= s}, float comparisons."""
    y01, scores = np.asarray(y01).astype(bool), np.atleast_2d(np.asarray(scores)).astype(np.float64)
    seg, G = segments(groups, len(y01))
    out = np.zeros((len(scores), G, 3), dtype=np.int64)
    for m, s in enumerate(scores):
        for g in range(G):
            neg, pos = np.sort(s[(seg == g) & ~y01]), s[(seg == g) & y01]
            u2 = int(np.searchsorted(neg, pos, side="left").sum()) + int(np.searchsorted(neg, pos, side="right").sum())
            out[m, g] = [u2, len(pos), len(neg)]
    return out


def _fused(acc, d):
    """acc + d * d rounded once: what a fused multiply-add would give."""
    return float(Fraction(float(acc)) + Fraction(float(d)) * Fraction(float(d)))


def fixed_order_sum(terms, include, square=False, fused=False):
    """The work-group's sum of ``terms`` (or of their squares) over the rows of ``include``, in the kernel's order."""
    terms, include = np.asarray(terms, dtype=np.float64), np.asarray(include, dtype=bool)
    acc = np.zeros(LANES, dtype=np.float64)
    for start in range(0, len(terms), LANES):
        t, inc = terms[start:start + LANES], include[start:start + LANES]
        k = len(t)
        if fused:
            acc[:k] = [_fused(a, d) if i else a for a, d, i in zip(acc[:k], t, inc)]
        else:
            acc[:k] = np.where(inc, acc[:k] + (t * t if square else t), acc[:k])
    v = acc.reshape(LANES // WAVE, WAVE).copy()
    off = WAVE // 2
    while off:
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
        off //= 2
    total = v[0, 0]
    for w in range(1, LANES // WAVE):
        total = total + v[w, 0]
    return total


def squared_error_sums(y, pred, groups=None, fused=False):
    """(sse [M, G], ystat [G, 3] = (sum y, sum (y - ybar)^2, count)) as the kernel forms them; float32 predictions widen exactly."""
    y, pred = np.asarray(y, dtype=np.float64), np.atleast_2d(np.asarray(pred)).astype(np.float64)
    seg, G = segments(groups, len(y))
    sse, ystat = np.zeros((len(pred), G)), np.zeros((G, 3))
    for g in range(G):
        inc = seg == g
        total, count = fixed_order_sum(y, inc), float(np.count_nonzero(inc))
        mean = total / count if count else 0.0
        ystat[g] = [total, fixed_order_sum(y - mean, inc, square=True, fused=fused), count]
        for m, p in enumerate(pred):
            sse[m, g] = fixed_order_sum(y - p, inc, square=True, fused=fused)
    return sse, ystat


def classification_scores(y01, pred01, scores=None, groups=None, zero_division="warn"):
    """The eight scores [M, G] for 0/1 truth and predictions (positive = 1) and scores of class 1 (``None``: the hard predictions)."""
    out = metrics.scores_from_counts(confusion_counts(y01, pred01, groups), zero_division)
    pairs = pair_counts(y01, np.atleast_2d(np.asarray(pred01)).astype(np.float64) if scores is None else scores, groups)
    out["ROC AUC"] = metrics.auc_from_pairs(pairs[..., 0], pairs[..., 1], pairs[..., 2])
    return out


def regression_scores(y, pred, groups=None):
    return metrics.regression_from_sums(*squared_error_sums(y, pred, groups))


def bits(a):
    """A float64 array's bytes as int64, for ``==`` on the bits (NaN payloads included)."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def problem(n, M, G=1, seed=0, ties=0.0, dtype=np.float64, left_out=False, one_class=False):
    """(y01 [n], pred01 [M, n] uint8, scores [M, n], groups or None): a seeded two-class problem.  ``ties``: the share of scores drawn
    from four values only.  With G = 3 segment 1 is empty and segment 2 holds one class only (where n allows); ``left_out`` puts every
    seventh row at -1."""
    rs = np.random.RandomState(seed + 1000 * n + 10 * M + G)
    y = (rs.rand(n) < 0.4).astype(np.uint8)
    if one_class:
        y[:] = 1
    scores = rs.rand(M, n) * 0.6 + 0.4 * y * rs.rand(M, n)
    if ties:
        coarse = rs.choice([0.0, 0.25, 0.5, 1.0], size=(M, n))
        scores = np.where(rs.rand(M, n) < ties, coarse, scores)
    scores = scores.astype(dtype)
    pred = (scores > 0.5).astype(np.uint8)
    groups = None
    if G > 1:
        groups = rs.choice([0, G - 1], size=n)
        y[groups == G - 1] = 1 if not one_class else y[0]
        if left_out:
            groups[::7] = -1
    return y, pred, scores, groups
