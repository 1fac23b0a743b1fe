"""``bbbp_amd.cat`` restated in numpy: CatBoost's Plain boosting of symmetric trees for RMSE with no sum that has an order.

The module docstring of ``bbbp_amd/cat.py`` states the algorithm; this file is the same algorithm once more, written for reading, and the
GPU fit must equal it bit for bit (``tests/test_gpu_cat.py``).  Nothing here imports the package; the quantisation is ``tests/xgb_numpy.py``'s.

* ``border``: the float32 number that the predict kernel's ``x > border`` needs so that it agrees with ``bin(x) > c`` on the training column.
* ``quantise_gradients`` / ``to_S`` / ``terms``: a part's exact integer sum and what a side adds to a candidate's ``num`` and ``den``.
* ``scores``: every candidate's score over the parts in order; ``fit``: the boosted trees; ``predict``: ``obl_sum_kernel``'s order.

Float64 throughout, every operation rounded on its own (numpy never fuses).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xgb_numpy as xn  # noqa: E402

MAX_ROWS = 8192


def border(col, cut):
    """``a`` is the largest value of the float32 column below ``cut``: the midpoint ``float32(0.5 (a + cut))`` formed in float64, or ``a``
    when the midpoint rounds up to ``cut`` (adjacent floats)."""
    col = np.asarray(col, np.float32)
    cut = np.float32(cut)
    a = col[col < cut].max() + np.float32(0)                           # -0.0 + 0.0 = +0.0: which of two equal zeros a maximum keeps is not defined
    mid = np.float32(0.5 * (np.float64(a) + np.float64(cut)))
    return a if mid >= cut else mid


def quantise_gradients(g):
    """(k, q): ``k = 47 - ilogb(max |g|)`` (0 when every g is 0) and ``q_i = rint(g_i 2^k)`` as int64: one rounding of g to a grid."""
    gmax = np.float64(np.max(np.abs(g)))
    if gmax == 0:
        return 0, np.zeros(len(g), np.int64)
    k = 47 - (int(np.frexp(gmax)[1]) - 1)
    return k, np.rint(np.ldexp(g, k)).astype(np.int64)


def to_S(Q, k):
    """A part's gradient sum from its integer sum: one rounding (int64 -> float64), then an exact scaling."""
    return np.ldexp(np.asarray(Q, np.int64).astype(np.float64), -k)


def terms(Q, m, k, lam):
    """What a side of ``m > 0`` rows adds: ``alpha S`` to num and ``(alpha alpha) m`` to den, ``alpha = S / (m + lambda)``."""
    S = to_S(Q, k)
    alpha = S / (np.asarray(m, np.float64) + lam)
    return alpha * S, (alpha * alpha) * np.asarray(m, np.float64)


def scores(right, q, parts, k, lam):
    """float64 [K]: the score of every candidate.  ``right`` [K, n] says which rows a candidate sends right, ``parts`` are the level's row
    sets in the order of the leaf index read with level 0 as the most significant bit.  In a part left then right; an empty side is skipped."""
    K = right.shape[0]
    num, den = np.zeros(K), np.zeros(K)
    for rows in parts:
        m, Q = len(rows), int(q[rows].sum())
        r = right[:, rows]
        m_r = r.sum(axis=1)
        Q_r = (r * q[rows][None, :]).sum(axis=1)                      # exact: int64
        for Q_s, m_s in ((Q - Q_r, m - m_r), (Q_r, m_r)):
            has = m_s > 0
            a, b = terms(Q_s, np.where(has, m_s, 1), k, lam)
            num = np.where(has, num + a, num)
            den = np.where(has, den + b, den)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (num * num) / den, 0.0)


def fit(X, y, iterations=1000, learning_rate=0.03, depth=6, l2_leaf_reg=3.0, border_count=254):
    """The boosted trees flattened as ``boosters.CatBoostTrees`` holds them (``split_feature``, ``split_border``, ``tree_first_split``,
    ``tree_first_leaf``, ``leaf_values``) with ``leaf_weights``, ``split_bin`` (the cut's index in its feature), ``bias`` and
    ``train_approx``."""
    X = np.asarray(X, np.float32)
    y = np.asarray(y, np.float64)
    n = X.shape[0]
    assert 2 <= n <= MAX_ROWS and 1 <= border_count <= 255 and 1 <= depth <= 16
    live, cc, B = xn.quantise(X, border_count + 1)
    if not len(live):
        raise ValueError("all features are constant")
    lam, eta = np.float64(l2_leaf_reg), np.float64(learning_rate)
    cand_f = np.concatenate([np.full(len(c), j) for j, c in enumerate(cc)])           # (live feature, cut) in the tie rule's order
    cand_c = np.concatenate([np.arange(len(c)) for c in cc])
    right = B[cand_f].astype(np.int64) > cand_c[:, None]              # [K, n]
    bias = np.float64(np.mean(y))
    s = np.zeros(n)
    sf, sb, sbin, first_split, first_leaf, values, weights = [], [], [], [0], [0], [], []
    for _ in range(iterations):
        approx = s + bias
        k, q = quantise_gradients(y - approx)
        parts, leaves = [np.arange(n)], [0]
        used = np.zeros(len(cand_f), bool)
        levels = 0
        for level in range(depth):
            if used.all():
                break                                                # no unused candidate is left: a shallower tree
            sc = np.where(used, -1.0, scores(right, q, parts, k, lam))
            best = int(np.argmax(sc))                                 # the first maximum: the lowest feature, then the lowest cut
            used[best] = True
            f, c = int(cand_f[best]), int(cand_c[best])
            sf.append(int(live[f])); sbin.append(c); sb.append(border(X[:, live[f]], cc[f][c]))
            new_parts, new_leaves = [], []
            for rows, leaf in zip(parts, leaves):                     # stably: a part's left rows, then its right rows
                go_right = right[best, rows]
                for side, lf in ((rows[~go_right], leaf), (rows[go_right], leaf | (1 << level))):
                    if len(side):
                        new_parts.append(side); new_leaves.append(lf)
            parts, leaves = new_parts, new_leaves
            levels += 1
        v, w = np.zeros(1 << levels), np.zeros(1 << levels, np.int32)  # an empty leaf is 0.0
        leaf_of = np.zeros(n, np.int64)
        for rows, leaf in zip(parts, leaves):
            v[leaf] = eta * (to_S(int(q[rows].sum()), k) / (np.float64(len(rows)) + lam))
            w[leaf] = len(rows)
            leaf_of[rows] = leaf
        s = s + v[leaf_of]
        values.append(v); weights.append(w)
        first_split.append(len(sf)); first_leaf.append(first_leaf[-1] + len(v))
    return dict(split_feature=np.asarray(sf, np.int32), split_border=np.asarray(sb, np.float32), split_bin=np.asarray(sbin, np.int32),
                tree_first_split=np.asarray(first_split, np.int32), tree_first_leaf=np.asarray(first_leaf[:-1], np.int64),
                leaf_values=np.concatenate(values), leaf_weights=np.concatenate(weights), bias=bias, train_approx=s + bias, n_features=X.shape[1])


def predict(model, X):
    """CatBoost's rule (bit i of the leaf index is ``x[feature] > border`` of split i), summed as ``obl_sum_kernel`` sums: the leaf values
    in tree order from 0.0, times the scale 1, plus the bias."""
    X = np.asarray(X, np.float32)
    s = np.zeros(X.shape[0])
    fs, fl = model["tree_first_split"], model["tree_first_leaf"]
    for t in range(len(fs) - 1):
        idx = np.zeros(X.shape[0], np.int64)
        for i, j in enumerate(range(fs[t], fs[t + 1])):
            idx |= (X[:, model["split_feature"][j]] > model["split_border"][j]).astype(np.int64) << i
        s = s + model["leaf_values"][fl[t] + idx]
    return 1.0 * s + model["bias"]
