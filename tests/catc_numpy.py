"""``bbbp_amd.cat.CatBoostClassifier`` restated in numpy: CatBoost's Plain boosting of symmetric trees for Logloss with a Bayesian
bootstrap, with no sum that has an order.

The module docstring of ``bbbp_amd/cat.py`` states the algorithm; this file is the same algorithm once more, written from that text for
reading, and the GPU fit must equal it bit for bit (``tests/test_gpu_catc.py``).  Nothing here imports the package.  The quantisation is
``tests/xgb_numpy.py``'s, the border rule and the prediction order are ``tests/cat_numpy.py``'s (the regressor's, unchanged); the sigmoid,
the hash, the weight draw, the score over weighted sums and the Newton leaves are this file's own.

* ``sigmoid64``: IEEE operations only, so the device gives the same bits.
* ``mix`` / ``draw`` / ``bootstrap_weights``: the counter-based hash and a tree's fixed-point weights.
* ``quantise``: a tree's ``k``, ``q`` and ``r``; ``terms``: what a side adds to ``num`` and ``den``; ``scores``: every candidate's score.
* ``fit``: the boosted trees; ``predict`` / ``predict_proba``.

Float64 throughout, every operation rounded on its own (numpy never fuses).  The bounds that make the integer sums exact are asserted
with Python ints, which cannot overflow.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_numpy as cn  # noqa: E402
import xgb_numpy as xn  # noqa: E402

MAX_ROWS = 8192
Q_BITS, H_BITS, W_BITS = 27, 48, 16
WEIGHT_STREAM = 2                                                     # the bootstrap's stream tag; xgb's row and column draws hold 0 and 1
LN2_HI, LN2_LO, INV_LN2 = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33"), float.fromhex("0x1.71547652b82fep+0")
FACTORIALS = [1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0, 39916800.0, 479001600.0, 6227020800.0]


def sigmoid64(x):
    """``exp(-|z|)`` by the reduction ``a = k ln2 + r`` (``|r| <= ln2 / 2``) and the Taylor polynomial of degree 13 in ``r`` by Horner's
    rule, then ``1 / (1 + e)`` for ``z >= 0`` and ``e / (1 + e)`` otherwise.  The clamp at -700 keeps the result a normal float64."""
    z = np.asarray(x, np.float64)
    a = np.maximum(-np.abs(z), -700.0)
    k = np.rint(a * INV_LN2)
    r = (a - k * LN2_HI) - k * LN2_LO
    P = np.full_like(r, 1.0 / FACTORIALS[13])
    for j in range(12, -1, -1):
        P = P * r + 1.0 / FACTORIALS[j]
    e = np.ldexp(P, k.astype(np.int32))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def mix(x):
    """The splitmix64 finaliser on uint64 arrays (which wrap modulo 2^64)."""
    x = np.array(x, dtype=np.uint64, ndmin=1)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draw(seed, stream, tree, i):
    """uint64: ``mix(mix(mix(seed + golden (stream + 1)) + tree) + i)``, broadcast over ``i``."""
    s = np.array([(int(seed) + 0x9E3779B97F4A7C15 * (int(stream) + 1)) % 2 ** 64], np.uint64)
    return mix(mix(mix(s) + np.uint64(tree)) + np.asarray(i, np.uint64))


def bootstrap_weights(seed, tree, n, temperature):
    """uint32 [n]: tree ``tree``'s Bayesian-bootstrap weights in fixed point with 16 fraction bits.  ``u = ((hash >> 11) + 1) 2^-53`` lies in
    (0, 1], ``w = (-log u) ** temperature`` and ``w_i = max(1, rint(w 2^16))``.  The draw depends on (seed, tree, position) only."""
    assert 0.0 <= temperature <= 1.0
    u = ((draw(seed, WEIGHT_STREAM, tree, np.arange(n)) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    assert u.min() > 0.0 and u.max() <= 1.0
    w = np.power(-np.log(u), np.float64(temperature))
    wi = np.maximum(1, np.rint(w * 2.0 ** W_BITS).astype(np.int64))
    assert int(wi.min()) >= 1 and int(wi.max()) <= 2407583 < 2 ** 22
    return wi.astype(np.uint32)


def quantise(t, approx):
    """(k, q, r) of a tree: ``g = t - p``, ``h = p (1 - p)``, ``k = 27 - ilogb(max |g|)`` (0 when every g is 0), ``q = rint(g 2^k)`` and
    ``r = max(1, rint(h 2^48))`` as int64."""
    p = sigmoid64(approx)
    g, h = t - p, p * (1.0 - p)
    gmax = np.float64(np.max(np.abs(g)))
    k = 0 if gmax == 0 else Q_BITS - (int(np.frexp(gmax)[1]) - 1)
    q = np.rint(np.ldexp(g, k)).astype(np.int64)
    r = np.maximum(1, np.rint(np.ldexp(h, H_BITS)).astype(np.int64))
    assert max(abs(int(q.min())), abs(int(q.max()))) <= 2 ** 28 and 1 <= int(r.min()) and int(r.max()) <= 2 ** 46
    return k, q, r


def exact_sum(values):
    """The sum as a Python int: no order, no overflow."""
    return sum(int(x) for x in values)


def terms(QW, MW, k, lam):
    """What a side that holds a row adds: ``alpha S`` to num and ``(alpha alpha) M`` to den, with ``S = QW 2^-(k + 16)``, ``M = MW 2^-16``
    (one rounding each, then an exact scaling) and ``alpha = S / (M + lambda)``."""
    S = np.ldexp(np.asarray(QW, np.int64).astype(np.float64), -(k + W_BITS))
    M = np.ldexp(np.asarray(MW, np.int64).astype(np.float64), -W_BITS)
    alpha = S / (M + lam)
    return alpha * S, (alpha * alpha) * M


def scores(right, qw, w, parts, k, lam):
    """float64 [K]: the score of every candidate.  ``right`` [K, n] says which rows a candidate sends right, ``parts`` are the level's row
    sets in the order of the leaf index read with level 0 as the most significant bit.  In a part left then right; a side without a row
    is skipped."""
    K = right.shape[0]
    num, den = np.zeros(K), np.zeros(K)
    for rows in parts:
        QW, MW = exact_sum(qw[rows]), exact_sum(w[rows])
        assert abs(QW) < 2 ** 63 and 0 < MW < 2 ** 35                 # |qw| < 2^50, w < 2^22, n <= 2^13: int64 sums are exact in any order
        r = right[:, rows]
        m_r = r.sum(axis=1)
        QW_r = (r * qw[rows][None, :]).sum(axis=1)                    # exact: int64
        MW_r = (r * w[rows][None, :]).sum(axis=1)
        for QW_s, MW_s, m_s in ((QW - QW_r, MW - MW_r, len(rows) - m_r), (QW_r, MW_r, m_r)):
            has = m_s > 0
            assert np.array_equal(has, MW_s > 0)                      # w >= 1: a side is empty iff its weight sum is 0
            a, b = terms(QW_s, np.where(has, MW_s, 1), k, lam)
            num = np.where(has, num + a, num)
            den = np.where(has, den + b, den)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (num * num) / den, 0.0)


def fit(X, t, iterations=1000, learning_rate=0.03, depth=6, l2_leaf_reg=3.0, border_count=254, bagging_temperature=None, random_seed=0,
        boost_from_average=True):
    """The boosted trees flattened as ``boosters.CatBoostTrees`` holds them (``split_feature``, ``split_border``, ``tree_first_split``,
    ``tree_first_leaf``, ``leaf_values``) with ``leaf_weights``, ``split_bin``, ``bias`` and ``train_approx``.  ``t`` holds 0 / 1;
    ``bagging_temperature=None`` is no bootstrap: every weight is 2^16."""
    X = np.asarray(X, np.float32)
    t = np.asarray(t, np.float64)
    n = X.shape[0]
    assert 2 <= n <= MAX_ROWS and 1 <= border_count <= 255 and 1 <= depth <= 16 and set(np.unique(t)) == {0.0, 1.0}
    live, cc, B = xn.quantise(X, border_count + 1)
    if not len(live):
        raise ValueError("all features are constant")
    lam, eta = np.float64(l2_leaf_reg), np.float64(learning_rate)
    cand_f = np.concatenate([np.full(len(c), j) for j, c in enumerate(cc)])           # (live feature, cut) in the tie rule's order
    cand_c = np.concatenate([np.arange(len(c)) for c in cc])
    right = B[cand_f].astype(np.int64) > cand_c[:, None]              # [K, n]
    P, N = int((t == 1).sum()), int((t == 0).sum())
    bias = np.log(np.float64(P) / np.float64(N)) if boost_from_average else np.float64(0.0)
    s = np.zeros(n)
    sf, sb, sbin, first_split, first_leaf, values, weights = [], [], [], [0], [0], [], []
    for tree in range(iterations):
        approx = s + bias
        k, q, r = quantise(t, approx)
        w = np.full(n, 1 << W_BITS, np.int64) if bagging_temperature is None else \
            bootstrap_weights(random_seed, tree, n, bagging_temperature).astype(np.int64)
        qw = q * w
        assert all(abs(int(a) * int(b)) < 2 ** 50 for a, b in zip(q, w)) and np.array_equal(qw, [int(a) * int(b) for a, b in zip(q, w)])
        parts, leaves = [np.arange(n)], [0]
        used = np.zeros(len(cand_f), bool)
        levels = 0
        for level in range(depth):
            if used.all():
                break                                                # no unused candidate is left: a shallower tree
            sc = np.where(used, -1.0, scores(right, qw, w, parts, k, lam))
            best = int(np.argmax(sc))                                 # the first maximum: the lowest feature, then the lowest cut
            used[best] = True
            f, c = int(cand_f[best]), int(cand_c[best])
            sf.append(int(live[f])); sbin.append(c); sb.append(cn.border(X[:, live[f]], cc[f][c]))
            new_parts, new_leaves = [], []
            for rows, leaf in zip(parts, leaves):                     # stably: a part's left rows, then its right rows
                go_right = right[best, rows]
                for side, lf in ((rows[~go_right], leaf), (rows[go_right], leaf | (1 << level))):
                    if len(side):
                        new_parts.append(side); new_leaves.append(lf)
            parts, leaves = new_parts, new_leaves
            levels += 1
        v, lw = np.zeros(1 << levels), np.zeros(1 << levels, np.int32)  # an empty leaf is 0.0
        leaf_of = np.zeros(n, np.int64)
        for rows, leaf in zip(parts, leaves):                         # one Newton step over all rows of the leaf, unweighted
            Qg, R = exact_sum(q[rows]), exact_sum(r[rows])
            assert abs(Qg) <= 2 ** 41 and 0 < R <= 2 ** 59
            G, H = np.ldexp(np.float64(Qg), -k), np.ldexp(np.float64(R), -H_BITS)
            v[leaf] = eta * (G / (H + lam))
            lw[leaf] = len(rows)
            leaf_of[rows] = leaf
        s = s + v[leaf_of]
        values.append(v); weights.append(lw)
        first_split.append(len(sf)); first_leaf.append(first_leaf[-1] + len(v))
    return dict(split_feature=np.asarray(sf, np.int32), split_border=np.asarray(sb, np.float32), split_bin=np.asarray(sbin, np.int32),
                tree_first_split=np.asarray(first_split, np.int32), tree_first_leaf=np.asarray(first_leaf[:-1], np.int64),
                leaf_values=np.concatenate(values), leaf_weights=np.concatenate(weights), bias=np.float64(bias), train_approx=s + bias,
                n_features=X.shape[1])


def predict(model, X):
    """The raw values: ``cat_numpy.predict``'s order, the leaf values in tree order from 0.0, then the bias."""
    return cn.predict(model, X)


def predict_proba(model, X):
    """float64 [m, 2]: ``(1 - p1, p1)`` with ``p1 = sigmoid64(raw)``."""
    p1 = sigmoid64(predict(model, X))
    return np.stack([1.0 - p1, p1], axis=1)


def predict_class(model, X):
    """bool [m]: ``raw > 0``, the index into ``classes_``."""
    return predict(model, X) > 0
