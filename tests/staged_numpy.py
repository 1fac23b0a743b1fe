"""numpy restatement of the staged prediction of both boosted families (``bbbp_gbt_staged_predict`` / ``bbbp_oblivious_staged_predict``,
``boosters.*.staged_predict_device``) and of the RMSE curve built on it, for comparison bit for bit.

A tree's leaf per row comes from the walk rules restated (XGBoost: NaN takes the default child, otherwise left when ``x[feature] <
cond`` in float32; CatBoost: bit i of the leaf index is ``x[feature] > border`` of level i, a NaN gives ``nan_true[feature]``).  The running
sum over trees is ``np.cumsum`` along the tree axis, which adds one row after the other in the array's own precision, started from a row
of zeros as the kernels start from 0 (``0 + -0.0`` is ``+0.0``: the sign can reach the output through ``scale * s``).  Stage k is the
running sum after the trees ``[start, ends[k])``, then ``float32(base_score) + s`` in float32, or ``scale * s`` and ``+ bias`` as two
float64 roundings (numpy forms no fused multiply-add).

``random_gbt`` / ``random_oblivious`` build seeded models that hold every tree shape the kernels treat differently: random binary trees
of depth up to 6, a chain of depth 40, a single leaf; oblivious trees of depth 0, 1 and 6."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_numpy as mn  # noqa: E402

from bbbp_amd import metrics  # noqa: E402

GBT_KEYS = ("left", "right", "feature", "cond", "default_left", "root")
OBL_KEYS = ("split_feature", "split_border", "nan_true", "tree_first_split", "tree_first_leaf", "leaf_values")


# ---- the walks ------------------------------------------------------------------------------------------------------------------------------
def gbt_leaves(m, X):
    """float32 [T, n]: the leaf value of every (tree, row)."""
    X = np.asarray(X, np.float32)
    n, rows = X.shape[0], np.arange(X.shape[0])
    left, right, feature, cond, dleft, root = (np.asarray(m[k]) for k in GBT_KEYS)
    out = np.empty((len(root) - 1, n), np.float32)
    for t in range(len(root) - 1):
        node = np.full(n, root[t], np.int64)
        while True:
            inner = left[node] >= 0
            if not inner.any():
                break
            v = X[rows, np.where(inner, feature[node], 0)]
            go_left = np.where(np.isnan(v), dleft[node] != 0, v < cond[node])
            node = np.where(inner, np.where(go_left, left[node], right[node]), node)
        out[t] = cond[node]
    return out


def oblivious_leaves(m, X):
    """float64 [T, n]: the leaf value of every (tree, row)."""
    X = np.asarray(X, np.float32)
    sf, sb, nan_true, fs, fl, values = (np.asarray(m[k]) for k in OBL_KEYS)
    out = np.empty((len(fs) - 1, X.shape[0]), np.float64)
    for t in range(len(fs) - 1):
        idx = np.zeros(X.shape[0], np.int64)
        for level, s in enumerate(range(fs[t], fs[t + 1])):
            v = X[:, sf[s]]
            idx |= np.where(np.isnan(v), nan_true[sf[s]] != 0, v > sb[s]).astype(np.int64) << level
        out[t] = values[fl[t] + idx]
    return out


def _running(leaves, ends, start):
    """The running sums after the trees [start, e) for e in ``ends``, in the precision of ``leaves``, started from zero."""
    ends = np.asarray(ends, np.int64)
    part = leaves[start:int(ends[-1])]
    s = np.cumsum(np.concatenate([np.zeros((1, part.shape[1]), part.dtype), part]), axis=0, dtype=part.dtype)
    return s[ends - start]


def staged_gbt(m, X, ends, start=0, leaves=None):
    """float32 [K, n]: ``base_score + s_k`` with ``s`` summed in float32 in tree order from ``start``."""
    leaves = gbt_leaves(m, X) if leaves is None else leaves
    return (np.float32(m["base_score"]) + _running(leaves, ends, start)).astype(np.float32)


def staged_oblivious(m, X, ends, start=0, leaves=None):
    """float64 [K, n]: ``scale * s_k``, then ``+ bias``: two roundings."""
    leaves = oblivious_leaves(m, X) if leaves is None else leaves
    prod = np.float64(m["scale"]) * _running(leaves, ends, start)
    return prod + np.float64(m["bias"])


def rmse_curve(staged, y):
    """One RMSE per row of ``staged`` [K, n] against ``y``: the squared-error sums in ``csrc/metrics.hip``'s order, the package's own
    division, a float64 square root.  Python floats."""
    mse = metrics.regression_from_sums(*mn.squared_error_sums(np.asarray(y, np.float64), staged))["MSE"][:, 0]
    return [float(v) for v in np.sqrt(mse)]


def bits(a):
    """An array's bytes as unsigned integers of its item size, for ``==`` on the bits."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def triples(T):
    """Every (tree_start, tree_end, period) the tests run on a model of ``T`` trees: starts 0, 1 and T - 1, ends at the model's end, one
    tree and three trees behind the start, periods 1, 2, 3, T and T + 5."""
    out = []
    for start in sorted({s for s in (0, 1, T - 1) if 0 <= s < T}):
        for end in sorted({e for e in (T, start + 1, start + 3) if start < e <= T}):
            out += [(start, end, period) for period in sorted({1, 2, 3, T, T + 5})]
    return out


def queries(n, d, seed):
    """float32 [n, d]: values on a grid of tenths (ties with the thresholds, which lie on the same grid), about a tenth of them NaN."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, d)), 1).astype(np.float32)
    X[rng.random((n, d)) < 0.1] = np.nan
    return X


def random_gbt(T, d, seed):
    """A seeded gbtree model of ``T`` trees over ``d`` features as a dict of ``boosters.XGBTrees``' arrays with ``n_features`` and
    ``base_score``: tree 1 is a chain of depth 40, tree 2 a single leaf, the others random binary trees of depth up to 6 whose root
    splits; ``default_left`` is drawn per node."""
    rng = np.random.default_rng(seed)
    left, right, feature, cond, dleft, root = [], [], [], [], [], [0]

    def node(is_leaf):
        left.append(-1); right.append(-1)
        feature.append(0 if is_leaf else int(rng.integers(d)))
        cond.append(np.float32(rng.normal()) if is_leaf else np.float32(np.round(rng.normal(), 1)))
        dleft.append(0 if is_leaf else int(rng.integers(2)))
        return len(left) - 1

    def grow(depth, max_depth):
        is_leaf = depth == max_depth or (depth > 0 and rng.random() < 0.3)
        me = node(is_leaf)
        if not is_leaf:
            left[me] = grow(depth + 1, max_depth)
            right[me] = grow(depth + 1, max_depth)
        return me

    for t in range(T):
        if t == 1:                                                    # a chain: every inner node has one leaf child, on a drawn side
            me = node(False)
            for _ in range(39):
                leaf, nxt = node(True), node(False)
                left[me], right[me] = (leaf, nxt) if rng.random() < 0.5 else (nxt, leaf)
                me = nxt
            left[me], right[me] = node(True), node(True)
        elif t == 2:
            node(True)
        else:
            grow(0, int(rng.integers(1, 7)) if t else 6)
        root.append(len(left))
    return dict(left=np.asarray(left, np.int32), right=np.asarray(right, np.int32), feature=np.asarray(feature, np.int32),
                cond=np.asarray(cond, np.float32), default_left=np.asarray(dleft, np.uint8), root=np.asarray(root, np.int32), n_features=d,
                base_score=np.float32(0.37))


def random_oblivious(T, d, seed):
    """A seeded model of ``T`` oblivious trees over ``d`` features as a dict of ``boosters.CatBoostTrees``' arrays with ``n_features``,
    ``scale`` and ``bias``: tree 0 has depth 6, tree 1 depth 0, tree 2 depth 1, the others a drawn depth in 0..6; every third feature
    treats NaN as true."""
    rng = np.random.default_rng(seed)
    depths = [6 if t == 0 else 0 if t == 1 else 1 if t == 2 else int(rng.integers(0, 7)) for t in range(T)]
    fs = np.concatenate([[0], np.cumsum(depths)])
    sizes = 1 << np.asarray(depths, np.int64)
    return dict(split_feature=rng.integers(d, size=fs[-1]).astype(np.int32), split_border=np.round(rng.normal(size=fs[-1]), 1).astype(np.float32),
                nan_true=(np.arange(d) % 3 == 1).astype(np.uint8), tree_first_split=fs.astype(np.int32),
                tree_first_leaf=np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), leaf_values=rng.normal(size=int(sizes.sum())),
                n_features=d, scale=1.7, bias=0.3)


def xgb_trees(m, device):
    from bbbp_amd import boosters
    return boosters.XGBTrees(*(m[k] for k in GBT_KEYS), m["n_features"], m["base_score"], device=device)


def cat_trees(m, device):
    from bbbp_amd import boosters
    return boosters.CatBoostTrees(*(m[k] for k in OBL_KEYS), m["n_features"], m["scale"], m["bias"], device=device)


def of_xgb(trees, base_score, n_features):
    """The oracle's model dict from a regressor's ``trees_`` (or ``xgb_numpy.fit``'s result)."""
    return dict({k: np.asarray(trees[k]) for k in GBT_KEYS}, n_features=int(n_features), base_score=np.float32(base_score))


def of_cat(trees, bias, n_features):
    """The oracle's model dict from a regressor's ``trees_`` (or ``cat_numpy.fit``'s result): no NaN treatment, scale 1."""
    return dict({k: np.asarray(trees[k]) for k in OBL_KEYS if k != "nan_true"}, nan_true=np.zeros(int(n_features), np.uint8),
                n_features=int(n_features), scale=1.0, bias=float(bias))


def fitted_problem(seed=6, n=200, d=12, held_out=80):
    """(X_train, y_train, X_test, y_test) for the fitted-model tests: one weak column under unit noise, so that a booster of 20 small trees
    at learning rate 0.1 has the signal after some ten trees and fits noise from there on: the held-out curve turns inside the run.  That
    depends on the seed; the tests that rely on it check it on the numpy-fitted model first."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n + held_out, d)), 2).astype(np.float32)
    y = 0.4 * X[:, 0] + rng.normal(size=n + held_out)
    return X[:n], y[:n], X[n:], y[n:]
