"""numpy restatement of ``random_forest``'s regression fit (csrc/rf.hip, the squared-error criterion): the quantised targets, the integer
sums, the seven-operation score, the tie rule and the level-by-level numbering.  The hash, the bootstrap and the feature draw are
``rf_numpy``'s.  Sums are exact int64 and a score is a fixed sequence of IEEE operations, so the GPU's trees equal these bit for bit.
Plain numpy, no GPU."""
import numpy as np

import rf_numpy as N

TARGET_BITS = 49


def quantise(y):
    """(q, s): q_i = rint(y_i 2^s) as int64 with |q_i| <= 2^TARGET_BITS, s = TARGET_BITS - e for (_, e) = frexp(max |y|); s = 0 when all of y
    is 0.  y_hat = ldexp(q, -s) is within 2^-50 2^e of y."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    top = float(np.abs(y).max())
    s = 0 if top == 0.0 else TARGET_BITS - int(np.frexp(top)[1])
    return np.rint(np.ldexp(y, s)).astype(np.int64), s


def dequantise(q, s):
    return np.ldexp(np.asarray(q, dtype=np.float64), -s)


def position_sums(fv, w, wq, msl):
    """Valid positions of a node in one feature's order (``fv`` float32 ascending, ``w`` / ``wq`` the rows' weights and weight x target in
    that order, int64) and the exact left sums (W_L, S_L) there."""
    m = len(fv)
    p = np.arange(1, m)
    ok = (fv[1:] > (fv[:-1] + N.FEATURE_THRESHOLD).astype(np.float32)) & (p >= msl) & (m - p >= msl)
    p = p[ok]
    return p, np.cumsum(w)[p - 1], np.cumsum(wq)[p - 1]


def scores(WL, SL, W, S):
    """S_L S_L / W_L + S_R S_R / W_R: two conversions, two products, two divisions and one add, each rounded to nearest (numpy fuses nothing)."""
    sl, sr = SL.astype(np.float64), (S - SL).astype(np.float64)
    return sl * sl / WL.astype(np.float64) + sr * sr / (W - WL).astype(np.float64)


def fit_tree(X32, q, w, key, max_depth, min_samples_split, min_samples_leaf, max_features):
    """One tree over the rows of positive weight on integer targets ``q``.  Returns tree-relative arrays (left, right, feature, threshold,
    value = S / W in units of the grid, n_node_samples, weighted_n_node_samples)."""
    depth_limit = N.UNLIMITED if max_depth is None else int(max_depth)
    left, right, feature, threshold, value, nns, wns = [-1], [-1], [0], [-2.0], [0.0], [0], [0.0]
    level = [(0, np.nonzero(w > 0)[0], key)]
    depth = 0
    while level:
        nxt = []
        for node, rows, k in level:
            m = len(rows)
            W, S = int(w[rows].sum()), int((w[rows] * q[rows]).sum())
            nns[node], value[node], wns[node] = m, np.float64(S) / np.float64(W), float(W)
            if depth >= depth_limit or m < min_samples_split or m < 2 * min_samples_leaf or q[rows].min() == q[rows].max():
                continue
            best = None                                   # (score, feature, position, a, b)
            for f in N.draw_features(k, X32[rows], max_features):
                o = np.argsort(X32[rows, f], kind="stable")
                fv = X32[rows, f][o]
                p, WL, SL = position_sums(fv, w[rows][o], (w[rows] * q[rows])[o], min_samples_leaf)
                if not len(p):
                    continue
                score = scores(WL, SL, W, S)
                j = int(np.argmax(score))                 # the lowest position among equal scores
                if best is None or score[j] > best[0]:    # the lowest feature among equal scores
                    best = (score[j], int(f), int(p[j]), fv[p[j] - 1], fv[p[j]])
            if best is None:
                continue
            _, f, p, a, b = best
            thr = N.midpoint(a, b)
            goes_left = X32[rows, f].astype(np.float64) <= thr
            lc = len(left)
            for _ in range(2):
                left.append(-1); right.append(-1); feature.append(0); threshold.append(-2.0); value.append(0.0); nns.append(0); wns.append(0.0)
            left[node], right[node], feature[node], threshold[node] = lc, lc + 1, f, float(thr)
            nxt.append((lc, rows[goes_left], N.child_key(k, 0)))
            nxt.append((lc + 1, rows[~goes_left], N.child_key(k, 1)))
        level = nxt
        depth += 1
    return (np.asarray(left, dtype=np.int32), np.asarray(right, dtype=np.int32), np.asarray(feature, dtype=np.int32),
            np.asarray(threshold, dtype=np.float64), np.asarray(value, dtype=np.float64), np.asarray(nns, dtype=np.int32),
            np.asarray(wns, dtype=np.float64))


def fit_forest(X, y, n_estimators, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=None, bootstrap=True, seed=0,
               weights=None, with_weights=False):
    """The forest's trees in the flat convention of ``trees_`` (absolute child indices, ``root``; ``value`` the node mean of y_hat).
    ``weights`` [T, n] overrides the bootstrap; ``with_weights`` adds ``weighted_n_node_samples``."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    q, s = quantise(y)
    n, d = X32.shape
    mf = N.resolve_max_features(max_features, d)
    parts, root = [], [0]
    for t in range(n_estimators):
        w = np.asarray(weights[t], dtype=np.int64) if weights is not None else (N.bootstrap_weights(seed, t, n) if bootstrap else np.ones(n, dtype=np.int64))
        l, r, f, thr, v, nns, wns = fit_tree(X32, q, w, N.tree_key(seed, t), max_depth, min_samples_split, min_samples_leaf, mf)
        off = root[-1]
        parts.append((np.where(l >= 0, l + off, -1).astype(np.int32), np.where(r >= 0, r + off, -1).astype(np.int32), f, thr, np.ldexp(v, -s), nns, wns))
        root.append(off + len(l))
    cat = lambda i: np.concatenate([p[i] for p in parts])  # noqa: E731
    out = dict(left=cat(0), right=cat(1), feature=cat(2), threshold=cat(3), value=cat(4), n_node_samples=cat(5), root=np.asarray(root, dtype=np.int32))
    if with_weights:
        out["weighted_n_node_samples"] = cat(6)
    return out


def predict(trees, X, limits=None):
    """scikit-learn's forest arithmetic: the leaf values summed over trees in tree order in float64, divided by the number of trees.
    ``limits = (n_trees, max_depth, min_samples_split)`` stops every walk as a fit under them would."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    T, depth_limit, mss = (len(trees["root"]) - 1, None, 0) if limits is None else limits
    depth_limit = N.UNLIMITED if depth_limit is None else depth_limit
    out = np.zeros(len(X32))
    for t in range(T):
        node = np.full(len(X32), trees["root"][t], dtype=np.int64)
        depth = 0
        while True:
            go = (trees["left"][node] >= 0) & (trees["n_node_samples"][node] >= mss) & (depth < depth_limit)
            if not go.any():
                break
            x = X32[np.arange(len(X32)), trees["feature"][node]].astype(np.float64)
            nxt = np.where(x <= trees["threshold"][node], trees["left"][node], trees["right"][node])
            node = np.where(go, nxt, node)
            depth += 1
        out = out + trees["value"][node]
    return out / np.float64(T)
