"""numpy restatement of ``random_forest``'s fit (csrc/rf.hip): the hash, the bootstrap, the feature draws, the scores, the tie rule and the
level-by-level numbering.  Every quantity is an integer or one correctly rounded float64 division, so the GPU's trees equal these bit for
bit.  Plain numpy, no GPU."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
BOOT = 0xB007
FEATURE_THRESHOLD = np.float32(1e-7)
UNLIMITED = 1 << 30


def _mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def rf_hash(a, b):
    """mix(mix(a) + GOLDEN (b + 1)) over uint64, mix = splitmix64's finaliser; ``a`` and ``b`` scalars or arrays.  Returns uint64."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return _mix(_mix(a) + np.uint64(GOLDEN) * (b + np.uint64(1)))


def tree_key(seed, t):
    return int(rf_hash(int(seed) & M64, t))


def child_key(key, side):
    return int(rf_hash(key, side))


def bootstrap_weights(seed, t, n):
    """The histogram of n draws hash(hash(key(root), BOOT), j) mapped to [0, n) by multiply-high."""
    stream = rf_hash(tree_key(seed, t), BOOT)
    h = rf_hash(stream, np.arange(n, dtype=np.uint64))
    hi, lo = h >> np.uint64(32), h & np.uint64(0xFFFFFFFF)
    rows = (hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)      # floor(h n / 2^64), n < 2^32
    return np.bincount(rows.astype(np.int64), minlength=n).astype(np.int64)


def non_constant(Xn):
    """Which features are not constant in a node whose rows' float32 values are ``Xn`` [m, d]: max > min + 1e-7f in float32."""
    return Xn.max(axis=0) > (Xn.min(axis=0) + FEATURE_THRESHOLD).astype(np.float32)


def draw_features(key, Xn, max_features):
    """The node's candidate features, ascending: the ``max_features`` non-constant features with the lowest (hash(key, 2 + f), f)."""
    d = Xn.shape[1]
    nc = np.nonzero(non_constant(Xn))[0]
    h = rf_hash(key, np.uint64(2) + np.arange(d, dtype=np.uint64))[nc]
    pick = nc[np.lexsort((nc, h))][:max_features]
    return np.sort(pick)


def midpoint(a, b):
    thr = np.float64(a) / 2.0 + np.float64(b) / 2.0
    return np.float64(a) if thr == np.float64(b) else thr


def position_scores(fv, w, w1, msl):
    """Valid positions of a node in one feature's order (``fv`` float32 ascending, ``w`` / ``w1`` the rows' weights and class-1 weights in that
    order) and (numerator, denominator) of their scores as exact int64: (W_R L_1 - W_L R_1)^2 and W_L W_R."""
    m = len(fv)
    p = np.arange(1, m)
    ok = (fv[1:] > (fv[:-1] + FEATURE_THRESHOLD).astype(np.float32)) & (p >= msl) & (m - p >= msl)
    p = p[ok]
    WL, L1 = np.cumsum(w)[p - 1], np.cumsum(w1)[p - 1]
    W, W1 = int(w.sum()), int(w1.sum())
    WR, R1 = W - WL, W1 - L1
    diff = WR * L1 - WL * R1
    return p, diff * diff, WL * WR


def fit_tree(X32, y01, w, key, max_depth, min_samples_split, min_samples_leaf, max_features):
    """One tree over the rows of positive weight.  Returns tree-relative arrays (left, right, feature, threshold, value, n_node_samples)."""
    n, d = X32.shape
    depth_limit = UNLIMITED if max_depth is None else int(max_depth)
    left, right, feature, threshold, value, nns = [-1], [-1], [0], [-2.0], [0.0], [0]
    level = [(0, np.nonzero(w > 0)[0], key)]
    depth = 0
    while level:
        nxt = []
        for node, rows, k in level:
            m = len(rows)
            W, W1 = int(w[rows].sum()), int((w[rows] * y01[rows]).sum())
            nns[node], value[node] = m, np.float64(W1) / np.float64(W)
            if depth >= depth_limit or m < min_samples_split or m < 2 * min_samples_leaf or W1 == 0 or W1 == W:
                continue
            best = None                                   # (score, feature, position, a, b)
            for f in draw_features(k, X32[rows], max_features):
                o = np.argsort(X32[rows, f], kind="stable")
                fv = X32[rows, f][o]
                p, num, den = position_scores(fv, w[rows][o], (w[rows] * y01[rows])[o], min_samples_leaf)
                if not len(p):
                    continue
                score = num.astype(np.float64) / den.astype(np.float64)
                j = int(np.argmax(score))                 # the lowest position among equal scores
                if best is None or score[j] > best[0]:    # the lowest feature among equal scores
                    best = (score[j], int(f), int(p[j]), fv[p[j] - 1], fv[p[j]])
            if best is None:
                continue
            _, f, p, a, b = best
            thr = midpoint(a, b)
            goes_left = X32[rows, f].astype(np.float64) <= thr
            lc = len(left)
            for _ in range(2):
                left.append(-1); right.append(-1); feature.append(0); threshold.append(-2.0); value.append(0.0); nns.append(0)
            left[node], right[node], feature[node], threshold[node] = lc, lc + 1, f, float(thr)
            nxt.append((lc, rows[goes_left], child_key(k, 0)))
            nxt.append((lc + 1, rows[~goes_left], child_key(k, 1)))
        level = nxt
        depth += 1
    return (np.asarray(left, dtype=np.int32), np.asarray(right, dtype=np.int32), np.asarray(feature, dtype=np.int32),
            np.asarray(threshold, dtype=np.float64), np.asarray(value, dtype=np.float64), np.asarray(nns, dtype=np.int32))


def resolve_max_features(max_features, d):
    if max_features is None:
        return d
    if max_features == "sqrt":
        return max(1, int(np.sqrt(d)))
    if max_features == "log2":
        return max(1, int(np.log2(d)))
    return int(max_features)


def fit_forest(X, y01, n_estimators, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features="sqrt", bootstrap=True, seed=0,
               weights=None):
    """The forest's trees in the flat convention of ``trees_`` (absolute child indices, ``root``).  ``weights`` [T, n] overrides the bootstrap."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    y01 = np.asarray(y01).astype(np.int64)
    n, d = X32.shape
    mf = resolve_max_features(max_features, d)
    parts, root = [], [0]
    for t in range(n_estimators):
        w = np.asarray(weights[t], dtype=np.int64) if weights is not None else (bootstrap_weights(seed, t, n) if bootstrap else np.ones(n, dtype=np.int64))
        l, r, f, thr, v, nns = fit_tree(X32, y01, w, tree_key(seed, t), max_depth, min_samples_split, min_samples_leaf, mf)
        off = root[-1]
        parts.append((np.where(l >= 0, l + off, -1).astype(np.int32), np.where(r >= 0, r + off, -1).astype(np.int32), f, thr, v, nns))
        root.append(off + len(l))
    cat = lambda i: np.concatenate([p[i] for p in parts])  # noqa: E731
    return dict(left=cat(0), right=cat(1), feature=cat(2), threshold=cat(3), value=cat(4), n_node_samples=cat(5), root=np.asarray(root, dtype=np.int32))
