"""numpy restatement of ``isolation_forest``: the fit rule of csrc/iforest.hip (the hash keys, the sub-sample, the hashed feature order, the
threshold in three float64 roundings, the level-by-level numbering) and scikit-learn's scoring arithmetic (``ensemble/_iforest.py``:
``_average_path_length``, the path terms, ``_compute_score_samples``).  The GPU's trees equal these bit for bit; the scoring half is pinned
to scikit-learn on the CPU (tests/test_iforest_cpu.py).  Plain numpy, no GPU, nothing imported from the package."""
import numpy as np

from rf_numpy import M64, rf_hash

TAG = 0x1F0BE57                 # key(root of tree t) = hash(hash(seed, TAG), t): apart from the forests' hash(seed, t)
SAMPLE = 0x5A3B1E               # the stream of a tree's row hashes: hash(hash(key(root), SAMPLE), row)
THRESHOLD = 0x7412E5            # a node's threshold draw: hash(key, THRESHOLD); features use 2 + f, the children's keys 0 and 1
FEATURE_THRESHOLD = np.float32(1e-7)
MAX_SAMPLES = 1024              # BBBP_IFOREST_MAX_SAMPLES


def tree_key(seed, t):
    return int(rf_hash(rf_hash(int(seed) & M64, TAG), t))


def child_key(key, side):
    return int(rf_hash(key, side))


def sample_rows(seed, t, n, max_samples):
    """The tree's rows, ascending: the ``max_samples`` rows with the lowest hash (a bijection of the row: no ties)."""
    h = rf_hash(rf_hash(tree_key(seed, t), SAMPLE), np.arange(n, dtype=np.uint64))
    return np.sort(np.argsort(h, kind="stable")[:max_samples]).astype(np.int32)


def non_constant(lo, hi):
    """scikit-learn's rule in float32: a feature is constant on a node when max <= min + 1e-7f."""
    return hi > (lo + FEATURE_THRESHOLD).astype(np.float32)


def feature_order(key, d):
    """The node's features in ascending order of hash(key, 2 + f)."""
    return np.argsort(rf_hash(key, np.uint64(2) + np.arange(d, dtype=np.uint64)), kind="stable")


def draw_threshold(key, lo, hi):
    """lo + (hi - lo) u in float64, u = (hash(key, THRESHOLD) >> 11) 2^-53: one rounding per operation; a threshold that reaches hi is lo."""
    u = np.float64(int(rf_hash(key, THRESHOLD)) >> 11) * np.float64(2.0 ** -53)
    lo, hi = np.float64(lo), np.float64(hi)
    thr = lo + (hi - lo) * u
    return lo if thr >= hi else thr


def depth_limit(max_samples):
    return int(np.ceil(np.log2(max(max_samples, 2))))


def fit_tree(X32, rows, key, max_depth):
    """One tree on ``rows``: tree-relative children, nodes numbered level by level."""
    d = X32.shape[1]
    left, right, feature, threshold, nns = [], [], [], [], []
    level, total, depth = [(rows, key)], 1, 0
    while level:
        nxt = []
        for rws, k in level:
            m, split = len(rws), None
            nns.append(m)
            if m >= 2 and depth < max_depth:
                Xn = X32[rws]
                lo, hi = Xn.min(axis=0), Xn.max(axis=0)
                nc = non_constant(lo, hi)
                if nc.any():
                    split = next(int(f) for f in feature_order(k, d) if nc[f])
            if split is None:
                left.append(-1); right.append(-1); feature.append(0); threshold.append(-2.0)
                continue
            thr = draw_threshold(k, lo[split], hi[split])
            goes = Xn[:, split].astype(np.float64) <= thr
            at = total + len(nxt)
            left.append(at); right.append(at + 1); feature.append(split); threshold.append(thr)
            nxt += [(rws[goes], child_key(k, 0)), (rws[~goes], child_key(k, 1))]
        total += len(nxt)
        level, depth = nxt, depth + 1
    return (np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64), np.asarray(feature, dtype=np.int32),
            np.asarray(threshold, dtype=np.float64), np.asarray(nns, dtype=np.int32))


def fit_forest(X, n_estimators, max_samples, seed):
    """(trees, samples): the flat trees of ``IsolationForest.trees_`` (``value`` the path term) and int32 [T, max_samples] rows.
    ``max_samples`` is the resolved count, at most n."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    n = X32.shape[0]
    assert 1 <= max_samples <= min(n, MAX_SAMPLES)
    parts, samples, root = [], [], [0]
    for t in range(n_estimators):
        rows = sample_rows(seed, t, n, max_samples)
        l, r, f, thr, nns = fit_tree(X32, rows, tree_key(seed, t), depth_limit(max_samples))
        off = root[-1]
        parts.append((np.where(l >= 0, l + off, -1).astype(np.int32), np.where(r >= 0, r + off, -1).astype(np.int32), f, thr, nns))
        samples.append(rows)
        root.append(off + len(l))
    cat = lambda i: np.concatenate([p[i] for p in parts])  # noqa: E731
    trees = dict(left=cat(0), right=cat(1), feature=cat(2), threshold=cat(3), n_node_samples=cat(4), root=np.asarray(root, dtype=np.int32))
    trees["value"] = path_terms(trees)
    return trees, np.stack(samples)


# ---- scoring: scikit-learn's arithmetic -----------------------------------------------------------------------------------------------------
def average_path_length(n_samples_leaf):
    """``_average_path_length`` with ``np.log`` and ``np.euler_gamma``, on an integer array as scikit-learn calls it."""
    n = np.asarray(n_samples_leaf, dtype=np.int64)
    shape = n.shape
    n = n.reshape((1, -1))
    out = np.zeros(n.shape)
    one, two = n <= 1, n == 2
    rest = ~np.logical_or(one, two)
    out[one] = 0.0
    out[two] = 1.0
    out[rest] = 2.0 * (np.log(n[rest] - 1.0) + np.euler_gamma) - 2.0 * (n[rest] - 1.0) / n[rest]
    return out.reshape(shape)


def node_depths(trees):
    """Depth counted from 1 at the root, int64 (``tree_.compute_node_depths()``), whatever the numbering."""
    left, right, root = trees["left"], trees["right"], trees["root"]
    depth = np.zeros(len(left), dtype=np.int64)
    for t in range(len(root) - 1):
        stack = [(int(root[t]), 1)]
        while stack:
            node, at = stack.pop()
            depth[node] = at
            if left[node] >= 0:
                stack += [(int(left[node]), at + 1), (int(right[node]), at + 1)]
    return depth


def path_terms(trees):
    """``(depth + c(n_node_samples)) - 1.0`` per node: what ``_parallel_compute_tree_depths`` adds for a row whose walk ends there."""
    return (node_depths(trees) + average_path_length(trees["n_node_samples"])) - 1.0


def leaves(trees, X):
    """int64 [T, m]: the node every query row ends in, per tree ((double)x <= threshold goes left)."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    m, rows = X32.shape[0], np.arange(X32.shape[0])
    left, right, feature, threshold, root = trees["left"], trees["right"], trees["feature"], trees["threshold"], trees["root"]
    out = np.empty((len(root) - 1, m), dtype=np.int64)
    for t in range(len(root) - 1):
        node = np.full(m, int(root[t]), dtype=np.int64)
        while True:
            inner = left[node] >= 0
            if not inner.any():
                break
            goes = X32[rows, feature[node]].astype(np.float64) <= threshold[node]
            node = np.where(inner, np.where(goes, left[node], right[node]), node)
        out[t] = node
    return out


def path_sums(trees, X, terms=None):
    """float64 [m]: the terms of the rows' leaves added tree after tree, as scikit-learn's ``depths +=`` does."""
    terms = path_terms(trees) if terms is None else terms
    at = leaves(trees, X)
    out = np.zeros(at.shape[1])
    for t in range(at.shape[0]):
        out += terms[at[t]]
    return out


def scores_of_path_sums(sums, n_trees, max_samples):
    """``_compute_score_samples``' last lines and ``score_samples``' sign."""
    denominator = n_trees * average_path_length([max_samples])
    return -(2 ** (-np.divide(sums, denominator, out=np.ones_like(sums), where=denominator != 0)))


def score_samples(trees, X, max_samples):
    return scores_of_path_sums(path_sums(trees, X), len(trees["root"]) - 1, max_samples)


def offset(trees, X_train, max_samples, contamination):
    return -0.5 if isinstance(contamination, str) else np.percentile(score_samples(trees, X_train, max_samples), 100.0 * contamination)


def predict(trees, X, max_samples, offset_):
    out = np.ones(np.shape(X)[0], dtype=int)
    out[score_samples(trees, X, max_samples) - offset_ < 0] = -1
    return out
