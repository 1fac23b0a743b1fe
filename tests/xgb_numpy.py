"""``bbbp_amd.xgb`` restated in numpy: XGBoost 2.0's ``hist`` updater for ``reg:squarederror`` with no sum that has an order.

The module docstring of ``bbbp_amd/xgb.py`` states the algorithm; this file is the same algorithm once more, written for reading, and the
GPU fit must equal it bit for bit (``tests/test_gpu_xgb.py``).  Nothing here imports the package.

* ``cuts`` / ``bins`` / ``quantise``: the cut points of a column, ``bin(x)`` = the number of cuts ``<= x``, and a matrix's live columns.
* ``gain`` / ``weight``: the split score and the node weight in float64, every operation rounded on its own.
* ``fit``: the boosted trees; ``predict``: XGBoost's walk, margins summed as the fit sums them.

A node's gradient sum is an exact integer: ``g_i = margin_i - y_i`` in float32, ``k = 47 - ilogb(max |g|)``, ``q_i = rint(g_i 2^k)``,
``Q = sum q_i`` (``|Q| <= 2^61`` for ``n <= 8192``) and ``G = ldexp(float64(Q), -k)``.  A histogram over bins and a sort by bin give the same
``Q`` left of every boundary, so this file sorts: the candidates of a feature are the boundaries behind every occupied bin but the last, and
a boundary behind an empty bin parts the rows like the occupied bin below it, which has the lower index and wins the tie.
"""
import numpy as np

MAX_ROWS, RT_EPS = 8192, 1e-6


def cuts(col, max_bin=256):
    """The cut points of one float32 column: every distinct value above the minimum when there are at most ``max_bin`` distinct values,
    otherwise the distinct values among ``s[floor(j n / max_bin)]``, ``j = 1 .. max_bin - 1``, that exceed the minimum.  A cut of -0.0 is
    stored as +0.0 (they compare equal; which of the two a sort keeps is not defined)."""
    s = np.sort(np.asarray(col, np.float32)) + np.float32(0)
    distinct = np.unique(s)
    if len(distinct) <= max_bin:
        return distinct[1:]
    n = len(s)
    picks = np.unique(s[[(j * n) // max_bin for j in range(1, max_bin)]])
    return picks[picks > s[0]]


def bins(col, c):
    """``bin(x)``: the number of cuts ``<= x``, one byte."""
    return np.searchsorted(c, np.asarray(col, np.float32), side="right").astype(np.uint8)


def quantise(X, max_bin=256):
    """(the indices of the live columns, their cuts, the bin matrix [d_live, n]); a column without a cut is constant and dropped."""
    X = np.asarray(X, np.float32)
    live, cc, B = [], [], []
    for f in range(X.shape[1]):
        c = cuts(X[:, f], max_bin)
        if len(c):
            live.append(f); cc.append(c); B.append(bins(X[:, f], c))
    return np.asarray(live, np.int64), cc, (np.stack(B) if B else np.zeros((0, X.shape[0]), np.uint8))


def term(G, H, lam):
    return G * G / (H + lam)


def gain(G_l, H_l, G_r, H_r, G, H, lam):
    """float64, each operation rounded on its own.  The parent's ``G`` comes from its own integer sum, not from ``G_l + G_r``."""
    return (term(G_l, H_l, lam) + term(G_r, H_r, lam)) - term(G, H, lam)


def weight(G, H, lam):
    return -G / (H + lam)


def to_G(Q, k):
    """A node's gradient sum from its integer sum: one rounding (int64 -> float64), then an exact scaling."""
    return np.ldexp(np.asarray(Q, np.int64).astype(np.float64), -k)


def quantise_gradients(g):
    """(k, q): ``k = 47 - ilogb(max |g|)`` (0 when every g is 0) and ``q_i = rint(g_i 2^k)`` as int64, the product being exact."""
    gmax = np.float32(np.max(np.abs(g)))
    if gmax == 0:
        return 0, np.zeros(len(g), np.int64)
    k = 47 - (int(np.frexp(np.float64(gmax))[1]) - 1)
    return k, np.rint(np.ldexp(g.astype(np.float64), k)).astype(np.int64)


def best_split(B, q, rows, k, lam, min_rows):
    """The best candidate of a node: (gain, live feature, bin, Q_left, m_left) or None.  Ties: the lowest feature, then the lowest bin."""
    m = len(rows)
    if m < 2 or B.shape[0] == 0:
        return None
    b = B[:, rows].astype(np.int64)                                   # [d, m]
    order = np.argsort(b, axis=1, kind="stable")
    sb = np.take_along_axis(b, order, axis=1)
    cq = np.cumsum(q[rows][order], axis=1)                            # exact: int64
    m_l = np.arange(1, m)[None, :]
    valid = (sb[:, :-1] != sb[:, 1:]) & (m_l >= min_rows) & (m - m_l >= min_rows)
    if not valid.any():
        return None
    Q = int(q[rows].sum())
    Q_l = cq[:, :-1]
    g = gain(to_G(Q_l, k), m_l.astype(np.float64), to_G(Q - Q_l, k), (m - m_l).astype(np.float64), to_G(Q, k), np.float64(m), np.float64(lam))
    g = np.where(valid, g, -np.inf)
    f, j = np.unravel_index(int(np.argmax(g)), g.shape)               # the first maximum in (feature, position) order = (feature, bin) order
    return float(g[f, j]), int(f), int(sb[f, j]), int(Q_l[f, j]), int(j + 1)


def fit(X, y, n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0, max_bin=256, base_score=None):
    """The boosted trees as flat arrays in ``boosters.XGBTrees``' convention (``left`` / ``right`` absolute, -1 at a leaf; ``cond`` the
    threshold or the leaf's value; ``root`` the tree offsets) with XGBoost's recorded statistics per node and the training margins."""
    X = np.asarray(X, np.float32)
    y32 = np.asarray(y).astype(np.float32)
    n = X.shape[0]
    assert 2 <= n <= MAX_ROWS and 2 <= max_bin <= 256
    live, cc, B = quantise(X, max_bin)
    base = np.float32(np.mean(np.asarray(y, np.float64))) if base_score is None else np.float32(base_score)
    eta = np.float64(np.float32(learning_rate))
    lam = np.float64(reg_lambda)
    min_rows = max(1, int(np.ceil(min_child_weight)))
    margin = np.full(n, base, np.float32)
    out = {k_: [] for k_ in ("left", "right", "feature", "cond", "base_weights", "loss_changes", "sum_hessian", "parents")}
    root = [0]
    for _ in range(n_estimators):
        g = margin - y32                                              # float32
        k, q = quantise_gradients(g)
        off = root[-1]
        nodes = [dict(rows=np.arange(n), depth=0, parent=-1)]         # ids in creation order: level by level, ascending
        value = np.zeros(n, np.float32)
        i = 0
        while i < len(nodes):
            nd = nodes[i]
            rows = nd["rows"]
            m = len(rows)
            Q = int(q[rows].sum())
            w = weight(to_G(Q, k), np.float64(m), lam)
            best = best_split(B, q, rows, k, lam, min_rows) if nd["depth"] < max_depth else None
            if best is not None and best[0] > RT_EPS and best[0] >= gamma:
                gn, f, b, _, _ = best
                go_left = B[f, rows] <= b
                nd.update(left=len(nodes), right=len(nodes) + 1, feature=int(live[f]), cond=cc[f][b], bw=np.float32(w), loss=np.float32(gn))
                nodes.append(dict(rows=rows[go_left], depth=nd["depth"] + 1, parent=i))
                nodes.append(dict(rows=rows[~go_left], depth=nd["depth"] + 1, parent=i))
            else:
                v = np.float32(eta * w)
                nd.update(left=-1, right=-1, feature=0, cond=v, bw=v, loss=np.float32(0))
                value[rows] = v
            nd["hess"] = np.float32(m)
            i += 1
        margin = margin + value                                       # float32
        out["left"] += [nd["left"] + off if nd["left"] >= 0 else -1 for nd in nodes]
        out["right"] += [nd["right"] + off if nd["right"] >= 0 else -1 for nd in nodes]
        out["parents"] += [nd["parent"] + off if nd["parent"] >= 0 else -1 for nd in nodes]
        for key, name in (("feature", "feature"), ("cond", "cond"), ("base_weights", "bw"), ("loss_changes", "loss"), ("sum_hessian", "hess")):
            out[key] += [nd[name] for nd in nodes]
        root.append(off + len(nodes))
    res = {k_: np.asarray(v, np.float32 if k_ in ("cond", "base_weights", "loss_changes", "sum_hessian") else np.int32) for k_, v in out.items()}
    res.update(root=np.asarray(root, np.int32), default_left=np.zeros(root[-1], np.uint8), base_score=base, train_margin=margin,
               n_features=X.shape[1])
    return res


def predict(model, X):
    """XGBoost's walk (left when ``x[feature] < cond``), the margin summed as the fit sums it: ``base_score``, then the trees in order."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    out = np.full(n, model["base_score"], np.float32)
    left, right, feature, cond = model["left"], model["right"], model["feature"], model["cond"]
    for t in range(len(model["root"]) - 1):
        node = np.full(n, model["root"][t], np.int64)
        while (left[node] >= 0).any():
            inner = left[node] >= 0
            go_left = X[np.arange(n), feature[node]] < cond[node]
            node = np.where(inner, np.where(go_left, left[node], right[node]), node)
        out = out + cond[node]
    return out
