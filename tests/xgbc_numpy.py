"""``bbbp_amd.xgb.XGBClassifier`` restated in numpy: XGBoost 2.0's ``hist`` updater for ``binary:logistic`` with no sum that has an order.

The module docstring of ``bbbp_amd/xgb.py`` states the algorithm; this file is the same algorithm once more, written for reading, and the
GPU fit must equal it bit for bit (``tests/test_gpu_xgbc.py``).  Nothing here imports the package; cuts and bins are ``xgb_numpy``'s.

* ``sigmoid32``: the float32 sigmoid of a float32 margin from IEEE operations only (float64 inside, one rounding at the end).
* ``mix`` / ``draw``: the counter-based hash behind the row and the column sampling; ``row_sample`` / ``column_masks``: the two draws.
* ``fit``: the boosted trees; ``predict_margin`` / ``predict_proba``: XGBoost's walk, margins summed as the fit sums them.

A node carries two exact integers: ``Q = sum q_i`` as in the regressor (``gmax`` over the tree's sampled rows) and ``R = sum r_i`` with
``r_i = max(1, rint(h_i 2^48))``, ``h_i = p_i (1 - p_i) <= 1/4``, so ``R <= 2^59`` for ``n <= 8192``; ``H = ldexp(float64(R), -48)``.  A row that
the tree's draw left out has ``q_i = r_i = 0`` and stays in the row list.
"""
import numpy as np

import xgb_numpy as xn

MAX_ROWS, RT_EPS = xn.MAX_ROWS, xn.RT_EPS
LN2_HI, LN2_LO, INV_LN2 = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33"), float.fromhex("0x1.71547652b82fep+0")
EXP_COEFFS = [1.0 / float(np.prod(np.arange(1, j + 1, dtype=np.float64))) for j in range(14)]          # 1 / j!, j! exact in float64
GOLDEN, M1, M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
ROW_STREAM, COLUMN_STREAM = 0, 1


def sigmoid32(x):
    """``float32(1 / (1 + exp(-x)))`` of float32 margins: ``exp(-|x|)`` by fdlibm's reduction and a degree-13 Taylor polynomial in float64."""
    z = np.asarray(x, np.float32).astype(np.float64)
    a = np.maximum(-np.abs(z), -87.0)                                 # the clamp keeps p a normal float32
    k = np.rint(a * INV_LN2)
    r = (a - k * LN2_HI) - k * LN2_LO
    P = np.full_like(r, EXP_COEFFS[13])
    for j in range(12, -1, -1):
        P = P * r + EXP_COEFFS[j]
    e = np.ldexp(P, k.astype(np.int32))
    s = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return s.astype(np.float32)


def mix(x):
    """The splitmix64 finaliser on uint64 arrays (arrays wrap modulo 2^64 without a warning)."""
    x = np.atleast_1d(np.asarray(x, np.uint64)).copy()
    x ^= x >> np.uint64(30); x *= M1
    x ^= x >> np.uint64(27); x *= M2
    x ^= x >> np.uint64(31)
    return x


def draw(seed, stream, tree, i):
    """``u(stream, tree, i) = mix(mix(mix(seed + GOLDEN (stream + 1)) + tree) + i)`` as uint64, broadcast over ``tree`` and ``i``."""
    s = np.full(1, int(seed) % 2 ** 64, np.uint64) + np.full(1, GOLDEN) * np.uint64(stream + 1)
    return mix(mix(mix(s) + np.asarray(tree, np.uint64)) + np.asarray(i, np.uint64))


def subsample_threshold(subsample):
    """0 when nothing is sampled out, else ``max(1, floor(subsample 2^32))``."""
    return 0 if subsample >= 1.0 else max(1, int(np.floor(float(subsample) * 2.0 ** 32)))


def row_sample(seed, tree, n, subsample):
    """bool [n]: which rows tree ``tree`` uses; row ``i`` is in iff ``(u >> 32) < floor(subsample 2^32)``."""
    thr = subsample_threshold(subsample)
    if thr == 0:
        return np.ones(n, bool)
    return (draw(seed, ROW_STREAM, tree, np.arange(n)) >> np.uint64(32)) < np.uint64(thr)


def column_masks(seed, n_trees, cols, colsample):
    """bool [n_trees, len(cols)]: per tree the ``max(1, floor(colsample d_live))`` live columns with the smallest ``(u, original index)``."""
    cols = np.asarray(cols, np.int64)
    d = len(cols)
    masks = np.ones((n_trees, d), bool)
    if colsample >= 1.0 or d == 0:
        return masks
    keep = max(1, int(np.floor(float(colsample) * d)))
    u = draw(seed, COLUMN_STREAM, np.arange(n_trees)[:, None], cols[None, :])
    order = np.argsort(u, axis=1, kind="stable")                      # cols ascend: stable means (u, index)
    masks[:] = False
    np.put_along_axis(masks, order[:, :keep], True, axis=1)
    return masks


def to_H(R):
    return np.ldexp(np.asarray(R, np.int64).astype(np.float64), -48)


def initial_margin(t, base_score=None):
    """(m0, base_score_): ``float32(4 (mean(t) - 0.5))`` and its sigmoid, or the logit of a given probability and the probability."""
    if base_score is None:
        m0 = np.float32(4.0 * (np.mean(np.asarray(t, np.float64)) - 0.5))
        return m0, sigmoid32(m0)[()]
    p = float(base_score)
    assert 0.0 < p < 1.0
    return np.float32(np.log(p / (1.0 - p))), np.float32(p)


def best_split(B, q, r, rows, k, lam, mcw, eligible):
    """The best candidate of a node: (gain, live feature, bin, Q_left, R_left, m_left) or None.  Ties: the lowest feature, then the lowest bin."""
    m = len(rows)
    if m < 2 or B.shape[0] == 0:
        return None
    b = B[:, rows].astype(np.int64)
    order = np.argsort(b, axis=1, kind="stable")
    sb = np.take_along_axis(b, order, axis=1)
    Q_l = np.cumsum(q[rows][order], axis=1)[:, :-1]                   # exact: int64
    R_l = np.cumsum(r[rows][order], axis=1)[:, :-1]
    Q, R = int(q[rows].sum()), int(r[rows].sum())
    H_l, H_r = to_H(R_l), to_H(R - R_l)
    valid = (sb[:, :-1] != sb[:, 1:]) & (R_l >= 1) & (R - R_l >= 1) & (H_l >= mcw) & (H_r >= mcw) & eligible[:, None]
    if not valid.any():
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        g = xn.gain(xn.to_G(Q_l, k), H_l, xn.to_G(Q - Q_l, k), H_r, xn.to_G(Q, k), to_H(R), np.float64(lam))
    g = np.where(valid, g, -np.inf)
    f, j = np.unravel_index(int(np.argmax(g)), g.shape)
    return float(g[f, j]), int(f), int(sb[f, j]), int(Q_l[f, j]), int(R_l[f, j]), int(j + 1)


def fit(X, y, n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0, max_bin=256, base_score=None,
        subsample=1.0, colsample_bytree=1.0, random_state=None):
    """The boosted trees as flat arrays in ``boosters.XGBTrees``' convention with XGBoost's recorded statistics per node, ``classes``,
    ``base_margin`` (m0), ``base_score`` (a probability), the training margins, the draws -- ``live`` / ``col_masks`` [T, d_live] and
    ``row_masks`` [T, n] -- and per tree ``gmax`` and ``floored``, the number of sampled rows whose ``r`` the floor of 1 raised."""
    X = np.asarray(X, np.float32)
    classes = np.unique(np.asarray(y))
    assert len(classes) == 2
    t32 = (np.asarray(y) == classes[1]).astype(np.float32)
    n = X.shape[0]
    assert 2 <= n <= MAX_ROWS and 2 <= max_bin <= 256
    live, cc, B = xn.quantise(X, max_bin)
    seed = 0 if random_state is None else int(random_state)
    m0, base = initial_margin(t32, base_score)
    eta, lam, mcw = np.float64(np.float32(learning_rate)), np.float64(reg_lambda), np.float64(min_child_weight)
    col_masks = column_masks(seed, n_estimators, live, colsample_bytree)
    row_masks = np.stack([row_sample(seed, t, n, subsample) for t in range(n_estimators)])
    margin = np.full(n, m0, np.float32)
    out = {k_: [] for k_ in ("left", "right", "feature", "cond", "base_weights", "loss_changes", "sum_hessian", "parents")}
    root, gmax, floored = [0], [], []
    for tree in range(n_estimators):
        p = sigmoid32(margin)
        g = p - t32                                                   # float32
        h = p * (np.float32(1) - p)                                   # float32, the subtraction and the product each rounded
        used = row_masks[tree]
        k, q = xn.quantise_gradients(g[used]) if used.any() else (0, None)
        q_all, r_all = np.zeros(n, np.int64), np.zeros(n, np.int64)
        if used.any():
            q_all[used] = q
            r_all[used] = np.maximum(1, np.rint(np.ldexp(h[used].astype(np.float64), 48)).astype(np.int64))
        gmax.append(np.float32(np.abs(g[used]).max()) if used.any() else np.float32(0))
        floored.append(int((np.rint(np.ldexp(h[used].astype(np.float64), 48)) < 1).sum()))
        off = root[-1]
        nodes = [dict(rows=np.arange(n), depth=0, parent=-1)]
        value = np.zeros(n, np.float32)
        i = 0
        while i < len(nodes):
            nd = nodes[i]
            rows = nd["rows"]
            Q, R = int(q_all[rows].sum()), int(r_all[rows].sum())
            H = to_H(R)
            w = np.float64(-0.0) if R == 0 else xn.weight(xn.to_G(Q, k), H, lam)
            best = best_split(B, q_all, r_all, rows, k, lam, mcw, col_masks[tree]) if nd["depth"] < max_depth else None
            if best is not None and best[0] > RT_EPS and best[0] >= gamma:
                gn, f, b = best[:3]
                go_left = B[f, rows] <= b
                nd.update(left=len(nodes), right=len(nodes) + 1, feature=int(live[f]), cond=cc[f][b], bw=np.float32(w), loss=np.float32(gn))
                nodes.append(dict(rows=rows[go_left], depth=nd["depth"] + 1, parent=i))
                nodes.append(dict(rows=rows[~go_left], depth=nd["depth"] + 1, parent=i))
            else:
                v = np.float32(eta * w)
                nd.update(left=-1, right=-1, feature=0, cond=v, bw=v, loss=np.float32(0))
                value[rows] = v
            nd["hess"] = np.float32(H)
            i += 1
        margin = margin + value                                       # float32
        out["left"] += [nd["left"] + off if nd["left"] >= 0 else -1 for nd in nodes]
        out["right"] += [nd["right"] + off if nd["right"] >= 0 else -1 for nd in nodes]
        out["parents"] += [nd["parent"] + off if nd["parent"] >= 0 else -1 for nd in nodes]
        for key, name in (("feature", "feature"), ("cond", "cond"), ("base_weights", "bw"), ("loss_changes", "loss"), ("sum_hessian", "hess")):
            out[key] += [nd[name] for nd in nodes]
        root.append(off + len(nodes))
    res = {k_: np.asarray(v, np.float32 if k_ in ("cond", "base_weights", "loss_changes", "sum_hessian") else np.int32) for k_, v in out.items()}
    res.update(root=np.asarray(root, np.int32), default_left=np.zeros(root[-1], np.uint8), base_score=base, base_margin=m0, train_margin=margin,
               n_features=X.shape[1], classes=classes, live=live, col_masks=col_masks, row_masks=row_masks, gmax=np.asarray(gmax, np.float32),
               floored=np.asarray(floored, np.int64))
    return res


def predict_margin(model, X, offset_last=False):
    """XGBoost's walk (left when ``x[feature] < cond``), the margin summed as the fit sums it: ``m0``, then the trees in order.  With
    ``offset_last`` the trees are summed from 0 in float32 and ``m0`` is added last, which is the predict kernel's order."""
    if not offset_last:
        return xn.predict({**model, "base_score": model["base_margin"]}, X)
    return np.float32(model["base_margin"]) + xn.predict({**model, "base_score": np.float32(0)}, X)


def proba_of_margin(margin):
    """float32 [m, 2]: ``(1 - p1, p1)`` with ``p1 = sigmoid32(margin)``, the subtraction in float32, as XGBoost's wrapper forms it."""
    p1 = sigmoid32(margin)
    return np.stack([np.float32(1) - p1, p1], axis=1)


def predict_proba(model, X):
    """What ``XGBClassifier.predict_proba`` returns: the margins in the predict kernel's order, then ``proba_of_margin``."""
    return proba_of_margin(predict_margin(model, X, offset_last=True))
