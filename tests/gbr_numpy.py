"""A sequential numpy restatement of the fit kernels of csrc/gbt.hip under the squared error (bbbp_gbr_fit), for the CPU suite: the same
row keys, per-level segment tables, stable partition with the kernel's destination rule (asserted to hit every slot once), level-order node
numbering, stop rules and tie rule (lowest feature, then lowest position, among equal computed scores), as tests/gbt_numpy.py restates the
log-loss fit.  What the loss changes: g = y - raw, a node's value is sum g / m in leaves and split nodes alike (nothing is summed beside g
and g^2), the stage score is the mean of (y - raw)^2, init is np.average(y).  Its sums run in numpy's order, not the kernels', so its trees
need not equal the GPU's bit for bit; like any fit it is judged by tests/gbr_replay.py.  ``fit`` returns (trees, init, predictions of the
training rows after every stage [T, n], train scores [T])."""
import numpy as np

EMPTY, ACTIVE, LEAF = 0, 1, 2
EPSILON = 2.220446049250313e-16


def fit(X, y, T, lr, D, mss, msl):
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    y = np.asarray(y, dtype=np.float64)
    n, d = X32.shape
    XT = X32.T.copy()
    order0 = np.argsort(XT, axis=1, kind="stable").astype(np.int32)
    init = float(np.average(y))
    raw = np.full(n, init)
    g = y - raw
    cap = (2 << D) - 1
    out = dict(left=[], right=[], feature=[], threshold=[], value=[], n_node_samples=[], root=[0])
    scores, stages = [], []
    for t in range(T):
        left, right = np.full(cap, -9), np.full(cap, -9)
        feat, thr, val, nns = np.zeros(cap, int), np.zeros(cap), np.zeros(cap), np.zeros(cap, int)
        key, order, n_nodes, level = np.zeros(n, int), order0.copy(), 1, 0
        tab = dict(start=[0], cnt=[n], node=[0], flag=[ACTIVE], sg=[0.0])
        while True:
            nk, active = 1 << level, 0
            # stats: the new nodes' sums in feature 0's order, their value, the stop rules
            for k in range(nk):
                if tab["flag"][k] != ACTIVE:
                    continue
                s, m = tab["start"][k], tab["cnt"][k]
                rows = order[0][s:s + m]
                sg, sq = g[rows].sum(), (g[rows] ** 2).sum()
                mean = sg / m
                impurity = sq / m - mean * mean
                node = tab["node"][k]
                tab["sg"][k], nns[node], val[node] = sg, m, mean
                if level >= D or m < mss or m < 2 * msl or impurity <= EPSILON:
                    tab["flag"][k] = LEAF
                    left[node] = right[node] = -1
                    thr[node] = -2.0
                else:
                    active += 1
            if active == 0:
                break
            # split: per node the best (score, feature, position); a later feature or position must score strictly higher
            cand = {}
            for f in range(d):
                o = order[f]
                kk = key[o]
                for k in range(nk):
                    if tab["flag"][k] != ACTIVE:
                        continue
                    s, m = tab["start"][k], tab["cnt"][k]
                    assert (kk[s:s + m] == k).all()
                    rows = o[s:s + m]
                    fv, cs = XT[f][rows], np.cumsum(g[rows])
                    best = None
                    for p in range(1, m):
                        if fv[p] > np.float32(fv[p - 1] + np.float32(1e-7)) and p >= msl and m - p >= msl:
                            sl = cs[p - 1]
                            sr = tab["sg"][k] - sl
                            diff = (m - p) * sl - p * sr
                            sc = diff * diff / (p * (m - p))
                            if best is None or sc > best[0]:
                                best = (sc, s + p)
                    if best is not None and (k not in cand or best[0] > cand[k][0]):
                        cand[k] = (best[0], f, best[1])
            # choose: thresholds, children, the next level's table; a node without a valid split stays the leaf stats valued
            nxt = dict(start=[0] * (2 * nk), cnt=[0] * (2 * nk), node=[0] * (2 * nk), flag=[EMPTY] * (2 * nk), sg=[0.0] * (2 * nk))
            split, rank, nleft = {}, 0, [0] * nk
            for k in range(nk):
                s, m, node, flag = tab["start"][k], tab["cnt"][k], tab["node"][k], tab["flag"][k]
                if flag == ACTIVE and k in cand:
                    _, f, bp = cand[k]
                    a, b = XT[f][order[f][bp - 1]], XT[f][order[f][bp]]
                    th = np.float64(a) / 2.0 + np.float64(b) / 2.0
                    if th == np.float64(b):
                        th = np.float64(a)
                    nl, lc = bp - s, n_nodes + 2 * rank
                    rank += 1
                    left[node], right[node], feat[node], thr[node], split[k], nleft[k] = lc, lc + 1, f, th, (f, th), nl
                    for j, (ss, cc, nn) in enumerate(((s, nl, lc), (s + nl, m - nl, lc + 1))):
                        nxt["start"][2 * k + j], nxt["cnt"][2 * k + j], nxt["node"][2 * k + j], nxt["flag"][2 * k + j] = ss, cc, nn, ACTIVE
                else:
                    if flag == ACTIVE:
                        left[node] = right[node] = -1
                        thr[node] = -2.0
                    nleft[k] = 0 if flag == EMPTY else m
                    nxt["start"][2 * k], nxt["cnt"][2 * k], nxt["node"][2 * k], nxt["flag"][2 * k] = s, m, node, EMPTY if flag == EMPTY else LEAF
                    nxt["start"][2 * k + 1] = s + m
            n_nodes += 2 * rank
            lbase = np.concatenate([[0], np.cumsum(nleft)[:-1]])
            # side: every row's key at the next level
            newkey = key.copy()
            for i in range(n):
                k, side = key[i], 0
                if k in split:
                    side = 0 if np.float64(XT[split[k][0]][i]) <= split[k][1] else 1
                newkey[i] = 2 * k + side
            # partition: every feature's order, stably, by the new key's last bit inside each segment
            neworder = np.full_like(order, -1)
            for f in range(d):
                lefts = 0
                for p in range(n):
                    i = order[f][p]
                    k, isleft = newkey[i] >> 1, not (newkey[i] & 1)
                    inseg, s = lefts - lbase[k], tab["start"][k]
                    to = s + inseg if isleft else s + nleft[k] + (p - s - inseg)
                    assert neworder[f][to] == -1
                    neworder[f][to] = i
                    lefts += isleft
            order, key, tab, level = neworder, newkey, nxt, level + 1
        # update: raw += lr * value[leaf] (product and sum rounded separately), the stage score, the next residuals
        raw = raw + lr * val[np.array(tab["node"])[key]]
        stages.append(raw.copy())
        g = y - raw
        scores.append((g * g).sum() / n)
        off = out["root"][-1]
        out["left"].append(np.where(left[:n_nodes] >= 0, left[:n_nodes] + off, -1))
        out["right"].append(np.where(right[:n_nodes] >= 0, right[:n_nodes] + off, -1))
        for name, arr in (("feature", feat), ("threshold", thr), ("value", val), ("n_node_samples", nns)):
            out[name].append(arr[:n_nodes])
        out["root"].append(off + n_nodes)
    trees = {k: (np.concatenate(v) if k != "root" else np.array(v)) for k, v in out.items()}
    return trees, init, np.array(stages), np.array(scores)
