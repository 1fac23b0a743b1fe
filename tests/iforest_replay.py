"""CPU replay of isolation trees: certifies the flat trees of an ``IsolationForest`` (ours or scikit-learn's) node by node on each tree's own
sub-sample, without the hash -- two correct fits of one problem have different trees, so a fit is certified instead of compared.
``replay`` raises ``ReplayError(check, ...)`` with ``check`` one of

``sample``     a tree's rows are not distinct rows of X, or not ``max_samples`` of them
``samples``    a wrong ``n_node_samples``
``stop``       a leaf that no rule allows (two rows or more above the depth limit with a feature that is not constant), or a split that a rule
               forbids (fewer than two rows, the depth limit, every feature constant); also a tree whose nodes are not all reached
``valid``      a split feature that is constant on the node's rows, or a threshold outside [lo, hi) of that feature
``draw``       (only with a ``seed``) the rows, the feature or the threshold differ from what the hash draws

For scikit-learn's own trees pass ``own=False`` and no seed: its further stop on the impurity of the random target makes leaves that no rule
here allows, so the leaf half of ``stop`` is left out, and its random stream is not the hash.
"""
import numpy as np

import iforest_numpy as N


class ReplayError(AssertionError):
    def __init__(self, check, message):
        super().__init__(f"[{check}] {message}")
        self.check = check


def samples_of_sklearn(fitted):
    """The rows of every tree of a fitted scikit-learn IsolationForest, [T, max_samples_]."""
    return np.stack([np.asarray(s) for s in fitted.estimators_samples_])


def replay(X, trees, samples, max_samples, *, seed=None, own=True):
    """Replay every tree on its rows.  ``X`` [n, d] (cast to float32), ``trees`` the flat arrays (left, right, feature, threshold,
    n_node_samples, root), ``samples`` [T, max_samples] row indices.  Returns a dict of what was seen."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X32.shape
    left, right, feature, threshold, nns, root = (trees[k] for k in ("left", "right", "feature", "threshold", "n_node_samples", "root"))
    max_depth = int(np.ceil(np.log2(max(max_samples, 2))))
    seen = dict(nodes=0, splits=0, leaves=0, redraws=0, max_depth=0, stop_reasons={})
    if len(samples) != len(root) - 1:
        raise ReplayError("sample", f"{len(samples)} row sets for {len(root) - 1} trees")
    for t in range(len(root) - 1):
        rows = np.asarray(samples[t]).astype(np.int64)
        if len(rows) != max_samples or len(np.unique(rows)) != len(rows) or rows.min() < 0 or rows.max() >= n:
            raise ReplayError("sample", f"tree {t}: {len(rows)} rows, {len(np.unique(rows))} distinct, max_samples {max_samples}")
        if seed is not None and not np.array_equal(rows, N.sample_rows(seed, t, n, max_samples)):
            raise ReplayError("draw", f"tree {t}: the rows are not the hash's sub-sample in ascending order")
        lo_node, hi_node = int(root[t]), int(root[t + 1])
        visited = 0
        stack = [(lo_node, rows, 0, N.tree_key(seed, t) if seed is not None else None)]
        while stack:
            node, rws, depth, key = stack.pop()
            m = len(rws)
            where = f"tree {t} node {node - lo_node} (depth {depth}, {m} rows)"
            if not lo_node <= node < hi_node:
                raise ReplayError("stop", f"{where}: node index outside its tree")
            visited += 1
            seen["nodes"] += 1
            seen["max_depth"] = max(seen["max_depth"], depth)
            if int(nns[node]) != m:
                raise ReplayError("samples", f"{where}: n_node_samples {int(nns[node])}, the replay routes {m} rows here")
            Xn = X32[rws]
            if m:
                lo, hi = Xn.min(axis=0), Xn.max(axis=0)
                nc = hi > (lo + np.float32(1e-7)).astype(np.float32)
            else:
                nc = np.zeros(d, dtype=bool)
            reason = "rows" if m < 2 else "depth" if depth >= max_depth else "constant" if not nc.any() else None
            if left[node] < 0:
                if right[node] >= 0:
                    raise ReplayError("stop", f"{where}: one child only")
                if reason is None:
                    if own:
                        raise ReplayError("stop", f"{where}: a leaf, but no stop rule holds")
                    reason = "other"
                seen["leaves"] += 1
                seen["stop_reasons"][reason] = seen["stop_reasons"].get(reason, 0) + 1
                continue
            if reason is not None:
                raise ReplayError("stop", f"{where}: a split node, but the stop rule '{reason}' holds")
            f, thr = int(feature[node]), float(threshold[node])
            if not 0 <= f < d or not nc[f]:
                raise ReplayError("valid", f"{where}: split on feature {f}, which is constant on the node's rows")
            if not float(lo[f]) <= thr < float(hi[f]):
                raise ReplayError("valid", f"{where}: threshold {thr!r} outside [{float(lo[f])!r}, {float(hi[f])!r})")
            if key is not None:
                order = N.feature_order(key, d)
                want_f = next(int(g) for g in order if nc[g])
                seen["redraws"] += int(np.nonzero(order == want_f)[0][0])
                if f != want_f:
                    raise ReplayError("draw", f"{where}: split on feature {f}, the hash draws {want_f}")
                want_thr = N.draw_threshold(key, lo[f], hi[f])
                if thr != float(want_thr):
                    raise ReplayError("draw", f"{where}: threshold {thr!r}, the hash draws {float(want_thr)!r}")
            seen["splits"] += 1
            goes = Xn[:, f].astype(np.float64) <= thr
            stack.append((int(right[node]), rws[~goes], depth + 1, None if key is None else N.child_key(key, 1)))
            stack.append((int(left[node]), rws[goes], depth + 1, None if key is None else N.child_key(key, 0)))
        if visited != hi_node - lo_node:
            raise ReplayError("stop", f"tree {t}: {hi_node - lo_node} nodes, the replay reaches {visited}")
    return seen
