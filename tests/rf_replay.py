"""CPU replay of forest trees: certifies a fitted RandomForestClassifier / DecisionTreeClassifier (ours or scikit-learn's) node by node.

Many nodes have several split candidates whose scores tie exactly (scikit-learn breaks such ties by its random feature order), so two
correct fits of one problem have different trees and a fit is certified instead of compared.  With integer row weights every quantity is
exact: a candidate's score is the fraction (W_R L_1 - W_L R_1)^2 / (W_L W_R), compared as ``fractions.Fraction`` with no allowance.
``replay`` raises ``ReplayError(check, ...)`` with ``check`` one of

``stop``       a leaf that no stop rule allows, or a split node that a stop rule forbids
``samples``    a wrong ``n_node_samples`` or ``value`` (the weighted class-1 share)
``valid``      a (feature, threshold) that is no valid position: values not more than 1e-7f apart, a side below ``min_samples_leaf``, or a
               threshold that is not the midpoint rule applied to the two float32 neighbours
``draw``       a split on a feature outside the node's draw (only when the draw is known: a seed was given)
``optimal``    a chosen position whose exact score is below the maximum over the candidate features' valid positions
``tie``        (this project's trees only) a position that maximises the score but is not the lowest feature, then the lowest position, among
               the positions whose float64 score equals the maximum's

The pure rule: scikit-learn stops at ``impurity <= 2.2e-16``; with integer weights W <= 8192 the Gini impurity is 0 for a pure node and
at least (2 W - 2) / W^2 > 2.4e-4 for any other, so the rule is ``W_1 in {0, W}``.
"""
from fractions import Fraction

import numpy as np

import rf_numpy as N
from sklearn_trees import trees_of_sklearn  # noqa: F401  (``value`` is the class-1 share of every node)


class ReplayError(AssertionError):
    def __init__(self, check, message):
        super().__init__(f"[{check}] {message}")
        self.check = check


def replay(X, y, trees, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=None, weights=None, seed=None, bootstrap=True,
           own=False):
    """Replay every tree on its training data.  ``X`` [n, d] (cast to float32), ``y`` [n] in {0, 1}, ``trees`` the flat arrays (left, right,
    feature, threshold, value, n_node_samples, root).  Row weights per tree: ``weights`` [T, n] if given, else the hash's bootstrap of
    ``seed`` (ones without ``bootstrap``).  With a ``seed`` the drawn features of every node are recomputed from its path; without one every
    feature is a candidate.  ``own``: also hold the tree to the tie rule.  Returns a dict of what was seen."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    n, d = X32.shape
    mf = N.resolve_max_features(max_features, d)
    depth_limit = N.UNLIMITED if max_depth is None else int(max_depth)
    left, right, feature, threshold, value = trees["left"], trees["right"], trees["feature"], trees["threshold"], trees["value"]
    nns, root = trees["n_node_samples"], trees["root"]
    seen = dict(nodes=0, splits=0, leaves=0, ties=0, max_depth=0, stop_reasons={})
    for t in range(len(root) - 1):
        if weights is not None:
            w = np.asarray(weights[t]).astype(np.int64)
        else:
            w = N.bootstrap_weights(seed, t, n) if (bootstrap and seed is not None) else np.ones(n, dtype=np.int64)
        w1 = w * y
        lo, hi = int(root[t]), int(root[t + 1])
        visited = 0
        stack = [(lo, np.nonzero(w > 0)[0], 0, N.tree_key(seed, t) if seed is not None else None)]
        while stack:
            node, rows, depth, key = stack.pop()
            m = len(rows)
            where = f"tree {t} node {node - lo} (depth {depth}, {m} rows)"
            if not lo <= node < hi:
                raise ReplayError("stop", f"{where}: node index outside its tree")
            visited += 1
            seen["nodes"] += 1
            seen["max_depth"] = max(seen["max_depth"], depth)
            if m == 0:
                raise ReplayError("stop", f"{where}: an empty node")
            if int(nns[node]) != m:
                raise ReplayError("samples", f"{where}: n_node_samples {int(nns[node])}, the replay routes {m} distinct rows here")
            W, W1 = int(w[rows].sum()), int(w1[rows].sum())
            want = np.float64(W1) / np.float64(W)
            if np.float64(value[node]).tobytes() != want.tobytes():
                raise ReplayError("samples", f"{where}: value {float(value[node])!r}, the weighted class-1 share is {W1}/{W} = {float(want)!r}")
            Xn = X32[rows]
            forbidden = ("depth" if depth >= depth_limit else "min_samples_split" if m < min_samples_split else
                         "min_samples_leaf" if m < 2 * min_samples_leaf else "pure" if W1 in (0, W) else None)
            cands = {}                                                          # feature -> (fv, positions, numerators, denominators)
            if forbidden is None:
                drawn = N.draw_features(key, Xn, mf) if key is not None else np.nonzero(N.non_constant(Xn))[0]
                for f in drawn:
                    o = np.argsort(Xn[:, f], kind="stable")
                    fv = Xn[o, f]
                    p, num, den = N.position_scores(fv, w[rows][o], w1[rows][o], min_samples_leaf)
                    if len(p):
                        cands[int(f)] = (fv, p, num, den)
            if left[node] < 0:                                                  # ---- a leaf: which rule allows it?
                if right[node] >= 0:
                    raise ReplayError("stop", f"{where}: a left child only")
                reason = forbidden if forbidden is not None else ("no valid split" if not cands else None)
                if reason is None:
                    raise ReplayError("stop", f"{where}: a leaf, but no stop rule holds and a drawn feature has a valid position")
                seen["stop_reasons"][reason] = seen["stop_reasons"].get(reason, 0) + 1
                seen["leaves"] += 1
                continue
            # ---- a split node
            seen["splits"] += 1
            if right[node] < 0:
                raise ReplayError("stop", f"{where}: a right child is missing")
            if forbidden is not None:
                raise ReplayError("stop", f"{where}: split although the {forbidden} rule makes it a leaf")
            f, thr = int(feature[node]), np.float64(threshold[node])
            if not 0 <= f < d:
                raise ReplayError("valid", f"{where}: feature {f} outside 0..{d - 1}")
            goes_left = Xn[:, f].astype(np.float64) <= thr
            p = int(goes_left.sum())
            if key is not None and f not in set(int(g) for g in drawn):
                raise ReplayError("draw", f"{where}: feature {f} is not among the node's drawn features {[int(g) for g in drawn]}")
            if f not in cands or p not in cands[f][1]:
                raise ReplayError("valid", f"{where}: feature {f} threshold {thr!r} puts {p} of {m} rows left: not a valid split position")
            fv, pos, num, den = cands[f]
            want_thr = N.midpoint(fv[p - 1], fv[p])
            if thr.tobytes() != np.float64(want_thr).tobytes():
                raise ReplayError("valid", f"{where}: threshold {thr!r}, the midpoint rule between {fv[p - 1]!r} and {fv[p]!r} gives {want_thr!r}")
            j = int(np.nonzero(pos == p)[0][0])
            chosen = Fraction(int(num[j]), int(den[j]))
            # the exact maximum: only positions whose float64 score is within 1e-12 of the largest can hold it (one division errs by 2^-53)
            top, top_double, at_top = None, -1.0, []
            for g in sorted(cands):
                _, gp, gnum, gden = cands[g]
                score = gnum.astype(np.float64) / gden.astype(np.float64)
                for q in np.nonzero(score >= score.max() * (1 - 1e-12))[0]:
                    fr = Fraction(int(gnum[q]), int(gden[q]))
                    if top is None or fr > top:
                        top = fr
                if score.max() > top_double:
                    top_double, at_top = float(score.max()), []
                if score.max() == top_double:
                    at_top += [(g, int(gp[q])) for q in np.nonzero(score == top_double)[0]]
            if chosen != top:
                raise ReplayError("optimal", f"{where}: feature {f} position {p} scores {float(chosen):.17g} = {chosen}, another valid candidate "
                                             f"reaches {float(top):.17g} = {top}")
            seen["ties"] += int(len(at_top) > 1)
            if own and (f, p) != min(at_top):
                raise ReplayError("tie", f"{where}: feature {f} position {p} ties for the maximum, the rule takes feature {min(at_top)[0]} "
                                         f"position {min(at_top)[1]}")
            stack.append((int(right[node]), rows[~goes_left], depth + 1, N.child_key(key, 1) if key is not None else None))
            stack.append((int(left[node]), rows[goes_left], depth + 1, N.child_key(key, 0) if key is not None else None))
        if visited != hi - lo:
            raise ReplayError("stop", f"tree {t}: {hi - lo} nodes stored, {visited} reached from the root")
    return seen
