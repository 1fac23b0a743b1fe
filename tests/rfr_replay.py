"""CPU replay of regression trees: certifies a fitted RandomForestRegressor / DecisionTreeRegressor (ours or scikit-learn's) node by node, in
exact arithmetic on the targets it is given.

Every float64 target is a dyadic rational, so the targets are scaled to Python integers once and a node's W = sum w, S = sum w y and a
candidate's score S_L^2 / W_L + S_R^2 / W_R are exact (``fractions.Fraction``).  ``replay`` raises ``ReplayError(check, ...)`` with ``check``

``stop``       a leaf that no stop rule allows, or a split node that a stop rule forbids
``samples``    a wrong ``n_node_samples`` or ``value`` (the weighted mean of the node's targets)
``valid``      a (feature, threshold) that is no valid position: values not more than 1e-7f apart, a side below ``min_samples_leaf``, or a
               threshold that is not the midpoint rule applied to the two float32 neighbours
``draw``       a split on a feature outside the node's draw (only when the draw is known: a seed was given)
``optimal``    a chosen position whose exact score, with the allowance below, is under the maximum over the candidates
``tie``        (this project's trees only) a position that is not the lowest feature, then the lowest position, among the positions whose
               float64 score is bit-equal to the largest float64 score

The allowance of ``optimal`` for this project's trees (``own=True``; y must lie on the grid ``quantum`` Z, which makes the sums that the fit
forms exact int64).  The fit computes fl(fl(fl(S_L) fl(S_L)) / W_L) + fl(fl(fl(S_R) fl(S_R)) / W_R), the sum rounded once more: seven
roundings in all (the weights are below 2^13 and convert exactly).  With U = 2^-53 each term carries at most (1 + U)^2 from the conversion,
which enters squared, (1 + U) from the product and (1 + U) from the division; both terms are non-negative, so the rounded sum lies within
exact (1 -+ U)^5.  The chosen position's computed score is at least every other's, hence exact(chosen) (1 + U)^5 >= exact(k) (1 - U)^5
for every candidate k.  Seven roundings, counted generously as eight: the check demands exact(chosen) (1 + 8U) >= max_k exact(k) (1 - 8U),
which the inequality above implies.  Nothing here is fitted to a fit's output.

For other implementations' trees (scikit-learn's) the sums themselves are accumulated in float64.  Higham's bound for a recursive sum of m
terms is (m - 1) U sum |w y|; scikit-learn's right-hand sum is the node's total minus the left-hand sum, two such errors.  With
D = 2 (m - 1) U sum_node |w y| a side's term S^2 / W moves by at most (2 |S| D + D^2) / W, and both sides' bounds are added to the
allowance of either score.  Their pure-node rule is ``impurity <= 2.2e-16`` on a float64 impurity: a leaf is accepted when the exact impurity is
at most 2.2e-16 plus that impurity's rounding (4 m U mean(y^2)), and a split of a node whose targets are all equal is accepted too (their
rounded impurity need not be 0 there).  ``value`` may differ from the exact mean by (m + 2) U mean |w y|.
"""
from fractions import Fraction

import numpy as np

import rf_numpy as N
import rfr_numpy as Q
from sklearn_trees import trees_of_sklearn  # noqa: F401  (``value`` is every node's mean)

U = Fraction(1, 2 ** 53)
EPSILON = Fraction(2.220446049250313e-16)


class ReplayError(AssertionError):
    def __init__(self, check, message):
        super().__init__(f"[{check}] {message}")
        self.check = check


def _exact_ints(y):
    """(Y, E): Python integers with y_i = Y_i 2^-E exactly."""
    mant, ex = np.frexp(y)
    mant = (mant * 2.0 ** 53).astype(np.int64)                # exact: 53 bits
    ex = ex.astype(np.int64) - 53
    low = int(ex[mant != 0].min()) if (mant != 0).any() else 0
    return np.array([int(a) << (int(b) - low) if a else 0 for a, b in zip(mant, ex)], dtype=object), -low


def _term(S, W):
    return Fraction(int(S) * int(S), int(W))


def replay(X, y, trees, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=None, weights=None, seed=None, bootstrap=True,
           own=False, quantum=None):
    """Replay every tree on its training data.  ``X`` [n, d] (cast to float32), ``y`` [n] float64 (for ``own`` the rounded targets, with
    ``quantum`` the grid's step ``y_quantum_``), ``trees`` the flat arrays.  Row weights per tree: ``weights`` [T, n] if given, else the
    hash's bootstrap of ``seed`` (ones without ``bootstrap``).  With a ``seed`` the drawn features of every node are recomputed from its path;
    without one every feature is a candidate.  Returns a dict of what was seen."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float64)
    n, d = X32.shape
    mf = N.resolve_max_features(max_features, d)
    depth_limit = N.UNLIMITED if max_depth is None else int(max_depth)
    Y, E = _exact_ints(y)
    unit = Fraction(1, 2 ** E) if E >= 0 else Fraction(2 ** -E)
    q = None
    if own:
        if quantum is None:
            raise ValueError("rfr_replay: own=True needs the grid's quantum")
        qf = y / quantum
        if not (np.array_equal(qf, np.rint(qf)) and np.abs(qf).max() <= 2.0 ** Q.TARGET_BITS):
            raise ReplayError("samples", "the targets are not on the grid")
        q = qf.astype(np.int64)
    left, right, feature, threshold, value = trees["left"], trees["right"], trees["feature"], trees["threshold"], trees["value"]
    nns, root = trees["n_node_samples"], trees["root"]
    seen = dict(nodes=0, splits=0, leaves=0, ties=0, max_depth=0, stop_reasons={})
    for t in range(len(root) - 1):
        if weights is not None:
            w = np.asarray(weights[t]).astype(np.int64)
        else:
            w = N.bootstrap_weights(seed, t, n) if (bootstrap and seed is not None) else np.ones(n, dtype=np.int64)
        wo = w.astype(object)
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
            wY = wo[rows] * Y[rows]
            W, S, A = int(w[rows].sum()), int(wY.sum()), int(np.abs(wY).sum())
            mean = Fraction(S, W) * unit
            if own:
                want = np.ldexp(np.float64(int((w[rows] * q[rows]).sum())) / np.float64(W), int(np.log2(quantum)))
                if np.float64(value[node]).tobytes() != np.float64(want).tobytes():
                    raise ReplayError("samples", f"{where}: value {float(value[node])!r}, fl(S) / fl(W) on the grid gives {float(want)!r}")
            elif abs(Fraction(float(value[node])) - mean) > (m + 2) * U * Fraction(A, W) * unit:
                raise ReplayError("samples", f"{where}: value {float(value[node])!r}, the weighted mean is {float(mean)!r}")
            Xn = X32[rows]
            constant = int(Y[rows].min()) == int(Y[rows].max())
            forbidden = ("depth" if depth >= depth_limit else "min_samples_split" if m < min_samples_split else
                         "min_samples_leaf" if m < 2 * min_samples_leaf else "pure" if constant and own else None)
            cands = {}                                                          # feature -> (fv, positions, W_L, S_L) with S_L exact
            if forbidden is None:
                drawn = N.draw_features(key, Xn, mf) if key is not None else np.nonzero(N.non_constant(Xn))[0]
                for f in drawn:
                    o = np.argsort(Xn[:, f], kind="stable")
                    fv = Xn[o, f]
                    p, WL, _ = Q.position_sums(fv, w[rows][o], w[rows][o], min_samples_leaf)
                    if len(p):
                        cands[int(f)] = (fv, p, WL, np.cumsum(wY[o])[p - 1], o)
            if left[node] < 0:                                                  # ---- a leaf: which rule allows it?
                if right[node] >= 0:
                    raise ReplayError("stop", f"{where}: a left child only")
                reason = forbidden if forbidden is not None else ("no valid split" if not cands else None)
                if reason is None and not own:
                    sq = Fraction(int((wo[rows] * Y[rows] * Y[rows]).sum()), W) * unit * unit
                    if constant or sq - mean * mean <= EPSILON + 4 * m * U * sq:
                        reason = "pure"
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
            fv = cands[f][0]
            want_thr = N.midpoint(fv[p - 1], fv[p])
            if thr.tobytes() != np.float64(want_thr).tobytes():
                raise ReplayError("valid", f"{where}: threshold {thr!r}, the midpoint rule between {fv[p - 1]!r} and {fv[p]!r} gives {want_thr!r}")

            def exact(g, j):
                _, _, WL, SL, _ = cands[g]
                return _term(SL[j], WL[j]) + _term(S - int(SL[j]), W - int(WL[j]))

            def allowance(g, j):
                """What a float64 fit may add to or take from this candidate's exact score."""
                e = exact(g, j)
                if own:
                    return 8 * U * e
                _, _, WL, SL, _ = cands[g]
                D = 2 * (m - 1) * U * A
                return 8 * U * e + (2 * abs(int(SL[j])) * D + D * D) / int(WL[j]) + (2 * abs(S - int(SL[j])) * D + D * D) / (W - int(WL[j]))

            j = int(np.nonzero(cands[f][1] == p)[0][0])
            chosen = exact(f, j) + allowance(f, j)
            # the exact maximum: only positions whose float64 score is within 1e-9 of the largest can hold it (a score computed from exact
            # sums errs by a few 2^-53), or -- with another implementation's allowance -- come close to it
            approx = {}
            for g in sorted(cands):
                _, _, WL, SL, _ = cands[g]
                sl, sr = SL.astype(np.float64), (S - SL).astype(np.float64)
                approx[g] = sl * sl / WL.astype(np.float64) + sr * sr / (W - WL).astype(np.float64)
            peak = max(float(a.max()) for a in approx.values())
            for g in sorted(cands):
                for k in np.nonzero(approx[g] >= peak - abs(peak) * 1e-9)[0]:
                    other = exact(g, int(k)) - allowance(g, int(k))
                    if chosen < other:
                        raise ReplayError("optimal", f"{where}: feature {f} position {p} scores {float(exact(f, j) * unit * unit):.17g}, feature {g} "
                                                     f"position {int(cands[g][1][k])} reaches {float(exact(g, int(k)) * unit * unit):.17g}: more than the "
                                                     "roundings of a float64 fit allow")
            if own:                                                             # the tie rule, on the float64 scores the fit itself forms
                wq = w[rows] * q[rows]
                Sq = int(wq.sum())
                top, at_top = -1.0, []
                for g in sorted(cands):
                    _, gp, WL, _, o = cands[g]
                    score = Q.scores(WL, np.cumsum(wq[o])[gp - 1], W, Sq)
                    if score.max() > top:
                        top, at_top = float(score.max()), []
                    if score.max() == top:
                        at_top += [(g, int(gp[k])) for k in np.nonzero(score == top)[0]]
                seen["ties"] += int(len(at_top) > 1)
                if (f, p) != min(at_top):
                    raise ReplayError("tie", f"{where}: feature {f} position {p}; the largest float64 score {top!r} is at {at_top[:4]}, the rule "
                                             f"takes feature {min(at_top)[0]} position {min(at_top)[1]}")
            stack.append((int(right[node]), rows[~goes_left], depth + 1, N.child_key(key, 1) if key is not None else None))
            stack.append((int(left[node]), rows[goes_left], depth + 1, N.child_key(key, 0) if key is not None else None))
        if visited != hi - lo:
            raise ReplayError("stop", f"tree {t}: {hi - lo} nodes stored, {visited} reached from the root")
    return seen


def bootstrap_weights_of_sklearn(forest, n):
    """The integer row weights of every tree of a fitted scikit-learn forest (its bootstrap, regenerated from each tree's random_state)."""
    from sklearn.ensemble._forest import _generate_sample_indices
    return [np.bincount(_generate_sample_indices(est.random_state, n, n), minlength=n).astype(np.int64) for est in forest.estimators_]
