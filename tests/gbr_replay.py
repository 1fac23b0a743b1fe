"""CPU replay of a squared-error boosted chain: certifies a fitted GradientBoostingRegressor (ours or scikit-learn's) node by node and
stage by stage, the way ``gbt_replay`` certifies the classifier.

Two correct fits of one problem may break ties differently, so a fit is not compared with another fit; every decision it took is checked
against the data in extended precision (``np.longdouble``) with allowances for what float64 rounding can change.  ``replay`` raises
``ReplayError(check, ...)`` with the same named checks:

``stop``       a leaf that no stop rule allows, or a split node that a stop rule forbids
``optimal``    a split that is not a valid candidate, or whose score is below the best valid candidate's by more than rounding explains
``threshold``  a threshold that is not the midpoint rule applied to the two float32 neighbours, or a wrong ``n_node_samples``
``leaf``       a node value (leaf or split node) away from sum g / m
``raw``        raw scores or ``train_score_`` that are not what the model's own trees give

Notation as in ``gbt_replay``: U = 2^-53; a node has m rows, residuals g_i = y_i - raw_i from the raw scores *the model's own earlier trees
give*, A = sum |g_i|, G = max |g_i|.  A float64 sum of m terms t_i in any order is within (m - 1) U sum |t_i| of the exact sum (Higham, eq.
4.4 to first order; products of U^2 are covered by rounding every constant up).

* residuals.  y_i and raw_i are float64 numbers; the fit's residual is their float64 difference: one rounding, so it is within
  D_i = U |g_i| of the exact g_i (the extended-precision difference itself is off by at most 2^-64 |g_i|, 2 000 times less).  D = sum of D_i.
* impurity = sum g^2 / m - (sum g / m)^2: ``gbt_replay``'s derivation word for word, with this D_i.  Allowance (3 m + 6) U G^2 + 4 G max D_i.
  A leaf is accepted by the impurity rule when impurity <= 2.2e-16 + allowance; a split node must have impurity > 2.2e-16 - allowance.
* score(f, p) = (n_r S_l - n_l S_r)^2 / (n_l n_r): ``gbt_replay._scores`` with this D (E = (2 m + 4) m U A + 2 m D; allowance
  (2 |diff| E + E^2) / (n_l n_r) + 4 U score, per candidate).  The chosen candidate c must satisfy score_x(c) + allow(c) >= max over valid
  candidates k of (score_x(k) - allow(k)).
* node value v = sum g / m, in leaves and split nodes alike (scikit-learn skips ``_update_terminal_regions`` for the squared error, so
  the tree's own node mean is the update).  The sum is within (m - 1) U A + D <= m U A + D of the exact one; the division adds U |v| <=
  U A / m.  Allowance: ((m + 1) U A + D) / m.
* raw scores: raw += learning_rate * value[leaf] is two IEEE operations, replayed exactly in float64 from the model's own trees; a fused
  multiply-add would differ by one rounding per stage, so the allowance after s stages is s U max(|raw|, 1).
* train_score_ = mean of (y - raw)^2.  A term: the difference carries U, its square 2 U + U for the product, so 3 U to first order; the sum
  of n non-negative terms (n - 1) U; the division U: (n + 3) U relative.  The raw scores may be off by their allowance a, which moves the
  mean of squares by at most 2 max |y - raw| a (+ a^2, below U a).  Allowance: (n + 3) U mean + 2 max |y - raw| a.

No constant here was fitted to any implementation's output.
"""
import numpy as np

from gbt_replay import ReplayError, _scores, candidates, midpoint
import sklearn_trees

U = 2.0 ** -53
LD = np.longdouble
EPSILON = float(np.finfo(np.float64).eps)


def residuals_x(y, raw):
    """(g, D): y - raw in extended precision and the bound on a float64 fit's residuals' distance from it."""
    g = y.astype(LD) - raw.astype(LD)
    return g, (U * np.abs(g)).astype(LD)


def replay(X, y, trees, init, learning_rate, max_depth, min_samples_split=2, min_samples_leaf=1, raw_stages=None, train_score=None):
    """Replay the chain on its training data.  ``X`` [n, d] (cast to float32), ``y`` [n] float64, ``trees`` the flat arrays (left, right,
    feature, threshold, value, n_node_samples, root); ``raw_stages`` [T, n] the model's predictions of the training rows after every stage
    and ``train_score`` [T], both optional.  Returns a dict of what was seen (counts, the largest used share of each allowance)."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    y = np.asarray(y, dtype=np.float64)
    n, d = X32.shape
    left, right, feature, threshold, value = trees["left"], trees["right"], trees["feature"], trees["threshold"], trees["value"]
    nns, root = trees["n_node_samples"], trees["root"]
    T = len(root) - 1
    raw = np.full(n, np.float64(init))
    seen = dict(nodes=0, splits=0, leaves=0, ties=0, zero_best=0, leaf_share=0.0, optimal_margin=np.inf, stop_reasons={})
    for t in range(T):
        g, D = residuals_x(y, raw)
        stack = [(int(root[t]), np.arange(n), 0)]
        leaf_of = np.empty(n, dtype=np.int64)
        while stack:
            node, rows, depth = stack.pop()
            where = f"tree {t} node {node - int(root[t])} (depth {depth}, {len(rows)} rows)"
            if not (int(root[t]) <= node < int(root[t + 1])):
                raise ReplayError("stop", f"{where}: node index outside its tree")
            m = len(rows)
            seen["nodes"] += 1
            if int(nns[node]) != m:
                raise ReplayError("threshold", f"{where}: n_node_samples {int(nns[node])}, the replay routes {m} rows here")
            if m == 0:
                raise ReplayError("stop", f"{where}: an empty node")
            gn, Dn = g[rows], D[rows]
            G, A, Dsum = float(np.abs(gn).max()), np.abs(gn).sum(), Dn.sum()
            mean = gn.sum() / m
            impurity = float((gn * gn).sum() / m - mean * mean)
            imp_allow = (3 * m + 6) * U * G * G + 4 * G * float(Dn.max())
            # the node's value: sum g / m, whether it is a leaf or not
            val_allow = float(((m + 1) * U * A + Dsum) / m)
            err = abs(float(value[node]) - float(mean))
            if not err <= val_allow:
                raise ReplayError("leaf", f"{where}: value {float(value[node])!r}, sum g / m = {float(mean)!r}: off by {err:.3e}, allowance {val_allow:.3e}")
            if val_allow > 0:
                seen["leaf_share"] = max(seen["leaf_share"], err / val_allow)
            # the best valid candidate of every feature, in extended precision
            best_lo, any_valid, per_feature = -np.inf, False, {}
            if depth < max_depth and m >= 2:
                for f in range(d):
                    o = np.argsort(X32[rows, f], kind="stable")
                    fv = X32[rows, f][o]
                    pos = candidates(fv, min_samples_leaf)
                    if len(pos):
                        any_valid = True
                        score, allow = _scores(gn[o], Dsum, pos)
                        per_feature[f] = (fv, pos, score, allow)
                        best_lo = max(best_lo, float((score - allow).max()))
            if left[node] < 0:                                                  # ---- a leaf: which rule allows it?
                if right[node] >= 0:
                    raise ReplayError("stop", f"{where}: a left child only")
                reason = ("depth" if depth >= max_depth else "min_samples_split" if m < min_samples_split else
                          "min_samples_leaf" if m < 2 * min_samples_leaf else "impurity" if impurity <= EPSILON + imp_allow else
                          "no valid split" if not any_valid else None)
                if reason is None:
                    raise ReplayError("stop", f"{where}: a leaf, but depth < {max_depth}, m >= min_samples_split = {min_samples_split}, m >= 2 "
                                              f"min_samples_leaf, impurity {impurity:.3e} > {EPSILON:.3e} + {imp_allow:.3e} and a valid split exists")
                seen["stop_reasons"][reason] = seen["stop_reasons"].get(reason, 0) + 1
                seen["leaves"] += 1
                leaf_of[rows] = node
                continue
            # ---- a split node
            seen["splits"] += 1
            if right[node] < 0:
                raise ReplayError("stop", f"{where}: a right child is missing")
            if depth >= max_depth:
                raise ReplayError("stop", f"{where}: split at depth {depth} >= max_depth {max_depth}")
            if m < min_samples_split:
                raise ReplayError("stop", f"{where}: split with {m} rows < min_samples_split {min_samples_split}")
            if m < 2 * min_samples_leaf:
                raise ReplayError("stop", f"{where}: split with {m} rows < 2 min_samples_leaf")
            if impurity <= EPSILON - imp_allow:
                raise ReplayError("stop", f"{where}: split although the impurity {impurity:.3e} <= {EPSILON:.3e} - {imp_allow:.3e}")
            f, thr = int(feature[node]), np.float64(threshold[node])
            if not 0 <= f < d:
                raise ReplayError("optimal", f"{where}: feature {f} outside 0..{d - 1}")
            goes_left = X32[rows, f].astype(np.float64) <= thr
            p = int(goes_left.sum())
            if f not in per_feature or p not in per_feature[f][1]:
                raise ReplayError("optimal", f"{where}: feature {f} threshold {thr!r} puts {p} of {m} rows left: not a valid split position")
            fv, pos, score, allow = per_feature[f]
            j = int(np.nonzero(pos == p)[0][0])
            want_thr = midpoint(fv[p - 1], fv[p])
            if thr.tobytes() != np.float64(want_thr).tobytes():
                raise ReplayError("threshold", f"{where}: threshold {thr!r}, the midpoint rule between {fv[p - 1]!r} and {fv[p]!r} gives {want_thr!r}")
            chosen_hi = float(score[j] + allow[j])
            if not chosen_hi >= best_lo:
                raise ReplayError("optimal", f"{where}: feature {f} position {p} scores {float(score[j]):.17g} (+ allowance {float(allow[j]):.3e}), "
                                             f"another valid candidate reaches {best_lo:.17g} after its allowance")
            top = max(float(v[2].max()) for v in per_feature.values())
            seen["optimal_margin"] = min(seen["optimal_margin"], chosen_hi - best_lo)
            seen["ties"] += int(sum(int((v[2] >= top).sum()) for v in per_feature.values()) > 1)
            seen["zero_best"] += int(top == 0)
            stack.append((int(right[node]), rows[~goes_left], depth + 1))
            stack.append((int(left[node]), rows[goes_left], depth + 1))
        # ---- the stage's update, with the model's own values: two float64 operations per row, replayed exactly
        step = np.float64(learning_rate) * value[leaf_of].astype(np.float64)
        raw = raw + step
        raw_allow = (t + 1) * U * max(float(np.abs(raw).max()), 1.0)
        if raw_stages is not None:
            err = float(np.abs(np.asarray(raw_stages[t], dtype=np.float64) - raw).max())
            if not err <= raw_allow:
                raise ReplayError("raw", f"stage {t}: the model's predictions are off the replay of its own trees by {err:.3e}, allowance {raw_allow:.3e}")
        if train_score is not None:
            r = y.astype(LD) - raw.astype(LD)
            want = (r * r).sum() / n
            allow = float((n + 3) * U * want + 2 * np.abs(r).max() * raw_allow)
            err = abs(float(train_score[t]) - float(want))
            if not err <= allow:
                raise ReplayError("raw", f"stage {t}: train_score_ {float(train_score[t])!r}, the mean square of the replayed residuals is {float(want)!r}: "
                                         f"off by {err:.3e}, allowance {allow:.3e}")
    seen["raw"] = raw
    return seen


def trees_of_sklearn(fitted):
    """A fitted scikit-learn GradientBoostingRegressor's trees in the flat convention, and its initial raw score (the targets' mean)."""
    return sklearn_trees.trees_of_sklearn(fitted), float(np.ravel(fitted.init_.constant_)[0])


def make_data(n, d, seed=1, variant=None):
    """A seeded regression problem on continuous features: a linear rule plus a bend in feature 0 plus noise.  Variants: "decimals"
    (features rounded to one decimal: real ties), "constant" (a constant column), "collide" (two float64 values that are one float32
    value), "flat" (y is one value wherever feature 0 > 0: an impurity leaf at depth 1 in the first tree), "constant_y"."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, d)
    w = rs.randn(d)
    y = X @ w + np.sin(2.0 * X[:, 0]) + 0.3 * rs.randn(n)
    if variant == "decimals":
        X = np.round(X, 1)
    elif variant == "constant":
        X[:, min(2, d - 1)] = 3.0
    elif variant == "collide":
        X[0, 0], X[1, 0] = 1.0, 1.0 + 1e-10
        y[0], y[1] = -2.0, 2.0
    elif variant == "flat":
        # small targets: the impurity any summation order computes for m equal residuals g is within 3 m U g^2 of 0, and with |g| < 0.1
        # and m < 257 that is below the floor 2.2e-16 the rule compares with, so the node is an impurity leaf for every correct fit
        y *= 0.01
        y[X[:, 0] > 0] = 0.1
    elif variant == "constant_y":
        y[:] = 1.5                       # a dyadic value: the mean of n copies is that value exactly, so every residual is exactly 0
    elif variant is not None:
        raise ValueError(variant)
    return X, y


# n, d, max_depth, min_samples_split, min_samples_leaf, learning_rate.  257 = one row more than the 256 positions the split and partition
# kernels scan per pass; 1025 = four passes and one row; depth 7 at n = 257: tiny nodes, branches that stop beside ones that go on
CONTINUOUS_CASES = [(2, 1, 1, 2, 1, 0.1), (64, 3, 3, 2, 1, 0.1), (65, 3, 3, 5, 1, 0.1), (257, 5, 7, 2, 1, 0.1), (257, 5, 3, 10, 3, 0.01), (1025, 3, 3, 2, 1, 0.1),
                    (257, 33, 3, 2, 3, 0.1), (257, 1, 7, 5, 1, 0.01), (257, 5, 1, 2, 1, 0.1)]
# (case, trees) on which training-row predictions are compared with scikit-learn's: every continuous case, the row limit among them
PARITY_CASES = [(c, 8) for c in CONTINUOUS_CASES] + [((8192, 2, 2, 2, 1, 0.1), 2)]
# (case, variant, trees): the continuous cases with eight trees, the row limit (and the largest LDS request) with two, and the variants
CASES = ([(c, None, 8) for c in CONTINUOUS_CASES] + [((8192, 2, 2, 2, 1, 0.1), None, 2)] +
         [((257, 5, 5, 2, 1, 0.1), "decimals", 8), ((257, 5, 7, 10, 3, 0.1), "decimals", 8), ((257, 5, 3, 2, 1, 0.1), "constant", 8),
          ((65, 3, 3, 2, 1, 0.1), "collide", 8), ((257, 5, 3, 2, 1, 0.1), "flat", 8), ((257, 5, 3, 2, 1, 0.1), "constant_y", 8)])


def parity_bound(y, staged, learning_rate, init):
    """The distance e_s two correct fits' training-row predictions may have after stage s, [T], when every node of both holds the same
    rows (on continuous features exact score ties arise only between candidates that induce the same partition), and the bound that
    gives for ``train_score_``.  ``staged`` [T, n] are one of the two fits' predictions.

    e_0 = 0: both start at the same ``init``.  In stage s both fit a tree to g = y - raw with raw off by e_(s-1) between them, so a node's
    values differ by e_(s-1) plus the rounding of either mean: the difference U max |g|, a sum of m <= n terms (m - 1) U max |g|, the
    division U max |g|, together at most (n + 2) U max |g| with both fits' roundings to first order absorbed by n >= m + 1.  The update
    raw += lr * value multiplies that by lr, keeps the old distance and rounds the product and the sum: U max(|raw|, 1).  Hence
    e_s <= (1 + lr) e_(s-1) + lr (n + 2) U max |g| + U max(|raw|, 1), with max |g| over the residuals stage s is fitted to and max |raw|
    over the predictions after it.  train_score_ = mean (y - raw)^2 then differs by at most 2 max |y - raw| e_s + e_s^2 from the
    predictions and 2 (n + 3) U mean from the two evaluations (see the module docstring)."""
    n = len(y)
    e, out, score = 0.0, [], []
    before = np.full(n, np.float64(init))
    for s in range(len(staged)):
        G = float(np.abs(y - before).max())
        e = (1.0 + learning_rate) * e + learning_rate * (n + 2) * U * G + U * max(float(np.abs(staged[s]).max()), 1.0)
        r = y - staged[s]
        out.append(e)
        score.append(2.0 * float(np.abs(r).max()) * e + e * e + 2.0 * (n + 3) * U * float(np.mean(r * r)))
        before = staged[s]
    return np.array(out), np.array(score)
