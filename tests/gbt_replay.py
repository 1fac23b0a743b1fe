"""CPU replay of a boosted chain: certifies a fitted GradientBoostingClassifier (ours or scikit-learn's) node by node and stage by stage.

Ties between split candidates are broken by rounding (scikit-learn: by a random feature order), so two correct fits of one problem have
different trees.  A fit is therefore not compared with another fit; every decision it took is checked against the data in extended
precision (``np.longdouble``: u_x = 2^-64 on x86, 2 000 times finer than float64's u = 2^-53 =: U) with allowances for what float64
rounding can change.  ``replay`` raises ``ReplayError(check, ...)`` with ``check`` one of

``stop``       a leaf that no stop rule allows, or a split node that a stop rule forbids
``optimal``    a split that is not a valid candidate, or whose score is below the best valid candidate's by more than rounding explains
``threshold``  a threshold that is not the midpoint rule applied to the two float32 neighbours, or a wrong ``n_node_samples``
``leaf``       a leaf value away from mean(g) / mean(p (1 - p))
``raw``        raw scores or ``train_score_`` that are not what the model's own trees give

Notation: a node has m rows, residuals g_i = y_i - expit(raw_i) from the raw scores *the model's own earlier trees give*, A = sum |g_i|,
G = max |g_i|.  A float64 sum of m terms t_i in any order is within (m - 1) U sum |t_i| of the exact sum (Higham, Accuracy and Stability,
eq. 4.4 to first order; the products of U^2 are covered by rounding every constant below up).  The residuals a fit worked with are
float64 evaluations of y - expit(raw); exp is accurate to 1 ulp and its argument carries |raw| U, so each is within
D_i = CG (1 + |raw_i|) U |g_i| + U/2 of the exact one with CG = 4 (exp, one add, one division, the subtraction; the U/2 is the rounding
of p = y - g back from g where g is close to 1).  D = sum over the node of D_i.

* impurity = sum g^2 / m - (sum g / m)^2.  Sum of squares: (m + 1) U m G^2 before the division, so (m + 1) U G^2 after it; the mean is
  within (m + 1) U G, its square within 2 (m + 1) U G^2 + U G^2; the inputs add 4 G max D_i.  Allowance: (3 m + 6) U G^2 + 4 G max D_i.
  A leaf is accepted by the impurity rule when impurity <= 2.2e-16 + allowance, a split node must have impurity > 2.2e-16 - allowance.
* score(f, p) = (n_r S_l - n_l S_r)^2 / (n_l n_r), S_r = S - S_l.  S_l and S are sums of at most m terms: each within m U A + D.  S_r adds
  one rounding: within 2 m U A + 2 D + U A.  diff = n_r S_l - n_l S_r: two products and a subtraction, 3 U m A, plus n_r dS_l + n_l dS_r
  <= m (2 m U A + 2 D + U A).  So |d diff| <= E := (2 m + 4) m U A + 2 m D, and |diff| <= m A.  The score: (2 |diff| E + E^2) / (n_l n_r)
  plus 4 U score for the square, the product of the counts and the division.  This allowance is absolute (the best score can be 0) and
  is evaluated per candidate: the chosen candidate c must satisfy score_x(c) + allow(c) >= max over valid candidates k of
  (score_x(k) - allow(k)), which holds whenever c maximises the float64 scores.
* leaf value v = (sum g / m) / (sum q / m), q_i = p_i (1 - p_i), p_i = y_i - g_i.  Numerator: m U A + D before the division by m, one
  more U after it.  Denominator terms are positive: (m + 3) U sum q, plus |1 - 2 p_i| D_i <= D_i from the inputs.  Allowance (absolute):
  ((m + 1) U A + D) / |sum q| + |v| (((m + 4) U sum q + D) / sum q + 2 U).  The numerator cancels, so this is far above U |v| for a leaf
  whose residuals nearly sum to zero -- and it is what makes a flat relative tolerance fail.
* raw scores: raw += learning_rate * value[leaf] is two IEEE operations, replayed exactly in float64 from the model's own trees; a fused
  multiply-add would differ by one rounding per stage, so the allowance after s stages is s U max(|raw|, 1).  train_score_ = 2 mean(
  log(1 + exp(raw)) - y raw): n terms each within 4 U (|loss_i| + |raw_i|) (exp, log, product, difference), the mean within
  (n + 1) U mean |loss_i|, plus the raw allowance itself (the loss is 1-Lipschitz in raw).

No constant here was fitted to any implementation's output.
"""
import numpy as np

import sklearn_trees

U = 2.0 ** -53
CG = 4.0
LD = np.longdouble
EPSILON = float(np.finfo(np.float64).eps)
FEATURE_THRESHOLD = np.float32(1e-7)


class ReplayError(AssertionError):
    def __init__(self, check, message):
        super().__init__(f"[{check}] {message}")
        self.check = check


def residuals_x(y, raw):
    """(g, D): y - expit(raw) in extended precision, stable on both sides, and the bound on a float64 fit's residuals' distance from it."""
    r = raw.astype(LD)
    e = np.exp(-np.abs(r))
    p_small = e / (1 + e)                                  # expit(-|r|)
    one_minus = p_small                                    # 1 - expit(|r|)
    pos = r >= 0
    g = np.where(y > 0.5, np.where(pos, one_minus, 1 / (1 + e)), np.where(pos, -1 / (1 + e), -p_small))
    D = CG * (1 + np.abs(raw)) * U * np.abs(g).astype(np.float64) + U / 2
    return g, D.astype(LD)


def candidates(fv, msl):
    """Valid split positions of a node's float32 feature values sorted ascending: p splits [0, p) from [p, m)."""
    m = len(fv)
    p = np.arange(1, m)
    ok = fv[1:] > (fv[:-1] + FEATURE_THRESHOLD).astype(np.float32)
    return p[ok & (p >= msl) & (m - p >= msl)]


def midpoint(a, b):
    """scikit-learn's threshold between the float32 neighbours a < b, in float64."""
    thr = np.float64(a) / 2.0 + np.float64(b) / 2.0
    return np.float64(a) if thr == np.float64(b) else thr


def _scores(g_sorted, D_node, pos):
    """(score_x, allowance) at the positions ``pos`` of a node whose residuals are ``g_sorted`` in the feature's order."""
    m = len(g_sorted)
    A = np.abs(g_sorted).sum()
    S = g_sorted.sum()
    S_l = np.cumsum(g_sorted)[pos - 1]
    n_l = pos.astype(LD)
    n_r = m - n_l
    diff = n_r * S_l - n_l * (S - S_l)
    score = diff * diff / (n_l * n_r)
    E = (2 * m + 4) * m * U * A + 2 * m * D_node
    allow = (2 * np.abs(diff) * E + E * E) / (n_l * n_r) + 4 * U * score
    return score, allow


def replay(X, y, trees, init, learning_rate, max_depth, min_samples_split=2, min_samples_leaf=1, raw_stages=None, train_score=None):
    """Replay the chain on its training data.  ``X`` [n, d] (cast to float32), ``y`` [n] in {0, 1}, ``trees`` the flat arrays (left,
    right, feature, threshold, value, n_node_samples, root); ``raw_stages`` [T, n] the model's raw scores of the training rows after every
    stage and ``train_score`` [T], both optional.  Returns a dict of what was seen (counts, the largest used share of each allowance)."""
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
        q = (y.astype(LD) - g) * (1 - (y.astype(LD) - g))
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
            G = float(np.abs(gn).max())
            mean = gn.sum() / m
            impurity = float((gn * gn).sum() / m - mean * mean)
            imp_allow = (3 * m + 6) * U * G * G + 4 * G * float(Dn.max())
            # the best valid candidate of every feature, in extended precision
            best_lo, any_valid, per_feature = -np.inf, False, {}
            if depth < max_depth and m >= 2:
                for f in range(d):
                    o = np.argsort(X32[rows, f], kind="stable")
                    fv = X32[rows, f][o]
                    pos = candidates(fv, min_samples_leaf)
                    if len(pos):
                        any_valid = True
                        score, allow = _scores(gn[o], Dn.sum(), pos)
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
                sq, A = q[rows].sum(), np.abs(gn).sum()
                Dsum = Dn.sum()
                if float(sq) / m < 1e-150:
                    want, allow = (0.0, 0.0) if float(sq) / m < 0.5e-150 else (float(value[node]), 0.0)
                else:
                    want_x = (gn.sum() / m) / (sq / m)
                    allow = float(((m + 1) * U * A + Dsum) / sq + np.abs(want_x) * (((m + 4) * U * sq + Dsum) / sq + 2 * U))
                    want = float(want_x)
                err = abs(float(value[node]) - want)
                if not err <= allow:
                    raise ReplayError("leaf", f"{where}: value {float(value[node])!r}, mean(g) / mean(p (1 - p)) = {want!r}: off by {err:.3e}, "
                                              f"allowance {allow:.3e}")
                if allow > 0:
                    seen["leaf_share"] = max(seen["leaf_share"], err / allow)
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
                raise ReplayError("raw", f"stage {t}: the model's raw scores are off the replay of its own trees by {err:.3e}, allowance {raw_allow:.3e}")
        if train_score is not None:
            r = raw.astype(LD)
            loss = np.where(r > 0, r + np.log1p(np.exp(-np.abs(r))), np.log1p(np.exp(-np.abs(r)))) - y.astype(LD) * r
            want = 2 * loss.sum() / n
            allow = 2 * float((4 * U * (np.abs(loss) + np.abs(r))).sum() / n + (n + 1) * U * np.abs(loss).sum() / n + raw_allow)
            err = abs(float(train_score[t]) - float(want))
            if not err <= allow:
                raise ReplayError("raw", f"stage {t}: train_score_ {float(train_score[t])!r}, the log-loss of the replayed raw scores is {float(want)!r}: "
                                         f"off by {err:.3e}, allowance {allow:.3e}")
    seen["raw"] = raw
    return seen


def trees_of_sklearn(fitted):
    """A fitted scikit-learn GradientBoostingClassifier's trees in the flat convention, and its initial raw score."""
    from scipy.special import logit
    eps32 = np.finfo(np.float32).eps
    init = float(logit(np.clip(np.float64(fitted.init_.class_prior_[1]), eps32, 1 - eps32)))
    return sklearn_trees.trees_of_sklearn(fitted), init


def make_data(n, d, seed=0, decimals=None, informative=None):
    """A seeded two-class problem: the label follows a noisy linear rule over the first ``informative`` features."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, d)
    k = d if informative is None else informative
    w = rs.randn(k)
    y = (X[:, :k] @ w + 0.7 * rs.randn(n) > 0).astype(np.int64)
    if n >= 2 and y.min() == y.max():
        y[0] = 1 - y[0]
    if decimals is not None:
        X = np.round(X, decimals)
    return X, y
