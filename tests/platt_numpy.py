"""numpy float64 restatement of libsvm's ``sigmoid_train``: Platt scaling by the Newton method with backtracking of Lin, Lin and Weng,
"A note on Platt's probabilistic outputs for support vector machines" (Machine Learning 68, 2007), with libsvm's constants.

    minimise  F(A, B) = sum_i t_i f_i + log(1 + exp(-f_i)),   f_i = A dec_i + B
    t_i = (N+ + 1) / (N+ + 2) for y_i > 0, 1 / (N- + 2) otherwise;  start A = 0, B = log((N- + 1) / (N+ + 1))
    Hessian + 1e-12 I; stop when |g_A| and |g_B| < 1e-5; Armijo constant 1e-4; the step is halved down to 1e-10; at most 100 iterations.

The sums are numpy's (pairwise), so an implementation with another summation order agrees to rounding, not to the bit: tests compare through
``bound``, which holds for any two approximate minimisers of this strictly convex function."""
import numpy as np

MAX_ITER, MIN_STEP, SIGMA, EPS, ARMIJO = 100, 1e-10, 1e-12, 1e-5, 1e-4
MIN_PROB = 1e-7
U52 = 2.0 ** -52
CONVERGED, LINE_SEARCH, ITER_LIMIT = 0, 1, 2


def targets(y):
    """(t [n], N+, N-): libsvm's smoothed targets of the labels y (> 0 is the positive class)."""
    pos = np.asarray(y) > 0
    n1, n0 = int(pos.sum()), int((~pos).sum())
    return np.where(pos, (n1 + 1.0) / (n1 + 2.0), 1.0 / (n0 + 2.0)), n1, n0


def objective_terms(dec, t, A, B):
    """The n terms of F in the overflow-safe two-branch form."""
    f = dec * A + B
    with np.errstate(over="ignore"):
        return np.where(f >= 0, t * f + np.log(1.0 + np.exp(-np.abs(f))), (t - 1.0) * f + np.log(1.0 + np.exp(-np.abs(f))))


def p_q(dec, A, B):
    """(p, q) = (1 / (1 + exp(f)), 1 / (1 + exp(-f))) in the two-branch form."""
    f = dec * A + B
    e = np.exp(-np.abs(f))
    return np.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e)), np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def gradient_terms(dec, t, A, B):
    """([n] terms of g_A, [n] terms of g_B): g = sum of them."""
    p, _ = p_q(dec, A, B)
    return dec * (t - p), t - p


def grad_hess(dec, t, A, B):
    """(g [2], H [2, 2]) at (A, B), H with libsvm's sigma on the diagonal."""
    p, q = p_q(dec, A, B)
    d2, d1 = p * q, t - p
    g = np.array([(dec * d1).sum(), d1.sum()])
    h21 = (dec * d2).sum()
    return g, np.array([[SIGMA + (dec * dec * d2).sum(), h21], [h21, SIGMA + d2.sum()]])


def sigmoid_train(dec, y):
    """(A, B, n_iter, status, g [2], H [2, 2]): the fit, and the gradient and Hessian at the result."""
    dec = np.asarray(dec, dtype=np.float64)
    t, n1, n0 = targets(y)
    A, B = 0.0, float(np.log((n0 + 1.0) / (n1 + 1.0)))
    fval = objective_terms(dec, t, A, B).sum()
    status, it = ITER_LIMIT, 0
    while it < MAX_ITER:
        g, H = grad_hess(dec, t, A, B)
        if abs(g[0]) < EPS and abs(g[1]) < EPS:
            status = CONVERGED
            break
        h11, h22, h21 = H[0, 0], H[1, 1], H[0, 1]
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g[0] - h21 * g[1]) / det
        dB = -(-h21 * g[0] + h11 * g[1]) / det
        gd = g[0] * dA + g[1] * dB
        step = 1.0
        while step >= MIN_STEP:
            nA, nB = A + step * dA, B + step * dB
            nf = objective_terms(dec, t, nA, nB).sum()
            if nf < fval + ARMIJO * step * gd:
                A, B, fval = nA, nB, nf
                break
            step /= 2.0
        if step < MIN_STEP:
            status = LINE_SEARCH
            break
        it += 1
    g, H = grad_hess(dec, t, A, B)
    return float(A), float(B), it, status, g, H


def sigmoid_predict(f, A, B):
    """libsvm's two-branch 1 / (1 + exp(A f + B)), unclipped."""
    z = np.asarray(f, dtype=np.float64) * A + B
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def bound(g1, g2, H, dec_max=0.0):
    """|theta_1 - theta_2| <= (|g(theta_1)| + |g(theta_2)|) / lambda for two approximate minimisers of a strictly convex F whose Hessian
    on the segment between them is at least lambda.  H is evaluated at one end.  Along the segment f_i moves by at most
    R |theta_1 - theta_2|, R = sqrt(dec_max^2 + 1), and |d log(p q) / df| <= 1, so every weight p q, and with them the Hessian, keeps at
    least exp(-R x) of its value: lambda = lambda_min(H) exp(-R x), x the distance itself.  With x0 the bound at lambda_min(H), x0
    exp(2 R x0) solves that for R x0 <= 0.1; beyond, the bound is infinite: no statement."""
    lam = float(np.linalg.eigvalsh(H)[0])
    x0 = (float(np.linalg.norm(g1)) + float(np.linalg.norm(g2))) / lam
    R = float(np.hypot(dec_max, 1.0))
    return x0 * float(np.exp(2.0 * R * x0)) if R * x0 <= 0.1 else float("inf")


# ---- what the CPU and the GPU tests share: inputs and the bound with its rounding slack ---------------------------------------------------
def make_dec(n, kind, seed, ratio=0.5):
    """(dec [n], y [n] in {-1, +1}): decision-like values of a chosen character; a fraction ``ratio`` of the labels is +1 (by count, so a
    9:1 split is exact), n = 1 and ratio = 1 give one class."""
    rs = np.random.RandomState(seed)
    n1 = n if ratio >= 1.0 else min(max(int(round(ratio * n)), 1 if n > 1 else 0), n - 1 if n > 1 else n)
    y = np.r_[np.ones(n1), -np.ones(n - n1)][rs.permutation(n)]
    if kind == "mixed":
        dec = 1.5 * y + 1.5 * rs.randn(n)
    elif kind == "separable":
        dec = y * (0.5 + rs.rand(n))
    elif kind == "equal":
        dec = np.full(n, 2.0)
    elif kind == "zero":
        dec = np.zeros(n)
    elif kind == "large":
        # the mixed values with every 16th row far on its own side: |A dec + B| reaches several hundred, where exp of it overflows.  (With
        # every |dec| of that size libsvm's own iteration can end in its line search: a step that would bring |g_A| below 1e-5 changes
        # the objective by less than its rounding.)
        dec = 1.5 * y + 1.5 * rs.randn(n)
        dec[::16] = 1e3 * y[::16]
    else:
        raise ValueError(kind)
    return dec, y


def rounding(terms):
    """First-order rounding of a float64 sum of these n terms in any order: n 2^-52 sum |terms|."""
    return len(terms) * U52 * float(np.abs(terms).sum())


def theta_bound(dec, y, theta1, theta2, H):
    """``bound`` for two parameter pairs, the gradients evaluated by the restatement, plus the rounding of those gradient sums
    carried through the same division."""
    t, _, _ = targets(y)
    gs, slack = [], 0.0
    for A, B in (theta1, theta2):
        ga, gb = gradient_terms(dec, t, A, B)
        gs.append(np.array([ga.sum(), gb.sum()]))
        slack += float(np.hypot(rounding(ga), rounding(gb)))
    return bound(gs[0], gs[1], H, float(np.abs(dec).max())) + slack / float(np.linalg.eigvalsh(H)[0])
