"""Numpy restatement of scikit-learn's ``MLPClassifier(solver="adam", shuffle=True)`` for two classes, in float64: the oracle of the batched
MLP trainer (csrc/mlp.hip, mlp.py).  It does not import the package under test.

The rule (sklearn/neural_network/_multilayer_perceptron.py, _stochastic_optimizers.py):
  start     rs = RandomState(seed); per layer W ~ rs.uniform(-b, b, (fan_in, fan_out)) then bias ~ rs.uniform(-b, b, fan_out), b = sqrt(6 / (fan_in + fan_out))
  epoch     perm = arange(n); rs.shuffle(perm); idx = idx[perm]  (composed onto the previous order); mini-batches of min(batch_size, n) rows of idx
  forward   a[l + 1] = act(a[l] W[l] + b[l]), hidden relu | tanh, output logistic
  loss      -(sum y log p + sum (1 - y) log(1 - p)) / n_b with p clipped to [eps, 1 - eps], plus 0.5 alpha sum_l sum W[l]^2 / n_b
  backward  delta[last] = p - y; dW[l] = (a[l]^T delta[l] + alpha W[l]) / n_b; db[l] = mean over rows of delta[l];
            delta[l - 1] = delta[l] W[l]^T, zero where a relu activation is exactly zero, times 1 - a^2 for tanh
  Adam      t += 1; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); p += -lr_t m / (sqrt(v) + eps)
  epoch end loss = sum(batch loss * batch rows) / n; count the epochs whose loss is > best - tol; stop when the count exceeds n_iter_no_change

``order`` chooses how every sum is taken, so that the scatter among orders measures what a different but equally valid evaluation may move:
  "blas"          numpy's own (``@``, ``np.dot``, ``np.mean``): what scikit-learn itself runs
  "chunk16r"      every reduction in 16-deep chunks of the reduction axis: a chunk's terms are summed last to first, the chunk sums are added last
                  chunk first
  "chunk16r-ulp"  chunk16r, and every tanh and logistic result is moved to its float64 neighbour, up on even and down on odd elements
                  (``np.nextafter``): another libm
"""
import numpy as np

ORDERS = ("blas", "chunk16r", "chunk16r-ulp")

# n, features, hidden, activation, batch, lr, alpha, epochs -- every case uses make_data(n, f, 1) and seed 3
CASES = [
    (65, 7, (1,), "relu", 32, 1e-3, 1e-4, 4),               # width 1; last batch of one row; f % 4 = 3
    (333, 167, (256,), "tanh", 200, 1e-3, 1e-4, 3),         # default batch (13 row tiles, tail 133, the division by n_b); width 256; odd f
    (150, 100, (256, 17, 33), "relu", 64, 1e-3, 1e-4, 3),   # three hidden layers; ragged widths; tail 22
    (40, 3, (20,), "relu", 200, 1e-2, 0.0, 4),              # n < batch; alpha 0; K = 3
    (130, 33, (48, 48), "tanh", 16, 1e-3, 1.0, 3),          # one row tile; tail of 2; large alpha
    (97, 1, (31,), "relu", 48, 1e-3, 1e-4, 4),              # one feature; 3 row tiles on the 4-tile path; tail 1
    (333, 100, (100, 50), "tanh", 64, 1e-2, 1e-4, 4),       # the grid case of test_few_epochs_follow_sklearn_step_for_step, as an anchor
]
CASE_IDS = ["w1-tail1", "batch200-w256", "three-layers", "n-below-batch", "batch16-alpha1", "one-feature", "grid-anchor"]
DATA_SEED, FIT_SEED = 1, 3

# The scatter of the restatement among ORDERS over CASES (tests/test_mlp_cpu.py::test_scatter_among_summation_orders prints and bounds it):
# S_PARAM the largest absolute difference of any parameter, S_LOSS the largest relative difference of any epoch's loss.  Recorded by hand from
# that test's output on an x86-64 Linux host (Intel Xeon), Python 3.10.12, numpy 2.2.6 on its bundled OpenBLAS 0.3.29, scikit-learn 1.7.2.
# Both maxima come from the grid-anchor case (lr 0.01, four epochs) with all three orders.  Per case, S_param / S_loss:
#   w1-tail1 0 / 0; batch200-w256 9.2e-15 / 4.1e-16; three-layers 7.9e-16 / 0; n-below-batch 5.6e-17 / 2.8e-16;
#   batch16-alpha1 5.6e-17 / 1.3e-16; one-feature 5.6e-17 / 1.6e-16; grid-anchor 1.03e-13 / 2.8e-15
# The GPU tests derive their tolerances from these two constants and from nothing the GPU returned.
S_PARAM = 1.03e-13
S_LOSS = 2.8e-15

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def make_data(n, f, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, f)
    w = rs.randn(f)
    y = ((X @ w + 0.5 * rs.randn(n)) > 0).astype(np.float64)
    return X, y


def _vsum(v, order):
    """Sum of a vector."""
    if order == "blas":
        return float(np.sum(v))
    v = np.asarray(v, dtype=np.float64).ravel()
    pad = (-len(v)) % 16
    c = np.concatenate([v, np.zeros(pad)]).reshape(-1, 16)          # (x + 0.0 == x for every x that is summed here)
    part = np.zeros(len(c))
    for k in range(15, -1, -1):
        part = part + c[:, k]
    s = 0.0
    for p in part[::-1]:
        s = s + float(p)
    return s


def _matmul(A, B, order):
    """A [m, K] times B [K, n]."""
    if order == "blas":
        return A @ B
    K = A.shape[1]
    acc = np.zeros((A.shape[0], B.shape[1]))
    for c0 in range(16 * ((K - 1) // 16), -1, -16):
        part = np.zeros_like(acc)
        for k in range(min(c0 + 16, K) - 1, c0 - 1, -1):
            part += A[:, k, None] * B[None, k, :]
        acc += part
    return acc


def _nudge(a, order):
    if order != "chunk16r-ulp":
        return a
    flat = a.ravel().copy()
    flat[0::2] = np.nextafter(flat[0::2], np.inf)
    flat[1::2] = np.nextafter(flat[1::2], -np.inf)
    return flat.reshape(a.shape)


def _forward(coefs, intercepts, activation, a, order):
    acts = [a]
    for l, (W, b) in enumerate(zip(coefs, intercepts)):
        z = _matmul(acts[-1], W, order) + b
        if l + 1 < len(coefs):
            z = np.maximum(z, 0.0) if activation == "relu" else _nudge(np.tanh(z), order)
        else:
            z = _nudge(1.0 / (1.0 + np.exp(-z)), order)
        acts.append(z)
    return acts


def _xlogy(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 0.0, x * np.log(y))


def init_params(units, rs):
    coefs, intercepts = [], []
    for fan_in, fan_out in zip(units[:-1], units[1:]):
        bound = np.sqrt(6.0 / (fan_in + fan_out))
        coefs.append(rs.uniform(-bound, bound, (fan_in, fan_out)))
        intercepts.append(rs.uniform(-bound, bound, fan_out))
    return coefs, intercepts


def fit(X, y, hidden, activation, batch_size, lr, alpha, max_iter, seed, tol=1e-4, n_iter_no_change=10, train_rows=None, order="blas"):
    """-> (coefs, intercepts, loss_curve, n_iter).  ``train_rows``: row ids into X (a fold); the rows are gathered mini-batch by mini-batch."""
    assert activation in ("relu", "tanh") and order in ORDERS
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    rows = np.arange(len(y)) if train_rows is None else np.asarray(train_rows, dtype=np.int64)
    n = len(rows)
    units = [X.shape[1]] + list(hidden) + [1]
    rs = np.random.RandomState(seed)
    coefs, intercepts = init_params(units, rs)
    params = coefs + intercepts
    ms = [np.zeros_like(p) for p in params]
    vs = [np.zeros_like(p) for p in params]
    L = len(coefs)
    bs = int(np.clip(batch_size, 1, n))
    eps = np.finfo(np.float64).eps
    idx = np.arange(n)
    t, best, no_improve, curve = 0, np.inf, 0, []
    for _ in range(max_iter):
        perm = np.arange(n)
        rs.shuffle(perm)
        idx = idx[perm]
        accumulated = 0.0
        for b0 in range(0, n, bs):
            take = rows[idx[b0:b0 + bs]]
            nb = len(take)
            yb = y[take].reshape(-1, 1)
            acts = _forward(coefs, intercepts, activation, X[take], order)
            p = np.clip(acts[-1], eps, 1.0 - eps)
            loss = -(_vsum(_xlogy(yb, p), order) + _vsum(_xlogy(1.0 - yb, 1.0 - p), order)) / nb
            if order == "blas":
                values = 0
                for W in coefs:
                    values += np.dot(W.ravel(), W.ravel())
            else:
                values = 0.0
                for W in coefs[::-1]:
                    values += _vsum(W.ravel() * W.ravel(), order)
            loss += (0.5 * alpha) * values / nb
            accumulated += loss * nb
            delta = acts[-1] - yb
            cg, ig = [None] * L, [None] * L
            for l in range(L - 1, -1, -1):
                g = _matmul(np.ascontiguousarray(acts[l].T), delta, order)
                g += alpha * coefs[l]
                g /= nb
                cg[l] = g
                ig[l] = np.mean(delta, 0) if order == "blas" else _matmul(np.ones((1, nb)), delta, order)[0] / nb
                if l > 0:
                    delta = _matmul(delta, np.ascontiguousarray(coefs[l].T), order)
                    if activation == "relu":
                        delta[acts[l] == 0.0] = 0.0
                    else:
                        delta *= 1.0 - acts[l] ** 2
            t += 1
            lr_t = lr * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
            for i, g in enumerate(cg + ig):
                ms[i] = BETA1 * ms[i] + (1.0 - BETA1) * g
                vs[i] = BETA2 * vs[i] + (1.0 - BETA2) * (g ** 2)
                params[i] += -lr_t * ms[i] / (np.sqrt(vs[i]) + ADAM_EPS)
        epoch_loss = accumulated / n
        curve.append(float(epoch_loss))
        no_improve = no_improve + 1 if epoch_loss > best - tol else 0
        if epoch_loss < best:
            best = epoch_loss
        if no_improve > n_iter_no_change:
            break
    return coefs, intercepts, curve, len(curve)


def predict_proba(coefs, intercepts, activation, X):
    """The forward pass alone: [n, 2], columns P(class 0), P(class 1)."""
    p1 = _forward(coefs, intercepts, activation, np.asarray(X, dtype=np.float64), "blas")[-1][:, 0]
    return np.stack([1.0 - p1, p1], axis=1)


_FITS = {}


def case_fit(i):
    """fit(order="blas") of CASES[i], computed once per process and shared (treat as read-only): (X, y, coefs, intercepts, curve, n_iter)."""
    if i not in _FITS:
        n, f, hidden, act, bs, lr, alpha, epochs = CASES[i]
        X, y = make_data(n, f, DATA_SEED)
        _FITS[i] = (X, y) + tuple(fit(X, y, hidden, act, bs, lr, alpha, epochs, FIT_SEED))
    return _FITS[i]


def sklearn_fit(X, y, hidden, activation, batch_size, lr, alpha, max_iter, seed, tol=1e-4, n_iter_no_change=10):
    import warnings
    from sklearn.neural_network import MLPClassifier
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MLPClassifier(hidden_layer_sizes=tuple(hidden), activation=activation, solver="adam", alpha=alpha, batch_size=batch_size,
                             learning_rate_init=lr, max_iter=max_iter, tol=tol, n_iter_no_change=n_iter_no_change, random_state=seed,
                             shuffle=True).fit(X, y)
