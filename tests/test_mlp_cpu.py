"""CPU: the MLP-classifier oracle (tests/mlp_oracle.py) is pinned to scikit-learn's MLPClassifier on every case the GPU tests use, its
stopping rule and its fold handling are checked, and the scatter among its summation orders -- the figure the GPU tolerances are built
from -- stays below the bound recorded in the oracle."""
import numpy as np
import pytest

import mlp_oracle as O

pytest.importorskip("sklearn.neural_network")

BOUND = 1e-12                     # ~100 x the largest deviation measured (1.1e-14): room for another BLAS build


def _close(a, b, bound=BOUND):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max()) if a.size else 0.0


@pytest.mark.parametrize("case", range(len(O.CASES)), ids=O.CASE_IDS)
def test_oracle_follows_sklearn(case):
    n, f, hidden, act, bs, lr, alpha, epochs = O.CASES[case]
    X, y, coefs, intercepts, curve, n_iter = O.case_fit(case)
    assert 0.40 <= y.mean() <= 0.57
    ref = O.sklearn_fit(X, y, hidden, act, bs, lr, alpha, epochs, O.FIT_SEED)
    assert n_iter == ref.n_iter_ == epochs and len(curve) == len(ref.loss_curve_)
    d_loss = float(np.max(np.abs(np.array(curve) - np.array(ref.loss_curve_)) / np.abs(ref.loss_curve_)))
    d_par = max(_close(a, b) for a, b in zip(coefs + intercepts, ref.coefs_ + ref.intercepts_))
    Xt, _ = O.make_data(50, f, 2)
    d_prob = _close(O.predict_proba(coefs, intercepts, act, Xt), ref.predict_proba(Xt))
    print(f"{O.CASE_IDS[case]}: loss {d_loss:.3g}, parameters {d_par:.3g}, probabilities {d_prob:.3g}")
    assert [W.shape for W in coefs] == [W.shape for W in ref.coefs_]
    assert d_loss <= BOUND and d_par <= BOUND and d_prob <= BOUND


def test_stopping_rule_follows_sklearn():
    """The training-loss rule ends the fit at scikit-learn's epoch, well before max_iter."""
    X, y = O.make_data(200, 100, 5)
    ref = O.sklearn_fit(X, y, (100,), "relu", 32, 0.01, 1e-4, 60, 10)
    _, _, curve, n_iter = O.fit(X, y, (100,), "relu", 32, 0.01, 1e-4, 60, 10)
    print(f"stopped after {n_iter} epochs (scikit-learn: {ref.n_iter_})")
    assert n_iter == ref.n_iter_ < 60
    np.testing.assert_allclose(curve, ref.loss_curve_, rtol=1e-9, atol=0.0)
    # the rule itself: a tolerance nobody meets stops after n_iter_no_change + 1 epochs without improvement, a zero tolerance never
    assert O.fit(X, y, (20,), "tanh", 64, 0.001, 1e-4, 30, 0, tol=10.0, n_iter_no_change=2)[3] == 4
    assert O.fit(X, y, (20,), "tanh", 64, 0.001, 1e-4, 12, 0, tol=0.0, n_iter_no_change=10 ** 9)[3] == 12


@pytest.mark.parametrize("order", O.ORDERS)
def test_train_rows_equal_the_gathered_rows(order):
    X, y = O.make_data(120, 9, 4)
    rows = np.sort(np.random.RandomState(0).choice(120, 77, replace=False))
    a = O.fit(X, y, (12, 5), "tanh", 16, 0.01, 1e-3, 3, 2, train_rows=rows, order=order)
    b = O.fit(X[rows], y[rows], (12, 5), "tanh", 16, 0.01, 1e-3, 3, 2, order=order)
    assert a[3] == b[3] == 3 and a[2] == b[2]
    for p, q in zip(a[0] + a[1], b[0] + b[1]):
        assert np.array_equal(p, q)


def test_scatter_among_summation_orders():
    """S_param / S_loss per case: what another summation order and another libm move.  The GPU tests take 256 x the recorded maxima."""
    import sklearn
    print(f"numpy {np.__version__}, scikit-learn {sklearn.__version__}")
    worst_p = worst_l = 0.0
    for i, (n, f, hidden, act, bs, lr, alpha, epochs) in enumerate(O.CASES):
        X, y = O.case_fit(i)[:2]
        fits = [O.case_fit(i)[2:]] + [O.fit(X, y, hidden, act, bs, lr, alpha, epochs, O.FIT_SEED, order=o) for o in O.ORDERS[1:]]
        s_p = s_l = 0.0
        for u in range(len(fits)):
            for v in range(u + 1, len(fits)):
                assert fits[u][3] == fits[v][3] == epochs
                s_p = max(s_p, max(float(np.abs(a - b).max()) for a, b in zip(fits[u][0] + fits[u][1], fits[v][0] + fits[v][1])))
                cu, cv = np.array(fits[u][2]), np.array(fits[v][2])
                s_l = max(s_l, float((np.abs(cu - cv) / np.abs(cv)).max()))
        print(f"{O.CASE_IDS[i]}: S_param {s_p:.3g}, S_loss {s_l:.3g}")
        worst_p, worst_l = max(worst_p, s_p), max(worst_l, s_l)
    print(f"maxima: S_param {worst_p:.3g} (recorded {O.S_PARAM:.3g}), S_loss {worst_l:.3g} (recorded {O.S_LOSS:.3g})")
    assert worst_p <= 1e-12 and worst_l <= 1e-13
    assert 0.0 < O.S_PARAM <= 1e-12 and 0.0 < O.S_LOSS <= 1e-13


def test_ulp_order_moves_every_transcendental_by_one_neighbour():
    a = np.tanh(np.linspace(-2.0, 2.0, 7).reshape(1, 7))
    b = O._nudge(a, "chunk16r-ulp")
    assert np.array_equal(b.ravel()[0::2], np.nextafter(a.ravel()[0::2], np.inf)) and np.array_equal(b.ravel()[1::2], np.nextafter(a.ravel()[1::2], -np.inf))
    assert O._nudge(a, "chunk16r") is a
    rs = np.random.RandomState(0)
    A, B = rs.randn(5, 37), rs.randn(37, 3)
    assert np.abs(O._matmul(A, B, "chunk16r") - A @ B).max() <= 37 * 2.0 ** -52 * (np.abs(A) @ np.abs(B)).max()
    v = rs.randn(100)
    assert abs(O._vsum(v, "chunk16r") - np.sum(v)) <= 100 * 2.0 ** -52 * np.abs(v).sum()
