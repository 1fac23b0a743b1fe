"""GPU: the batched MLP-classifier trainer (csrc/mlp.hip, mlp.py) against scikit-learn's MLPClassifier with the same
hyper-parameters and random_state (third-party arithmetic, scikit-learn is the oracle), and -- beyond the reference's
grid: three hidden layers, widths 1 to 256, any feature count, the default batch of 200, one-row tails, both trainer kernels -- against its
numpy restatement tests/mlp_oracle.py, which tests/test_mlp_cpu.py pins to scikit-learn on the same cases."""
import ctypes
import warnings

import numpy as np
import pytest

from bbbp_amd import _lib
from bbbp_amd.mlp import GridMLPTrainer, MLPConfig, grid_search_cv
import mlp_oracle as O
from mlp_oracle import make_data
from poison import poisoned_allocations

pytestmark = pytest.mark.gpu
sk = pytest.importorskip("sklearn.neural_network")


def sk_fit(X, y, cfg):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = sk.MLPClassifier(hidden_layer_sizes=tuple(cfg.hidden_layer_sizes), activation=cfg.activation, solver="adam", alpha=cfg.alpha,
                             batch_size=cfg.batch_size, learning_rate_init=cfg.learning_rate_init, max_iter=cfg.max_iter, tol=cfg.tol,
                             n_iter_no_change=cfg.n_iter_no_change, random_state=cfg.random_state, shuffle=True)
        rows = np.arange(len(y)) if cfg.train_rows is None else cfg.train_rows
        m.fit(X[rows], y[rows])
    return m


@pytest.mark.parametrize("hidden,act,bs,lr", [((100,), "relu", 32, 0.001), ((100, 50), "tanh", 64, 0.01), ((200, 100), "relu", 128, 0.001),
                                              ((20,), "tanh", 7, 0.1)])
def test_few_epochs_follow_sklearn_step_for_step(dev, hidden, act, bs, lr):
    X, y = make_data(333, 100, 1)          # 333 rows: a ragged last mini-batch
    cfg = MLPConfig(hidden_layer_sizes=hidden, activation=act, batch_size=bs, learning_rate_init=lr, max_iter=4, random_state=3)
    ref = sk_fit(X, y, cfg)
    got = GridMLPTrainer(X, y, device=dev).fit([cfg], epochs_per_launch=3)[0]
    assert got.n_iter_ == ref.n_iter_ == 4
    np.testing.assert_allclose(got.loss_curve_, ref.loss_curve_, rtol=1e-9, atol=1e-12)
    # summation order inside the products differs from BLAS: last-bit differences, amplified by lr = 0.1 / batch 7
    tol = 1e-4 if lr >= 0.1 else 1e-6      # (scikit-learn's own BLAS threading changes its last bits from host to host)
    for a, b in zip(got.coefs_ + got.intercepts_, ref.coefs_ + ref.intercepts_):
        np.testing.assert_allclose(a, b, rtol=tol, atol=tol * 1e-2)
    Xt, _ = make_data(50, 100, 2)
    np.testing.assert_allclose(got.predict_proba(Xt), ref.predict_proba(Xt), rtol=tol, atol=tol * 1e-2)
    assert (got.predict(Xt) == ref.predict(Xt)).all()


def test_stopping_rule_and_many_models_at_once(dev):
    """Training-loss stopping (tol / n_iter_no_change) ends each fit at scikit-learn's epoch; several fits with different
    folds, sizes and seeds run in ONE launch sequence and do not disturb each other."""
    X, y = make_data(400, 100, 5)
    rs = np.random.RandomState(0)
    cfgs = []
    for i, (hidden, act, lr, bs) in enumerate([((100,), "relu", 0.01, 32), ((100, 50), "relu", 0.01, 64), ((100,), "tanh", 0.1, 128),
                                               ((200, 100), "tanh", 0.01, 64), ((100,), "relu", 0.1, 32)]):
        rows = np.sort(rs.choice(400, 320, replace=False))
        cfgs.append(MLPConfig(hidden_layer_sizes=hidden, activation=act, learning_rate_init=lr, batch_size=bs, max_iter=60,
                              random_state=10 + i, train_rows=rows))
    fitted = GridMLPTrainer(X, y, device=dev).fit(cfgs, epochs_per_launch=8)
    for cfg, got in zip(cfgs, fitted):
        ref = sk_fit(X, y, cfg)
        # chaotic amplification of last-bit differences over thousands of Adam steps: compare the trajectory loosely
        assert abs(got.n_iter_ - ref.n_iter_) <= 3, (got.n_iter_, ref.n_iter_)
        k = min(got.n_iter_, ref.n_iter_, 10)
        np.testing.assert_allclose(got.loss_curve_[:k], ref.loss_curve_[:k], rtol=1e-6)
        agree = (got.predict(X) == ref.predict(X)).mean()
        assert agree >= 0.97, agree


def test_grid_search_cv_matches_sklearn_choice(dev):
    X, y = make_data(300, 100, 9)
    grid = {"hidden_layer_sizes": [(100,), (100, 50)], "activation": ["relu", "tanh"], "learning_rate_init": [0.001, 0.1], "batch_size": [64]}
    base = MLPConfig(max_iter=15)
    best, scores, fitted = grid_search_cv(X, y, grid, cv=3, base=base, device=dev, random_state=0)
    assert len(scores) == 8 and len(fitted) == 24 and all(0.0 <= s <= 1.0 for s in scores)
    from sklearn.model_selection import GridSearchCV
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gs = GridSearchCV(sk.MLPClassifier(max_iter=15, random_state=0), {**grid, "solver": ["adam"]}, cv=3, scoring="f1").fit(X, y)
    keys = sorted(grid)
    ref_scores = {tuple(p[k] for k in keys): s for p, s in zip(gs.cv_results_["params"], gs.cv_results_["mean_test_score"])}
    from itertools import product
    ours = {vals: s for vals, s in zip(product(*(grid[k] for k in keys)), scores)}
    for kk in ours:
        assert abs(ours[kk] - ref_scores[kk]) <= 0.03, (kk, ours[kk], ref_scores[kk])


def test_mlp_errors(dev):
    X, y = make_data(20, 5, 0)
    with pytest.raises(RuntimeError):
        GridMLPTrainer(X, y, device="cpu")
    with pytest.raises(ValueError):
        GridMLPTrainer(X, y + 2, device=dev)
    with pytest.raises(ValueError):
        GridMLPTrainer(X, y, device=dev).fit([MLPConfig(activation="logistic")])
    assert GridMLPTrainer(X, y, device=dev).fit([]) == []
    # beyond the documented contract: refused by Python before any launch
    with pytest.raises(ValueError, match="1 to 3 hidden layers"):
        GridMLPTrainer(X, y, device=dev).fit([MLPConfig(hidden_layer_sizes=(4, 4, 4, 4))])
    with pytest.raises(ValueError, match="256 units"):
        GridMLPTrainer(X, y, device=dev).fit([MLPConfig(hidden_layer_sizes=(257,))])
    for bad in (dict(hidden_layer_sizes=(4, 0)), dict(hidden_layer_sizes=()), dict(batch_size=0), dict(max_iter=0),
                dict(train_rows=np.array([0, 20])), dict(train_rows=np.array([-1, 3])), dict(train_rows=np.array([], dtype=np.int64)),
                dict(train_rows=np.arange(4).reshape(2, 2))):         # row ids are gathered by the kernel unchecked: 20 is one past the end
        with pytest.raises(ValueError):
            GridMLPTrainer(X, y, device=dev).fit([MLPConfig(**bad)])
    with pytest.raises(RuntimeError, match="before fit"):
        GridMLPTrainer(X, y, device=dev)._predict(0, X)
    trainer = GridMLPTrainer(X, y, device=dev)
    fitted = trainer.fit([MLPConfig(hidden_layer_sizes=(4,), max_iter=1)])[0]
    for bad in (np.zeros((3, 4)), np.zeros((3, 6)), np.zeros(5)):
        with pytest.raises(ValueError, match="X must be"):
            fitted.predict(bad)
        with pytest.raises(ValueError, match="X must be"):
            fitted.predict_proba(bad)
    assert fitted.predict(X).shape == (20,)


def test_fits_that_share_a_random_stream_equal_the_same_fits_run_alone(dev):
    """Round 4: fits with the same (integer seed, layer sizes, number of training rows) consume ONE RandomState stream on the host (initial
    weights and shuffles drawn once per group).  Five such fits -- other folds, batch sizes, learning rates, epoch counts -- in one call
    must give, bit for bit, what each gives when it is the only fit of a call (where it owns its stream)."""
    X, y = make_data(400, 100, 9)
    rs = np.random.RandomState(1)
    cfgs = []
    for i, (bs, lr, epochs) in enumerate([(32, 0.01, 5), (64, 0.01, 3), (128, 0.1, 7), (32, 0.001, 2), (64, 0.1, 6)]):
        rows = np.sort(rs.choice(400, 320, replace=False))
        cfgs.append(MLPConfig(hidden_layer_sizes=(100, 50), activation="relu", learning_rate_init=lr, batch_size=bs, max_iter=epochs, tol=0.0,
                              n_iter_no_change=10 ** 9, random_state=0, train_rows=rows))
    together = GridMLPTrainer(X, y, device=dev).fit(cfgs, epochs_per_launch=4)
    for cfg, got in zip(cfgs, together):
        alone = GridMLPTrainer(X, y, device=dev).fit([cfg], epochs_per_launch=4)[0]
        assert got.n_iter_ == alone.n_iter_ == cfg.max_iter
        assert got.loss_curve_ == alone.loss_curve_
        for a, b in zip(got.coefs_ + got.intercepts_, alone.coefs_ + alone.intercepts_):
            assert np.array_equal(a, b)


# ---- against the numpy restatement, beyond the reference's grid --------------------------------------------------------------------------------
# S_PARAM / S_LOSS: what the restatement itself moves by when its sums are taken in another order and its tanh / logistic come from
# another libm (recorded in mlp_oracle.py from a CPU run).  The GPU's order and its tanh / exp are one more draw of that family; the factor
# 256 gives the draw eight more bits.  The bounds of the scikit-learn comparison above (1e-9 on the loss, 1e-6 on parameters) stay a ceiling.
TOL_PARAM = max(256 * O.S_PARAM, 1e-12)          # |a - b| <= TOL_PARAM (1 + |b|)
TOL_LOSS = max(256 * O.S_LOSS, 1e-13)            # relative
assert TOL_PARAM <= 1e-6 and TOL_LOSS <= 1e-9
THREE_LAYERS, BATCH_200, N_BELOW_BATCH = 2, 1, 3  # rows of O.CASES


def _case_config(case, **kw):
    n, f, hidden, act, bs, lr, alpha, epochs = O.CASES[case]
    return MLPConfig(hidden_layer_sizes=hidden, activation=act, batch_size=bs, learning_rate_init=lr, alpha=alpha, max_iter=epochs,
                     random_state=O.FIT_SEED, **kw)


def _fit_case(dev, case, epochs_per_launch=2):
    n, f = O.CASES[case][:2]
    X, y = make_data(n, f, O.DATA_SEED)
    return GridMLPTrainer(X, y, device=dev).fit([_case_config(case)], epochs_per_launch=epochs_per_launch)[0]


def _deviation(coefs, intercepts, curve, ref_coefs, ref_intercepts, ref_curve):
    """(largest |a - b| / (1 + |b|) over the parameters, largest relative difference of the loss curve)"""
    assert len(curve) == len(ref_curve) and [a.shape for a in coefs + intercepts] == [b.shape for b in ref_coefs + ref_intercepts]
    d_par = max(float((np.abs(a - b) / (1.0 + np.abs(b))).max()) for a, b in zip(coefs + intercepts, ref_coefs + ref_intercepts))
    d_loss = float((np.abs(np.array(curve) - np.array(ref_curve)) / np.abs(ref_curve)).max())
    return d_par, d_loss


def _bits(model, *queries):
    return ([np.array(model.loss_curve_), np.array([model.n_iter_])] + list(model.coefs_) + list(model.intercepts_)
            + [model.predict_proba(Q) for Q in queries] + [model.predict(Q) for Q in queries])


def _same_bits(want, got, what):
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"{what}: result {i} differs"


@pytest.mark.parametrize("kernel", ["mfma", "scalar"])
@pytest.mark.parametrize("case", range(len(O.CASES)), ids=O.CASE_IDS)
def test_cases_follow_the_restatement(dev, monkeypatch, case, kernel):
    """Both trainer kernels (BBBP_MLP_SCALAR is read at every launch) follow the restatement epoch for epoch within 256 x its own scatter, and
    the predict kernel gives the forward pass of the weights it is handed: three layers of dot products of at most 256 terms carry at most
    256 x 2^-53 ~ 3e-14 of sum |a||w| each, so 1e-11 absolute on a probability."""
    if kernel == "scalar":
        monkeypatch.setenv("BBBP_MLP_SCALAR", "1")
    n, f, hidden, act, bs, lr, alpha, epochs = O.CASES[case]
    _, _, coefs, intercepts, curve, n_iter = O.case_fit(case)
    got = _fit_case(dev, case)
    assert got.n_iter_ == n_iter == epochs
    d_par, d_loss = _deviation(got.coefs_, got.intercepts_, got.loss_curve_, coefs, intercepts, curve)
    Xt, _ = make_data(50, f, 2)
    d_prob = []
    for rows in (50, 1, 9):                      # 9 rows: a full and a partial 8-row work-group
        p = got.predict_proba(Xt[:rows])
        assert p.shape == (rows, 2)
        d_prob.append(float(np.abs(p - O.predict_proba(got.coefs_, got.intercepts_, act, Xt[:rows])).max()))
        assert np.array_equal(got.predict(Xt[:rows]), (p[:, 1] > 0.5).astype(np.int64))
    print(f"{O.CASE_IDS[case]} {kernel}: parameters {d_par:.3g} = {d_par / O.S_PARAM:.3g} S_PARAM, loss {d_loss:.3g} = {d_loss / O.S_LOSS:.3g} S_LOSS, "
          f"probabilities {max(d_prob):.3g}")
    assert d_loss <= TOL_LOSS
    assert d_par <= TOL_PARAM
    assert max(d_prob) <= 1e-11


def test_scalar_and_mfma_kernels_agree(dev, monkeypatch):
    """Neither kernel is the other's oracle: on the three-hidden-layer case they agree within the same bounds, in both directions."""
    mfma = _fit_case(dev, THREE_LAYERS)
    monkeypatch.setenv("BBBP_MLP_SCALAR", "1")
    scalar = _fit_case(dev, THREE_LAYERS)
    assert mfma.n_iter_ == scalar.n_iter_ == O.CASES[THREE_LAYERS][7]
    for a, b, name in ((mfma, scalar, "mfma against scalar"), (scalar, mfma, "scalar against mfma")):
        d_par, d_loss = _deviation(a.coefs_, a.intercepts_, a.loss_curve_, b.coefs_, b.intercepts_, b.loss_curve_)
        print(f"{name}: parameters {d_par:.3g}, loss {d_loss:.3g}")
        assert d_par <= TOL_PARAM and d_loss <= TOL_LOSS


def test_instrumented_kernel_gives_the_same_bits(dev):
    """mlp_train_mfma_kernel<true> (bbbp_mlp_profile, tools/mlp_phases.py) only counts cycles.  With three hidden layers the fourth layer's
    marks share the profile slots 10 and 11 with the tails; the mini-batch counter (slot 15) is exact."""
    n, _, _, _, bs, _, _, epochs = O.CASES[THREE_LAYERS]
    Q, _ = make_data(9, O.CASES[THREE_LAYERS][1], 2)
    want = _bits(_fit_case(dev, THREE_LAYERS), Q)
    L = _lib.lib()
    counters = (ctypes.c_ulonglong * 16)()
    _lib.check(L.bbbp_mlp_profile(1, None), "bbbp_mlp_profile")
    try:
        got = _bits(_fit_case(dev, THREE_LAYERS), Q)
    finally:
        _lib.check(L.bbbp_mlp_profile(0, ctypes.cast(counters, ctypes.c_void_p)), "bbbp_mlp_profile")
    _same_bits(want, got, "instrumented kernel")
    c = list(counters)
    assert c[15] == epochs * -(-n // bs), c
    assert all(c[k] > 0 for k in range(12) if k != 4) and c[4] == 0 and c[12] == c[13] == c[14] == 0, c     # slot 4: delta below layer 0, never


@pytest.mark.parametrize("case", [BATCH_200, N_BELOW_BATCH], ids=[O.CASE_IDS[BATCH_200], O.CASE_IDS[N_BELOW_BATCH]])
def test_launch_boundaries_do_not_change_the_bits(dev, case):
    """All of a fit's state crosses a launch boundary through memory: one, two or eight epochs per launch give the same bits."""
    Q, _ = make_data(9, O.CASES[case][1], 2)
    want = _bits(_fit_case(dev, case, epochs_per_launch=1), Q)
    for epl in (2, 8):
        _same_bits(want, _bits(_fit_case(dev, case, epochs_per_launch=epl), Q), f"{epl} epochs per launch")


def test_more_fits_than_compute_units(dev):
    """300 fits in one call: more work-groups than the chip has compute units, the cost sort permutes the slots, three RandomState
    streams are shared by 100 fits each.  Every seventh fit equals, bit for bit, the same fit run alone, and so does its prediction
    (FittedMLP maps its index to its slot)."""
    X, y = make_data(60, 5, 7)
    rs = np.random.RandomState(2)
    hiddens, batches = [(8,), (24, 8), (40, 3, 9)], [16, 200, 7]
    cfgs = [MLPConfig(hidden_layer_sizes=hiddens[i % 3], activation=("relu", "tanh")[(i // 9) % 2], batch_size=batches[(i // 3) % 3], max_iter=2,
                      random_state=i % 3, train_rows=np.sort(rs.choice(60, 48, replace=False))) for i in range(300)]
    trainer = GridMLPTrainer(X, y, device=dev)
    together = trainer.fit(cfgs)
    slots = [h["slot"] for h in trainer._keep]
    assert sorted(slots) == list(range(300)) and slots != list(range(300))
    for i in range(0, 300, 7):
        alone = GridMLPTrainer(X, y, device=dev).fit([cfgs[i]])[0]
        assert together[i].n_iter_ == 2
        _same_bits(_bits(alone, X), _bits(together[i], X), f"fit {i} of 300")


@pytest.mark.parametrize("case", [THREE_LAYERS, BATCH_200], ids=[O.CASE_IDS[THREE_LAYERS], O.CASE_IDS[BATCH_200]])
def test_fit_and_predict_under_poison(dev, monkeypatch, case):
    """The visiting orders, the model array and the predictor's output are ``torch.empty``: under the fills 0xFF (NaN as float64, -1 as a
    row id) and 0x7B a fit and a predict give the bits of an unpoisoned run, and no guard band is touched."""
    Q9, _ = make_data(9, O.CASES[case][1], 2)
    Q50, _ = make_data(50, O.CASES[case][1], 2)
    want = _bits(_fit_case(dev, case), Q9, Q50)
    for fill in (0xFF, 0x7B):
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _bits(_fit_case(dev, case), Q9, Q50)
        assert pa.check() > 0, "no allocation went through the pools"
        pa.release()
        _same_bits(want, got, f"fill {fill:#04x}")
