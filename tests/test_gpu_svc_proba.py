"""GPU: svm.platt_scale, the out-of-fold decision kernel, svm.PlattSVC and its predict_proba against the numpy restatement of libsvm's
sigmoid_train (tests/platt_numpy.py, pinned on the CPU by tests/test_platt_cpu.py) and against scikit-learn fitted on the same folds.

Bounds.  A float64 sum of n terms in any order is within n 2^-52 sum |terms| of the exact value (first order), two such sums within twice
that.  Two approximate minimisers of the strictly convex calibration objective differ by at most (|g(theta_1)| + |g(theta_2)|) /
lambda_min(H) (platt_numpy.bound); where the Hessian is singular up to sigma (one point, all decision values equal) that bound says
nothing and the gradient criterion alone is checked."""
import functools

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
from bbbp_amd.svm import SVC, PlattSVC, kernel_matrix, platt_folds, platt_scale
import platt_numpy as P
import svc_oracle as O
from platt_numpy import make_dec, rounding, theta_bound

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
RATIOS = (0.5, 0.9, 1.0)                  # balanced, 9:1, every label +1
KINDS = ("mixed", "separable", "equal", "zero", "large")


def platt_cases(kind):
    return [make_dec(n, kind, 100 + 7 * i + j, ratio) for i, n in enumerate(NS) for j, ratio in enumerate(RATIOS)]


def _gradient_check(dec, y, A, B):
    """|g| at (A, B) in numpy against libsvm's criterion plus the rounding of the two sums."""
    t, _, _ = P.targets(y)
    ga, gb = P.gradient_terms(dec, t, A, B)
    assert abs(ga.sum()) < P.EPS + rounding(ga) and abs(gb.sum()) < P.EPS + rounding(gb), (len(dec), ga.sum(), gb.sum())


@pytest.mark.parametrize("kind", KINDS)
def test_platt_scale_against_restatement(dev, kind):
    """Every size and label ratio of one kind of input in one batch.  The restatement stops by the gradient criterion on all of them
    (asserted); the device must report the same status, meet the criterion as numpy evaluates it, and land within the convexity bound."""
    cases = platt_cases(kind)
    A, B, n_iter, status = platt_scale([c[0] for c in cases], [c[1] for c in cases])
    assert A.shape == B.shape == n_iter.shape == status.shape == (len(cases),) and A.dtype == np.float64 and n_iter.dtype == np.int32
    worst = 0.0
    for q, (dec, y) in enumerate(cases):
        a, b, it, st, g, H = P.sigmoid_train(dec, y)
        assert st == P.CONVERGED, f"the restatement did not converge on case {q}"
        assert status[q] == st and 0 <= n_iter[q] <= P.MAX_ITER
        _gradient_check(dec, y, A[q], B[q])
        limit = theta_bound(dec, y, (A[q], B[q]), (a, b), H)
        diff = float(np.hypot(A[q] - a, B[q] - b))
        assert diff <= limit, (q, len(dec), diff, limit)
        if np.isfinite(limit) and limit > 0.0:
            worst = max(worst, diff / limit)
    print(f"{kind}: {len(cases)} problems, largest |theta - restatement| / bound = {worst:.3g}, iterations up to {n_iter.max()}")
    # one problem alone, as numpy and as a CUDA tensor: the same bits as in the batch
    q = len(cases) - 3
    dec, y = cases[q]
    assert platt_scale(dec, y) == (A[q], B[q], n_iter[q], status[q])
    assert platt_scale(torch.from_numpy(dec).cuda(), torch.from_numpy(y).cuda()) == (A[q], B[q], n_iter[q], status[q])


def test_platt_scale_where_the_criterion_cannot_be_met(dev):
    """|dec| of 1e13: the gradient's A component is a sum of terms of that size whose rounding alone exceeds 1e-5, so no step decreases
    the objective any further and the restatement ends by line-search failure (asserted).  The device must end the same way, at an
    objective no larger than the restatement's up to the rounding of that sum."""
    dec, y = make_dec(257, "mixed", 9)
    dec = dec * 1e13
    a, b, it, st, _, _ = P.sigmoid_train(dec, y)
    assert st == P.LINE_SEARCH
    A, B, n_iter, status = platt_scale(dec, y)
    t, _, _ = P.targets(y)
    got, want = P.objective_terms(dec, t, A, B), P.objective_terms(dec, t, a, b)
    print(f"restatement: {it} iterations, F {want.sum():.17g}; device: {n_iter} iterations, F {got.sum():.17g}")
    assert status == st
    assert got.sum() <= want.sum() + rounding(got) + rounding(want)


def test_platt_scale_batch_independence_and_repeatability(dev):
    """Seven problems of different n: together, alone, reversed and once more give the same bits."""
    cases = [make_dec(n, kind, 50 + n, ratio) for n, kind, ratio in ((1, "mixed", 1.0), (63, "mixed", 0.5), (130, "separable", 0.5), (256, "large", 0.9),
                                                                     (257, "equal", 0.5), (1000, "mixed", 0.9), (1025, "mixed", 0.5))]
    decs, ys = [c[0] for c in cases], [c[1] for c in cases]
    together = platt_scale(decs, ys)
    again = platt_scale(decs, ys)
    backwards = platt_scale(decs[::-1], ys[::-1])
    for a, b, c in zip(together, again, backwards):
        assert np.array_equal(a, b) and np.array_equal(a, c[::-1])
    for q, (dec, y) in enumerate(cases):
        assert platt_scale(dec, y) == tuple(v[q] for v in together), f"problem {q} alone differs from the batch"
    assert list(together[3]) == [P.sigmoid_train(dec, y)[3] for dec, y in cases]


def _two_class_data(n, d, seed):
    """Alternating labels (every training part of every fold below has both classes), X = randn + 0.7 y on the first features."""
    rs = np.random.RandomState(seed)
    y = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    X = rs.randn(n, d)
    X[:, :min(3, d)] += 0.7 * y[:, None]
    return X, y


@pytest.mark.parametrize("kind", ["rbf", "linear"])
@pytest.mark.parametrize("n,folds", [(5, [[0], [1], [2], [3], [4]]), (23, None), (130, "three")])
def test_oof_decision(dev, n, folds, kind):
    """The out-of-fold values against a numpy sum over the device's own kernel matrix and each fold's own alpha and rho: only the order of
    summation can differ.  Folds of one row (n = 5), libsvm's unequal folds 4, 5, 4, 5, 5 (n = 23) and three folds of 43, 43, 44."""
    X, y = _two_class_data(n, 7, n)
    held = platt_folds(23, 5, 4) if folds is None else platt_folds(130, 3, 4) if folds == "three" else [np.array(f) for f in folds]
    clf = PlattSVC(C=1.0, kernel=kind).fit(X, y, folds=held)
    assert clf.oof_decision_.shape == (n,) and clf.oof_decision_.dtype == np.float64 and len(clf._folds) == len(held)
    K = kernel_matrix(torch.from_numpy(X).cuda(), kind, clf._gamma)[0].cpu().numpy()
    ys = np.where(y == clf.classes_[0], 1.0, -1.0)
    worst = 0.0
    for te, (rows, te_dev, alpha, rho) in zip(held, clf._folds):
        tr = np.setdiff1d(np.arange(n), te)
        assert np.array_equal(rows, tr) and np.array_equal(te_dev, te) and alpha.shape == tr.shape
        single = SVC(C=1.0, kernel="linear").fit(X[tr], y[tr]).decision_function(X[te]) if kind == "linear" else None
        for k, i in enumerate(te):
            terms = np.r_[alpha * ys[tr] * K[i, tr], -rho]
            limit = 2.0 * n * P.U52 * np.abs(terms).sum()
            assert abs(clf.oof_decision_[i] - terms.sum()) <= limit
            worst = max(worst, abs(clf.oof_decision_[i] - terms.sum()) / limit)
            if single is not None:          # the fold problem over the shared matrix is the single fit (pinned bit for bit by grid_search_cv's tests)
                assert abs(-clf.oof_decision_[i] - single[k]) <= limit
    print(f"n {n} {kind}: largest error / bound = {worst:.3g}")
    # the rest of the fit is SVC's, bit for bit
    plain = SVC(C=1.0, kernel=kind).fit(X, y)
    assert np.array_equal(clf.alpha_, plain.alpha_) and clf.intercept_[0] == plain.intercept_[0] and clf.n_iter_ == plain.n_iter_
    assert np.array_equal(clf.decision_function(X), plain.decision_function(X)) and np.array_equal(clf.predict(X), plain.predict(X))


@pytest.mark.parametrize("minority,const", [(1.0, 1.0), (-1.0, -1.0)])
def test_one_class_training_fold(dev, minority, const):
    """Twelve rows, two of the minority class, both held out by the first fold: its training part has one class, libsvm solves nothing and
    gives the held-out rows +1 when that class is the solver's +1 (classes_[0], the label -1.0 here) and -1 otherwise."""
    rs = np.random.RandomState(3)
    y = np.full(12, -minority)
    y[[4, 9]] = minority
    X = rs.randn(12, 4) + 0.8 * y[:, None]
    folds = [[4, 9], [0, 1, 2, 3, 5], [6, 7, 8, 10, 11]]
    clf = PlattSVC().fit(X, y, folds=folds)
    assert (clf.oof_decision_[[4, 9]] == const).all() and len(clf._folds) == 2
    assert np.isfinite(clf.oof_decision_).all() and np.isfinite(clf.probA_).all() and np.isfinite(clf.probB_).all()
    proba = clf.predict_proba(X)
    assert proba.shape == (12, 2) and np.isfinite(proba).all()
    # every row in one fold: nothing is trained on, every value is 0
    clf = PlattSVC().fit(X, y, folds=[np.arange(12)])
    assert (clf.oof_decision_ == 0.0).all() and clf._folds == [] and clf.probA_.shape == clf.probB_.shape == (1,)


@functools.lru_cache(maxsize=None)
def _fitted():
    X, y = O.make_data(130, 17, 0.7, 4)
    return X, y, PlattSVC().fit(X, y)


def _check_proba(proba, f, A, B):
    z = f * A + B
    want = np.clip(P.sigmoid_predict(f, A, B), P.MIN_PROB, 1.0 - P.MIN_PROB)
    assert proba.shape == (len(f), 2) and proba.dtype == np.float64
    assert (np.abs(proba.sum(axis=1) - 1.0) <= P.U52).all()
    # column 0 is clipped to libsvm's [min_prob, 1 - min_prob]; column 1 is 1 - column 0, one rounding of that subtraction (2^-53 at
    # most: the operands lie in [0, 1]) from the same interval -- 1 - fl(1 - 1e-7) is 9.99999999e-08, which is what libsvm returns too
    assert (proba[:, 0] >= P.MIN_PROB).all() and (proba[:, 0] <= 1.0 - P.MIN_PROB).all()
    assert (proba[:, 1] >= P.MIN_PROB - P.U52 / 2).all() and (proba[:, 1] <= 1.0 - P.MIN_PROB + P.U52 / 2).all()
    assert (np.abs(proba[:, 0] - want) <= (np.abs(z) + 4.0) * P.U52 * want).all()
    assert np.array_equal(proba[:, 1], 1.0 - proba[:, 0])
    order = np.argsort(z, kind="stable")
    assert (np.diff(proba[order, 0]) <= 0.0).all(), "the probability of classes_[0] is not monotone in the decision value"


def test_predict_proba(dev):
    X, y, clf = _fitted()
    A, B = clf.probA_[0], clf.probB_[0]
    assert clf.platt_status_ == 0 and A < 0.0                  # a larger libsvm decision value means classes_[0]
    Q, _ = O.make_data(65, 17, 0.7, 5)
    for m in (0, 1, 65):
        got = clf.predict_proba(Q[:m])
        assert isinstance(got, np.ndarray)
        _check_proba(got, -clf.decision_function(Q[:m]), A, B)
        on_dev = clf.predict_proba(torch.from_numpy(Q[:m]).cuda())
        assert on_dev.is_cuda and on_dev.dtype == torch.float64 and np.array_equal(on_dev.cpu().numpy(), got)
        assert np.array_equal(clf.predict_log_proba(Q[:m]), np.log(got))
        assert clf.predict_log_proba(torch.from_numpy(Q[:m]).cuda()).is_cuda
    # the labels follow the sign of the decision value, and on clear rows so do the probabilities
    got, dec = clf.predict_proba(Q), clf.decision_function(Q)
    assert np.array_equal(clf.predict(Q), clf.classes_[(dec > 0).astype(int)])
    assert (got[dec > 1.0, 1] > 0.5).all() and (got[dec < -1.0, 0] > 0.5).all()
    # the entry point on its own, where the clip and both branches of the sigmoid act
    f = np.r_[-1e3, -40.0, -17.0, -1.0, -0.1, 0.0, 0.1, 1.0, 17.0, 40.0, 1e3, np.linspace(-20, 20, 300)]
    fd = torch.from_numpy(f).cuda()
    out = torch.empty((len(f), 2), dtype=torch.float64, device="cuda")
    for a, b in ((-1.0, 0.1), (2.5, -0.3), (0.0, 0.0)):
        _lib.check(_lib.lib().bbbp_svm_platt_proba(torch.cuda.current_stream().cuda_stream, fd.data_ptr(), len(f), a, b, out.data_ptr()), "proba")
        _check_proba(out.cpu().numpy(), f, a, b)
    assert out[0, 0].item() == 0.5


@functools.lru_cache(maxsize=None)
def _sklearn_oof_family(n, d, sep, kind, C):
    """The oracle: scikit-learn fitted per fold on the folds of platt_folds(n, 5, 0), minus its decision values on the held-out rows, then
    the restatement -- for the four fits of svc_oracle.sklearn_reference's family (shrinking off and on, rows in order and reversed)."""
    from sklearn.svm import SVC as SkSVC
    X, y = O.make_data(n, d, sep, 1)
    g = O.gamma_scale(X)
    ys = np.where(y == np.unique(y)[0], 1.0, -1.0)
    held = platt_folds(n, 5, 0)
    oofs = []
    for sh in (False, True):
        for step in (1, -1):
            oof = np.empty(n)
            for te in held:
                tr = np.setdiff1d(np.arange(n), te)[::step]
                oof[te] = -SkSVC(C=C, kernel=kind, gamma=g, tol=1e-3, shrinking=sh).fit(X[tr], y[tr]).decision_function(X[te])
            oofs.append(oof)
    return X, y, ys, held, np.array(oofs), [P.sigmoid_train(oof, ys) for oof in oofs]


@pytest.mark.parametrize("n,d,sep,kind,C", [(200, 10, 0.7, "rbf", 1.0), (333, 100, 0.5, "rbf", 10.0), (200, 10, 0.7, "linear", 1.0)])
def test_plattsvc_against_sklearn_with_the_same_folds(dev, n, d, sep, kind, C):
    """Tolerances come from the reference alone.  Decision values: 4 x the spread of the family's out-of-fold values, at least 10 tol
    (svc_oracle.sklearn_reference gives the reason).  (A, B): 4 x the spread of the family's (A, B), and at least that decision tolerance
    delta carried through the restatement's linearisation, |d theta| <= |H^-1| sum_i |dg / df_i| delta with
    dg_A / df_i = (t_i - p_i) + A f_i p_i q_i and dg_B / df_i = A p_i q_i."""
    X, y, ys, held, oofs, fits = _sklearn_oof_family(n, d, sep, kind, C)
    assert all(f[3] == P.CONVERGED for f in fits)
    clf = PlattSVC(C=C, kernel=kind, cv=5, random_state=0).fit(X, y)
    assert all(np.array_equal(np.sort(a), np.sort(b[1])) for a, b in zip(held, clf._folds))
    delta = max(4.0 * float((oofs.max(axis=0) - oofs.min(axis=0)).max()), 10.0 * 1e-3)
    thetas = np.array([[f[0], f[1]] for f in fits])
    spread = float(np.linalg.norm(thetas.max(axis=0) - thetas.min(axis=0)))
    a, b, _, _, _, H = fits[0]
    t, _, _ = P.targets(ys)
    p, q = P.p_q(oofs[0], a, b)
    carried = float(np.linalg.norm(np.linalg.inv(H), 2)) * float(np.hypot((t - p) + a * oofs[0] * p * q, a * p * q).sum()) * delta
    tolerance = max(4.0 * spread, carried)
    diff_dec = float(np.abs(clf.oof_decision_ - oofs[0]).max())
    diff = float(np.hypot(clf.probA_[0] - a, clf.probB_[0] - b))
    print(f"n {n} d {d} {kind} C {C}: A {clf.probA_[0]:.6g} B {clf.probB_[0]:.6g} (oracle {a:.6g} {b:.6g}); decision tolerance {delta:.3g}, "
          f"largest difference {diff_dec:.3g}; (A, B) tolerance {tolerance:.3g} (family spread {spread:.3g}, carried {carried:.3g}), difference {diff:.3g}")
    assert clf.platt_status_ == 0 and clf.probA_.shape == clf.probB_.shape == (1,)
    assert diff_dec <= delta
    assert diff <= tolerance
    # the device's own calibration of its own out-of-fold values is the restatement's, within the convexity bound
    a2, b2, _, st2, _, H2 = P.sigmoid_train(clf.oof_decision_, ys)
    assert st2 == P.CONVERGED and diff <= tolerance
    assert np.hypot(clf.probA_[0] - a2, clf.probB_[0] - b2) <= theta_bound(clf.oof_decision_, ys, (clf.probA_[0], clf.probB_[0]), (a2, b2), H2)


def test_labels_of_any_kind_and_the_default_folds(dev):
    X, y = O.make_data(130, 17, 0.7, 4)
    labels = np.where(y > 0, "pos", "neg")
    a = PlattSVC().fit(X, y)
    b = PlattSVC().fit(torch.from_numpy(X).cuda(), labels)
    c = PlattSVC(cv=5, random_state=0).fit(X, y, folds=platt_folds(130, 5, 0))
    assert list(b.classes_) == ["neg", "pos"] and np.isfinite(a.oof_decision_).all() and a.platt_status_ == 0 and a.platt_n_iter_ > 0
    for other in (b, c):
        assert np.array_equal(a.oof_decision_, other.oof_decision_) and a.probA_[0] == other.probA_[0] and a.probB_[0] == other.probB_[0]
        assert np.array_equal(a.alpha_, other.alpha_) and (a.platt_n_iter_, a.platt_status_) == (other.platt_n_iter_, other.platt_status_)
        assert np.array_equal(a.predict_proba(X), other.predict_proba(X))
    assert np.array_equal(b.predict(X) == "pos", a.predict(X) > 0)
    seeded = PlattSVC(random_state=1).fit(X, y)
    assert not np.array_equal(seeded.oof_decision_, a.oof_decision_) and np.array_equal(seeded.alpha_, a.alpha_)
    # out-of-fold values separate the classes about as the fit does: positive towards classes_[0]
    ys = np.where(y == a.classes_[0], 1.0, -1.0)
    assert (np.sign(a.oof_decision_) == ys).mean() > 0.8
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a.predict_proba(torch.zeros(2, 17))
