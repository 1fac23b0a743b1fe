"""CPU: the numpy restatement of the classifier stack (tests/ensemble_numpy.py) against scikit-learn's own ``StackingClassifier`` and
``VotingClassifier`` on deterministic scikit-learn base learners, bit for bit; then what of ``bbbp_amd.ensemble``, ``mlp.MLPClassifier`` and the
learners' new ``get_params`` / ``set_params`` needs no GPU: the argument checks and the round trips."""
import functools

import numpy as np
import pytest
import sklearn.ensemble as ske
from sklearn.base import clone
from sklearn.linear_model import LogisticRegression
from sklearn.naive_bayes import BernoulliNB
from sklearn.neighbors import KNeighborsClassifier
from sklearn.svm import SVC
from sklearn.tree import DecisionTreeClassifier

import ensemble_numpy as R
from bbbp_amd import ensemble, gradient_boosting, linear_model, mlp, naive_bayes, neighbors, random_forest, svm

N, D = 120, 7
ROWS = (1, 2, 123)
COUNTS = (1, 2, 3, 8, 9, 17)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(R.bits(a), R.bits(b))


@functools.lru_cache(maxsize=None)
def _problem(seed=0):
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(N, D))
    y = (X[:, 0] + 0.8 * X[:, 1] * X[:, 2] + 0.7 * rs.normal(size=N) > 0.2).astype(np.int64)
    Xq = rs.normal(size=(max(ROWS), D))
    return X, y, Xq


def _base():
    """The deterministic learners: four with ``predict_proba`` and ``SVC()`` for the ``decision_function`` route."""
    return [("knn", KNeighborsClassifier(3)), ("bnb", BernoulliNB()), ("lr", LogisticRegression()), ("tree", DecisionTreeClassifier(random_state=0)),
            ("svc", SVC())]


def _many(M):
    """M learners with ``predict_proba`` whose columns differ: the four kinds repeated with other parameters."""
    makers = [lambda i: KNeighborsClassifier(3 + 2 * i), lambda i: BernoulliNB(alpha=1.0 + i, binarize=0.1 * i),
              lambda i: LogisticRegression(C=1.0 / (1 + i)), lambda i: DecisionTreeClassifier(max_depth=2 + i, random_state=0)]
    return [(f"e{j}", makers[j % 4](j // 4)) for j in range(M)]


def _final():
    return ske.GradientBoostingClassifier(n_estimators=5, random_state=0)


@functools.lru_cache(maxsize=None)
def _stack(labels="int", passthrough=False, explicit=False):
    X, y, _ = _problem()
    y = {"int": y, "str": np.where(y == 1, "pos", "neg"), "pm1": 2 * y - 1}[labels]
    cv = R.folds(R.encode(y)[1], 4)[::-1] if explicit else 5
    cv = [(tr[::-1].copy(), te) for tr, te in cv] if explicit else cv
    sk = ske.StackingClassifier(_base(), final_estimator=_final(), cv=cv, passthrough=passthrough).fit(X, y)
    return sk, y, cv


# ---- stacking -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["int", "str", "pm1"])
def test_encoded_labels_and_stack_methods_are_scikit_learns(labels):
    sk, y, _ = _stack(labels)
    classes, t = R.encode(y)
    assert np.array_equal(classes, sk.classes_) and classes.dtype == sk.classes_.dtype
    assert np.array_equal(t, sk._label_encoder.transform(y)) and set(t) == {0, 1}
    assert [R.resolve_stack_method(est) for _, est in _base()] == sk.stack_method_ == ["predict_proba"] * 4 + ["decision_function"]
    assert all(np.array_equal(est.classes_, [0, 1]) for est in sk.estimators_), "scikit-learn fits the base learners on the encoded labels"


@pytest.mark.parametrize("passthrough", [False, True])
def test_transform_equals_the_full_fit_columns_bit_for_bit(passthrough):
    sk, _, _ = _stack(passthrough=passthrough)
    X, _, Xq = _problem()
    for Z in (X, Xq, Xq[:1]):
        got = R.transform(sk.estimators_, sk.stack_method_, Z, passthrough)
        assert got.shape == (len(Z), 5 + (D if passthrough else 0)) and _same(got, sk.transform(Z))
    # the columns are the learners' own: P(classes_[1]) and the decision values
    assert _same(R.transform(sk.estimators_, sk.stack_method_, Xq)[:, 2], sk.estimators_[2].predict_proba(Xq)[:, 1])
    assert _same(R.transform(sk.estimators_, sk.stack_method_, Xq)[:, 4], sk.estimators_[4].decision_function(Xq))


@pytest.mark.parametrize("labels,passthrough,explicit", [("int", False, False), ("str", False, False), ("pm1", False, False), ("int", True, False),
                                                         ("int", False, True)])
def test_final_estimator_on_the_restated_oof_has_scikit_learns_decision_function(labels, passthrough, explicit):
    sk, y, cv = _stack(labels, passthrough, explicit)
    X, _, Xq = _problem()
    classes, t = R.encode(y)
    pairs = R.folds(t, cv)
    assert sorted(np.concatenate([te for _, te in pairs]).tolist()) == list(range(N))
    meta = R.oof([est for _, est in _base()], X, t, pairs, sk.stack_method_, clone)
    assert meta.shape == (N, 5) and meta.dtype == np.float64 and not np.isnan(meta).any()
    if passthrough:
        meta = np.hstack([meta, X])
    final = clone(_final()).fit(meta, t)
    for Z in (X, Xq):
        cols = R.transform(sk.estimators_, sk.stack_method_, Z, passthrough)
        assert _same(final.decision_function(cols), sk.final_estimator_.decision_function(cols))
        assert _same(final.decision_function(cols), sk.decision_function(Z))
        assert np.array_equal(classes[final.predict(cols)], sk.predict(Z))
    assert not _same(meta[:, :5], R.transform(sk.estimators_, sk.stack_method_, X)), "out-of-fold columns must differ from the full fits' own"


def test_folds_are_checked():
    t = R.encode(_problem()[1])[1]
    pairs = R.folds(t, 5)
    assert len(pairs) == 5 and all(len(np.intersect1d(tr, te)) == 0 for tr, te in pairs)
    with pytest.raises(ValueError, match="partition"):
        R.folds(t, pairs[:4])
    with pytest.raises(ValueError, match="partition"):
        R.folds(t, pairs + pairs[:1])
    with pytest.raises(ValueError, match="leaves"):
        R.folds(t, [(pairs[0][0], pairs[0][1] + N)] + pairs[1:])


# ---- voting -------------------------------------------------------------------------------------------------------------------------------
def _weights(kind, M):
    if kind is None:
        return None
    rs = np.random.RandomState(1100 + M)                # at M = 8 and M = 17 these float weights sum to other bits one after the other than pairwise
    return rs.randint(1, 6, M).tolist() if kind == "int" else rs.uniform(0.1, 2.0, M).tolist()


@functools.lru_cache(maxsize=None)
def _voter(M, voting):
    X, y, _ = _problem()
    return ske.VotingClassifier(_many(M), voting=voting).fit(X, y)


@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("kind", [None, "int", "float"])
def test_soft_vote_is_scikit_learns_bit_for_bit(M, kind):
    sk = _voter(M, "soft")
    Xq = _problem()[2]
    sk.weights = _weights(kind, M)
    for m in ROWS:
        probas = [est.predict_proba(Xq[:m]) for est in sk.estimators_]
        avg, label = R.soft_vote(probas, sk.weights)
        assert avg.shape == (m, 2) and _same(avg, sk.predict_proba(Xq[:m]))
        assert np.array_equal(sk.classes_[label], sk.predict(Xq[:m]))


@pytest.mark.parametrize("M", [8, 17])
def test_a_sequential_sum_of_the_weights_gives_other_bits(M):
    """Why the sum of the weights is numpy's own and reaches the kernel as one double: from eight weights on numpy adds them pairwise."""
    sk = _voter(M, "soft")
    Xq = _problem()[2]
    sk.weights = _weights("float", M)
    sequential = 0.0
    for w in sk.weights:
        sequential += w
    assert sequential != R.scale(sk.weights)
    probas = [est.predict_proba(Xq) for est in sk.estimators_]
    assert not _same(R.soft_vote(probas, sk.weights, sequential_scale=True)[0], sk.predict_proba(Xq))
    assert _same(R.soft_vote(probas, sk.weights)[0], sk.predict_proba(Xq))


@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("kind", [None, "int", "float"])
def test_hard_vote_is_scikit_learns(M, kind):
    sk = _voter(M, "hard")
    Xq = _problem()[2]
    sk.weights = _weights(kind, M)
    for m in ROWS:
        preds = np.stack([est.predict(Xq[:m]) for est in sk.estimators_])
        assert _same(preds.T, sk.transform(Xq[:m]))
        counts, label = R.hard_vote(preds, sk.weights)
        assert np.array_equal(sk.classes_[label], sk.predict(Xq[:m]))
        for i in range(m):
            want = np.bincount(preds[:, i], weights=sk.weights, minlength=2).astype(np.float64)
            assert _same(counts[i], want)


def test_hard_vote_ties_go_to_the_first_class():
    tied = 0
    for M in (2, 8):
        sk = _voter(M, "hard")
        sk.weights = None
        Xq = _problem()[2]
        preds = np.stack([est.predict(Xq) for est in sk.estimators_])
        counts, label = R.hard_vote(preds)
        ties = counts[:, 0] == counts[:, 1]
        tied += int(ties.sum())
        assert (label[ties] == 0).all() and np.array_equal(sk.classes_[label], sk.predict(Xq))
    assert tied > 0, "no tie among the rows: the tie rule would go unchecked"


def test_soft_vote_ties_and_nan_follow_argmax():
    p = np.array([[0.5, 0.5], [0.25, 0.75], [np.nan, 0.5], [0.5, np.nan], [np.nan, np.nan]])
    avg, label = R.soft_vote([p, p])
    assert np.array_equal(label, np.argmax(avg, axis=1))
    assert label.tolist() == [0, 1, 0, 1, 0]


@pytest.mark.parametrize("flatten", [True, False])
def test_voting_transform_shapes(flatten):
    X, y, Xq = _problem()
    sk = ske.VotingClassifier(_many(3), voting="soft", flatten_transform=flatten).fit(X, y)
    probas = [est.predict_proba(Xq) for est in sk.estimators_]
    assert _same(np.hstack(probas) if flatten else np.stack(probas), sk.transform(Xq))


# ---- what of the package needs no GPU: argument checks --------------------------------------------------------------------------------------
def _ours():
    return [("knn", neighbors.KNeighborsClassifier(3)), ("lr", linear_model.LogisticRegression()), ("bnb", naive_bayes.BernoulliNB())]


@pytest.mark.parametrize("cls", [ensemble.StackingClassifier, ensemble.VotingClassifier])
def test_ensembles_refuse_by_name(cls):
    X, y, _ = _problem()
    with pytest.raises(NotImplementedError, match="n_jobs"):
        cls(_ours(), n_jobs=2)
    cls(_ours(), n_jobs=1), cls(_ours(), n_jobs=None)
    with pytest.raises(NotImplementedError, match="drop"):
        cls(_ours()[:2] + [("bnb", "drop")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cls(_ours(), device="cpu")
    with pytest.raises(ValueError, match="non-empty"):
        cls([])
    with pytest.raises(ValueError, match="distinct"):
        cls(_ours() + _ours()[:1])
    with pytest.raises(TypeError, match="needs fit"):
        cls(_ours() + [("x", object())])
    with pytest.raises(NotImplementedError, match="sample_weight"):
        cls(_ours()).fit(X, y, sample_weight=np.ones(N))
    with pytest.raises(NotImplementedError, match="3 classes"):
        cls(_ours()).fit(X, np.arange(N) % 3)
    with pytest.raises(RuntimeError, match="not fitted"):
        cls(_ours()).predict(X)


def test_stacking_refuses_by_name():
    S = ensemble.StackingClassifier
    with pytest.raises(NotImplementedError, match="cv='prefit'"):
        S(_ours(), cv="prefit")
    from sklearn.model_selection import KFold
    with pytest.raises(NotImplementedError, match="cv="):
        S(_ours(), cv=KFold(3))
    with pytest.raises(NotImplementedError, match="cv="):
        S(_ours(), cv=None)
    with pytest.raises(ValueError, match="at least 2"):
        S(_ours(), cv=1)
    with pytest.raises(ValueError, match="stack_method"):
        S(_ours(), stack_method="score")
    with pytest.raises(ValueError, match="passthrough"):
        S(_ours(), passthrough=1)
    with pytest.raises(TypeError, match="final_estimator"):
        S(_ours(), final_estimator=object())
    t = R.encode(_problem()[1])[1]
    pairs = R.folds(t, 3)
    assert [te.tolist() for _, te in ensemble._folds(3, t, "x")] == [te.tolist() for _, te in pairs]
    assert [tr.tolist() for tr, _ in ensemble._folds(pairs, t, "x")] == [tr.tolist() for tr, _ in pairs]
    with pytest.raises(ValueError, match="partition"):
        ensemble._folds(pairs[:2], t, "x")
    s = S(_ours(), gradient_boosting.GradientBoostingClassifier(5, 0.1, 3), cv=pairs, passthrough=True)
    assert s.get_params()["cv"] is pairs and s.set_params(cv=4).cv == 4
    with pytest.raises(NotImplementedError, match="prefit"):
        s.set_params(cv="prefit")
    assert s.cv == 4


def test_voting_refuses_by_name():
    V = ensemble.VotingClassifier
    with pytest.raises(ValueError, match="Voting must be 'soft' or 'hard'"):
        V(_ours(), voting="mean")
    with pytest.raises(ValueError, match="must be equal"):
        V(_ours(), weights=[1, 2])
    with pytest.raises(ValueError, match="finite"):
        V(_ours(), weights=[1, np.nan, 2])
    with pytest.raises(ZeroDivisionError):
        V(_ours(), weights=[1, -1, 0])
    with pytest.raises(ValueError, match="flatten_transform"):
        V(_ours(), flatten_transform="yes")
    with pytest.raises(TypeError, match="verbose"):
        V(_ours(), verbose=True)                         # not a parameter here: nothing is accepted and dropped
    with pytest.raises(TypeError, match="verbose"):
        ensemble.StackingClassifier(_ours(), verbose=1)
    v = V(_ours(), voting="soft", weights=[1, 2, 3])
    assert v.get_params()["weights"] == [1, 2, 3] and v.set_params(weights=None).weights is None
    w, scl = ensemble._check_weights([0.1] * 8, 8, "x")
    assert scl == np.asarray([0.1] * 8).sum() != sum([0.1] * 8), "the sum is numpy's pairwise one"
    assert ensemble._resolve_stack_method(SVC(), "auto", "svc", "x") == "decision_function"
    with pytest.raises(ValueError, match="does not implement"):
        ensemble._resolve_stack_method(SVC(), "predict_proba", "svc", "x")


def test_encode_is_the_restatements():
    for y in (_problem()[1], np.where(_problem()[1] == 1, "pos", "neg"), 2 * _problem()[1] - 1, _problem()[1].astype(np.float32)):
        got, want = ensemble._encode(y, "x"), R.encode(y)
        assert np.array_equal(got[0], want[0]) and got[0].dtype == want[0].dtype and _same(got[1], want[1])


def test_kernel_entries_validate_their_arguments_before_touching_the_gpu():
    import ctypes
    from bbbp_amd import _lib
    L = _lib.lib()
    ERR_ARG, fake = 1, 4096                              # never dereferenced: validation comes first
    col = (_lib.EnsColumn * 1)(_lib.EnsColumn(fake, 2, 1))
    out = ctypes.c_void_p(fake)
    assert L.bbbp_ens_soft_vote(None, col, fake, 1, None, 0.0, 5, out, out) == ERR_ARG and b"stride" in L.bbbp_last_error()
    col[0].col = 0
    assert L.bbbp_ens_soft_vote(None, col, fake, 0, None, 0.0, 5, out, out) == ERR_ARG and b"n_estimators" in L.bbbp_last_error()
    assert L.bbbp_ens_soft_vote(None, col, None, 1, None, 0.0, 5, out, out) == ERR_ARG
    assert L.bbbp_ens_soft_vote(None, col, fake, 1, None, 0.0, -1, out, out) == ERR_ARG
    assert L.bbbp_ens_soft_vote(None, col, fake, 1, None, 0.0, 5, None, out) == ERR_ARG
    assert L.bbbp_ens_soft_vote(None, col, fake, 1, None, 0.0, 0, None, None) == 0          # no rows: nothing to do
    col[0].stride = 0
    assert L.bbbp_ens_hard_vote(None, col, fake, 1, None, 5, out, out) == ERR_ARG
    col[0].stride, col[0].src = 1, None
    assert L.bbbp_ens_hard_vote(None, col, fake, 1, None, 5, out, out) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_ens_hard_vote(None, col, fake, 1, None, 0, None, None) == 0
    rows = (ctypes.c_long * 3)(0, 2, 1)
    src = (_lib.EnsSource * 1)(_lib.EnsSource(fake, 1, 0, fake, 3, 0))
    for change, word in ((dict(stride=0), b"stride"), (dict(dst=1), b"destination"), (dict(count=4), b"count"), (dict(src=None), b"null")):
        bad = (_lib.EnsSource * 1)(_lib.EnsSource(fake, 1, 0, fake, 3, 0))
        for k, v in change.items():
            setattr(bad[0], k, v)
        assert L.bbbp_ens_meta_scatter(None, bad, fake, 1, rows, 3, 1, out, 1) == ERR_ARG and word in L.bbbp_last_error()
    assert L.bbbp_ens_meta_scatter(None, src, fake, 1, None, 3, 1, out, 1) == ERR_ARG
    assert L.bbbp_ens_meta_scatter(None, src, fake, 1, rows, 3, 1, out, 0) == ERR_ARG and b"leading" in L.bbbp_last_error()
    for ids, word in (((0, 3, 1), b"outside"), ((0, 0, 1), b"twice"), ((0, -1, 1), b"outside")):
        assert L.bbbp_ens_meta_scatter(None, src, fake, 1, (ctypes.c_long * 3)(*ids), 3, 1, out, 1) == ERR_ARG and word in L.bbbp_last_error()
    src[0].count = 2
    assert L.bbbp_ens_meta_scatter(None, src, fake, 1, rows, 3, 1, out, 1) == ERR_ARG and b"never" in L.bbbp_last_error()
    assert L.bbbp_ens_meta_scatter(None, src, fake, 0, rows, 3, 1, out, 1) == ERR_ARG


# ---- mlp.MLPClassifier and the learners' parameter methods --------------------------------------------------------------------------------
def test_mlp_classifier_refuses_what_the_trainer_does_not_implement():
    M = mlp.MLPClassifier
    for kw, word in ((dict(solver="sgd"), "solver"), (dict(solver="lbfgs"), "solver"), (dict(activation="logistic"), "activation"),
                     (dict(hidden_layer_sizes=(10, 10, 10, 10)), "hidden_layer_sizes"), (dict(hidden_layer_sizes=(300,)), "hidden_layer_sizes"),
                     (dict(early_stopping=True), "early_stopping"), (dict(warm_start=True), "warm_start"), (dict(shuffle=False), "shuffle"),
                     (dict(beta_1=0.8), "beta_1"), (dict(random_state=None), "random_state"), (dict(learning_rate="adaptive"), "learning_rate")):
        with pytest.raises(NotImplementedError, match=word):
            M(**kw)
    for kw in (dict(batch_size=0), dict(batch_size="all"), dict(alpha=-1.0), dict(learning_rate_init=0.0), dict(max_iter=0), dict(tol=float("nan")),
               dict(momentum_decay=1)):
        with pytest.raises(ValueError):
            M(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M(device="cpu")
    X, y, _ = _problem()
    with pytest.raises(NotImplementedError, match="sample_weight"):
        M().fit(X, y, sample_weight=np.ones(N))
    with pytest.raises(RuntimeError, match="not fitted"):
        M().predict_proba(X)
    est = M((20, 10), "tanh", batch_size=32, max_iter=7, random_state=3)
    cfg = est._config(96, np.arange(96))
    assert (cfg.hidden_layer_sizes, cfg.activation, cfg.batch_size, cfg.max_iter, cfg.random_state) == ((20, 10), "tanh", 32, 7, 3)
    assert M()._config(96).batch_size == 96 and M()._config(6246).batch_size == 200 and M(50)._config(10).hidden_layer_sizes == (50,)


ESTIMATORS = [
    (neighbors.KNeighborsClassifier, dict(n_neighbors=3, weights="distance"), dict(n_neighbors=7), dict(n_neighbors=0)),
    (linear_model.LogisticRegression, dict(C=0.5, max_iter=50), dict(C=2.0), dict(C=-1.0)),
    (svm.SVC, dict(C=2.0, kernel="linear"), dict(gamma=0.5), dict(kernel="sigmoid")),
    (random_forest.RandomForestClassifier, dict(n_estimators=5, max_depth=4, random_state=7), dict(min_samples_leaf=2), dict(n_estimators=0)),
    (random_forest.DecisionTreeClassifier, dict(max_depth=3), dict(min_samples_split=5), dict(max_depth=0)),
    (gradient_boosting.GradientBoostingClassifier, dict(n_estimators=5, learning_rate=0.2, max_depth=2), dict(n_estimators=9), dict(max_depth=99)),
    (mlp.MLPClassifier, dict(hidden_layer_sizes=(8,), max_iter=5), dict(activation="tanh"), dict(solver="sgd")),
    (naive_bayes.BernoulliNB, dict(alpha=0.5), dict(binarize=0.25), dict(alpha=-1.0)),
    (svm.PlattSVC, dict(C=2.0), dict(cv=3), dict(cv=1)),
]


@pytest.mark.parametrize("cls,kw,change,bad", ESTIMATORS, ids=[e[0].__name__ for e in ESTIMATORS])
def test_get_params_and_set_params_round_trip(cls, kw, change, bad):
    est = cls(**kw)
    params = est.get_params()
    assert params == est.get_params(deep=True) == est.get_params(deep=False) and "device" in params
    assert all(params[k] == v for k, v in kw.items())
    twin = ensemble._clone(est)
    assert type(twin) is cls and twin is not est and twin.get_params() == params
    assert est.set_params(**change) is est and all(est.get_params()[k] == v for k, v in change.items())
    assert all(est.get_params()[k] == v for k, v in kw.items() if k not in change), "set_params changed a parameter it was not given"
    with pytest.raises((ValueError, NotImplementedError)):
        est.set_params(**bad)
    assert all(est.get_params()[k] == v for k, v in change.items()), "a refused set_params left its value behind"
    with pytest.raises(ValueError, match="unknown"):
        est.set_params(no_such_parameter=1)
    assert ensemble._batched_path(est) == {"KNeighborsClassifier": None, "SVC": None, "PlattSVC": None, "LogisticRegression": "linear_model._solve",
                                           "RandomForestClassifier": "random_forest._grow", "DecisionTreeClassifier": "random_forest._grow",
                                           "GradientBoostingClassifier": "gradient_boosting._fit_chains", "MLPClassifier": "GridMLPTrainer.fit",
                                           "BernoulliNB": "naive_bayes.fit_masks"}[cls.__name__]


def test_a_subclass_with_its_own_fit_is_looped_through_that_fit():
    class Mine(linear_model.LogisticRegression):
        def fit(self, X, y, sample_weight=None):
            return super().fit(X, y)

    class Same(linear_model.LogisticRegression):
        pass

    assert ensemble._batched_path(Mine()) is None and ensemble._batched_path(Same()) == "linear_model._solve"
