"""GPU: the three entries of ``csrc/ensemble.hip`` against the numpy restatement (tests/ensemble_numpy.py), bit for bit, at the shapes where
they can go wrong, and the whole classifier stack on this package's eight learners at their smallest: the batched fits of
``ensemble.fit_classifier_stack`` against one-at-a-time fits assembled by the restatement.

Shapes: 63 / 64 / 65 rows lie around one wave, 257 rows need a second block of 256 lanes, 0 and 1 are the ends; 1, 2, 8 and 9 estimators
are the single term, the first sum, and the counts around which numpy's own sum of the weights turns pairwise."""
import functools
import warnings

import numpy as np
import pytest
import torch

import ensemble_numpy as R
from bbbp_amd import ensemble, gradient_boosting, linear_model, mlp, naive_bayes, neighbors, random_forest, svm

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 63, 64, 65, 257)
COUNTS = (1, 2, 8, 9)


def _same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(R.bits(a), R.bits(b))


def _weights(M, seed=0):
    """Non-dyadic weights: every product with a probability rounds."""
    return np.random.RandomState(1100 + M + seed).uniform(0.1, 2.0, M)


def _placed(values, layout, dev, width):
    """``values`` [m, width] on the device in one of the layouts a learner hands over: (tensor, column).  0: the last ``width`` columns of a
    dense [m, width + 1] (column 1 of [m, 2] for a meta column); 1: a dense [m, width] (column 0 of [m, 1]); 2: columns 3 .. of a
    row-strided view, five columns wide, into a matrix of eight."""
    m = len(values)
    values = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
    fill = 7 if values.dtype == torch.uint8 else float("nan")
    if layout == 0:
        t = torch.full((m, width + 1), fill, dtype=values.dtype, device=dev)
        t[:, 1:] = values
        return t, 1
    if layout == 1:
        return values.clone(), 0
    big = torch.full((m, 8), fill, dtype=values.dtype, device=dev)
    view = big[:, 2:7]
    view[:, 3:3 + width] = values
    return view, 3


def _interleaved_folds(m, n_folds=3):
    """Test parts of unequal size with interleaved row ids: row i goes to fold min(i % 4, 2), so the last part is twice the others; some are
    empty for small m."""
    ids = np.arange(m)
    fold = np.minimum(ids % (n_folds + 1), n_folds - 1)
    parts = [ids[fold == f][::-1].copy() if f == 1 else ids[fold == f] for f in range(n_folds)]          # one part in descending order
    assert m < 9 or len({len(p) for p in parts}) > 1
    return parts


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("m", ROWS)
def test_meta_scatter_assembles_the_out_of_fold_matrix(dev, m, M):
    rs = np.random.RandomState(10 * m + M)
    parts = _interleaved_folds(m)
    want = np.full((m, M), np.nan)
    entries = []
    for j in range(M):
        for f, rows in enumerate(parts):
            col = rs.normal(size=len(rows))
            want[rows, j] = col
            src, c = _placed(col[:, None], (j + f) % 3, dev, 1)
            entries.append((src, c, rows, j))
    before = ensemble._LAUNCHES["meta_scatter"]
    meta = torch.full((m, M + 2), -7.0, dtype=torch.float64, device=dev)          # two passthrough columns behind the M: not the kernel's
    ensemble._meta_scatter(entries, meta, M)
    assert ensemble._LAUNCHES["meta_scatter"] - before == (1 if m else 0), "one launch, however many estimators and folds"
    assert _same(meta[:, :M].contiguous(), want) and bool((meta[:, M:] == -7.0).all())
    # transform: the same entry with identity rows, 1-D sources
    cols = [rs.normal(size=m) for _ in range(M)]
    flat = torch.empty((m, M), dtype=torch.float64, device=dev)
    ensemble._meta_scatter([(torch.from_numpy(c).to(dev), 0, None, j) for j, c in enumerate(cols)], flat, M)
    assert _same(flat, np.stack(cols, axis=1).reshape(m, M))


def test_meta_scatter_refuses_row_ids_that_are_no_partition(dev):
    src = torch.zeros(4, dtype=torch.float64, device=dev)
    meta = torch.empty((4, 1), dtype=torch.float64, device=dev)
    for rows, word in (([0, 1, 2, 4], "outside"), ([0, 1, 1, 3], "twice"), ([0, 1, 2, -1], "outside")):
        with pytest.raises(RuntimeError, match=word):
            ensemble._meta_scatter([(src, 0, np.array(rows), 0)], meta, 1)
    with pytest.raises(RuntimeError, match="never"):
        ensemble._meta_scatter([(src[:3], 0, np.array([0, 1, 2]), 0)], meta, 1)


def _probas(m, M, seed):
    """M probability pairs per row; the first rows tie exactly: 0.5 / 0.5 everywhere, and mirrored pairs that average to a tie."""
    rs = np.random.RandomState(seed)
    p1 = rs.uniform(size=(M, m))
    P = np.stack([1.0 - p1, p1], axis=2)
    if m > 2:
        P[:, 0] = 0.5
        if M % 2 == 0:
            P[0::2, 1], P[1::2, 1] = (0.25, 0.75), (0.75, 0.25)
    return P


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("m", ROWS)
def test_soft_vote_is_the_restatement_bit_for_bit(dev, m, M, weighted):
    P = _probas(m, M, 100 * m + M)
    w = _weights(M) if weighted else None
    want, want_label = R.soft_vote(list(P), w)
    placed = [_placed(P[j], j % 3, dev, 2) for j in range(M)]
    before = ensemble._LAUNCHES["soft_vote"]
    avg, label = ensemble._soft_vote([t for t, _ in placed], w, None if w is None else R.scale(w), [c for _, c in placed])
    assert ensemble._LAUNCHES["soft_vote"] - before == (1 if m else 0)
    assert _same(avg, want.reshape(m, 2)) and _same(label, want_label.reshape(m))
    if m > 2 and not weighted:
        assert want[0, 0] == want[0, 1] and want_label[0] == 0, "the tie row does not tie"
        if M % 2 == 0:
            assert want[1, 0] == want[1, 1] and want_label[1] == 0


@pytest.mark.parametrize("M", [2, 8, 9])
def test_contraction_canary_a_fused_multiply_add_would_change_the_vote_bits(dev, M):
    """Precondition: on these inputs fusing ``s + P_j * w_j`` into one rounding changes bits of the weighted average, so bit equality of
    the GPU result shows that the kernel does not contract them."""
    P, w = _probas(65, M, 7), _weights(M)
    want, _ = R.soft_vote(list(P), w)
    fused, _ = R.soft_vote(list(P), w, fused=True)
    assert (R.bits(fused) != R.bits(want)).any() and np.abs(fused - want).max() <= M * 2.0 ** -51          # a step differs by under an ulp of the running sum
    avg, _ = ensemble._soft_vote([torch.from_numpy(p).to(dev) for p in P], w, R.scale(w))
    assert _same(avg, want)


def test_soft_vote_takes_numpys_sum_of_the_weights(dev):
    """At eight weights numpy's sum is pairwise: the kernel divides by the double it is given and does not add the weights again."""
    w = _weights(8)
    sequential = 0.0
    for v in w:
        sequential += v
    assert sequential != R.scale(w)
    P = _probas(65, 8, 3)
    want, _ = R.soft_vote(list(P), w)
    assert not _same(R.soft_vote(list(P), w, sequential_scale=True)[0], want)
    assert _same(ensemble._soft_vote([torch.from_numpy(p).to(dev) for p in P], w, R.scale(w))[0], want)
    assert ensemble._check_weights(w.tolist(), 8, "x")[1] == R.scale(w)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("m", ROWS)
def test_hard_vote_is_the_restatement_bit_for_bit(dev, m, M, weighted):
    rs = np.random.RandomState(1000 * m + M)
    preds = rs.randint(0, 2, size=(M, m)).astype(np.uint8)
    if m > 2 and M % 2 == 0:
        preds[0::2, 0], preds[1::2, 0] = 0, 1                                     # an exact tie without weights
    w = _weights(M) if weighted else None
    want, want_label = R.hard_vote(preds, w)
    placed = [_placed(preds[j][:, None], j % 3, dev, 1) for j in range(M)]
    before = ensemble._LAUNCHES["hard_vote"]
    counts, label = ensemble._hard_vote([t for t, _ in placed], w, [c for _, c in placed])
    assert ensemble._LAUNCHES["hard_vote"] - before == (1 if m else 0)
    assert _same(counts, want.reshape(m, 2)) and _same(label, want_label.reshape(m))
    if m > 2 and M % 2 == 0 and not weighted:
        assert want[0, 0] == want[0, 1] == M / 2 and want_label[0] == 0, "ties go to the first class"
    for i in range(min(m, 5)):
        assert _same(want[i], np.bincount(preds[:, i], weights=w, minlength=2).astype(np.float64))


# ---- the whole stack ------------------------------------------------------------------------------------------------------------------------
N, D, CV = 120, 10, 5


def _learners():
    """This package's eight learners at their smallest."""
    return [("knn", neighbors.KNeighborsClassifier(3)), ("lr", linear_model.LogisticRegression()), ("svc", svm.PlattSVC()),
            ("bnb", naive_bayes.BernoulliNB()), ("tree", random_forest.DecisionTreeClassifier()), ("rf", random_forest.RandomForestClassifier(5)),
            ("gbc", gradient_boosting.GradientBoostingClassifier(5)), ("mlp", mlp.MLPClassifier(max_iter=5))]


def _final():
    return gradient_boosting.GradientBoostingClassifier(5, 0.1, 3)


@functools.lru_cache(maxsize=None)
def _data():
    rs = np.random.RandomState(5)
    X = rs.normal(size=(N, D))
    y = np.where(X[:, 0] + 0.8 * X[:, 1] * X[:, 2] + 0.7 * rs.normal(size=N) > 0.2, "pos", "neg")
    return X, y, rs.normal(size=(37, D))


@functools.lru_cache(maxsize=None)
def _fitted(kind):
    """The fits every test below shares, each computed once: "stack" = fit_classifier_stack on numpy, "tensor" = on a CUDA tensor, "alone" =
    the two classes' own fit, "single" = fresh clones fitted one at a time per fold and on all rows."""
    X, y, _ = _data()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # five epochs and 96 rows: the learners' convergence warnings are not the subject
        if kind == "stack":
            return ensemble.fit_classifier_stack(_learners(), X, y, _final(), cv=CV, weights=_weights(8).tolist())
        if kind == "tensor":
            return ensemble.fit_classifier_stack(_learners(), torch.from_numpy(X).to("cuda:0"), y, _final(), cv=CV, weights=_weights(8).tolist())
        if kind == "alone":
            return (ensemble.StackingClassifier(_learners(), _final(), cv=CV).fit(X, y),
                    ensemble.VotingClassifier(_learners(), voting="soft", weights=_weights(8).tolist()).fit(X, y))
        classes, t = R.encode(y)
        ests = [est for _, est in _learners()]
        methods = [R.resolve_stack_method(est) for est in ests]
        meta = R.oof(ests, X, t, R.folds(t, CV), methods, ensemble._clone)
        return meta, [ensemble._clone(est).fit(X, t) for est in ests], methods


def test_the_stack_reports_which_learners_looped(dev):
    stacking, vote = _fitted("stack")
    assert stacking.fit_paths_ == vote.fit_paths_ == {"knn": "looped", "lr": "linear_model._solve", "svc": "looped", "bnb": "naive_bayes.fit_masks",
                                                      "tree": "random_forest._grow", "rf": "random_forest._grow",
                                                      "gbc": "gradient_boosting._fit_chains", "mlp": "GridMLPTrainer.fit"}
    assert stacking.stack_method_ == ["predict_proba"] * 8 and list(stacking.classes_) == ["neg", "pos"]
    assert all(a is b for a, b in zip(stacking.estimators_, vote.estimators_)), "one set of full-data fits serves both models"


def test_batched_fold_fits_equal_the_one_at_a_time_fits_bit_for_bit(dev):
    stacking, _ = _fitted("stack")
    meta, _, _ = _fitted("single")
    assert isinstance(stacking.oof_, np.ndarray) and stacking.oof_.shape == (N, 8) and stacking.oof_.dtype == np.float64
    for j, (name, _) in enumerate(_learners()):
        assert _same(stacking.oof_[:, j], meta[:, j]), f"{name}: the batched fold fits differ from fresh clones fitted one at a time"


def test_transform_is_the_full_data_learners_own_columns(dev):
    stacking, _ = _fitted("stack")
    _, singles, methods = _fitted("single")
    X, _, Xq = _data()
    for Z in (X, Xq):
        got = stacking.transform(Z)
        for j, est in enumerate(stacking.estimators_):
            assert _same(got[:, j], est.predict_proba(Z)[:, 1])
        assert _same(got, R.transform(singles, methods, Z)), "a full-data fit inside the batch differs from the fit alone"


def test_voting_probabilities_are_the_restatement_on_the_learners_columns(dev):
    _, vote = _fitted("stack")
    _, _, Xq = _data()
    probas = [est.predict_proba(Xq) for est in vote.estimators_]
    want, label = R.soft_vote(probas, vote.weights)
    assert _same(vote.predict_proba(Xq), want)
    assert np.array_equal(vote.predict(Xq), vote.classes_[label])
    assert _same(vote.transform(Xq), np.hstack(probas))
    vote.weights = None
    try:
        assert _same(vote.predict_proba(Xq), R.soft_vote(probas)[0])
    finally:
        vote.weights = _weights(8).tolist()


def test_the_shared_fits_give_the_models_of_the_two_classes_own_fit(dev):
    stacking, vote = _fitted("stack")
    alone_s, alone_v = _fitted("alone")
    _, _, Xq = _data()
    assert _same(stacking.oof_, alone_s.oof_)
    for name in ("predict_proba", "decision_function", "transform"):
        assert _same(getattr(stacking, name)(Xq), getattr(alone_s, name)(Xq)), name
    assert np.array_equal(stacking.predict(Xq), alone_s.predict(Xq)) and stacking.predict(Xq).dtype == stacking.classes_.dtype
    assert _same(vote.predict_proba(Xq), alone_v.predict_proba(Xq)) and np.array_equal(vote.predict(Xq), alone_v.predict(Xq))
    # the final estimator was fitted on the out-of-fold matrix and the encoded labels
    t = R.encode(_data()[1])[1]
    again = _final().fit(stacking.oof_, t)
    assert _same(again.decision_function(stacking.transform(Xq)), stacking.decision_function(Xq))
    assert np.array_equal(stacking.predict(Xq), stacking.classes_[(stacking.decision_function(Xq) >= 0).astype(np.intp)])


def test_numpy_input_and_cuda_tensor_input_give_the_same_bits(dev):
    stacking, vote = _fitted("stack")
    t_stacking, t_vote = _fitted("tensor")
    _, _, Xq = _data()
    Xq_d = torch.from_numpy(Xq).to(dev)
    assert isinstance(t_stacking.oof_, torch.Tensor) and t_stacking.oof_.is_cuda and _same(t_stacking.oof_, stacking.oof_)
    for model, other in ((t_stacking, stacking), (t_vote, vote)):
        got = model.predict_proba(Xq_d)
        assert isinstance(got, torch.Tensor) and got.is_cuda and _same(got, other.predict_proba(Xq))
        assert isinstance(model.predict_proba(Xq), np.ndarray) and _same(model.predict_proba(Xq), other.predict_proba(Xq))
        labels = model.predict(Xq_d)
        assert isinstance(labels, np.ndarray) and labels.dtype == other.classes_.dtype and np.array_equal(labels, other.predict(Xq))
    assert _same(t_stacking.transform(Xq_d), stacking.transform(Xq)) and _same(t_stacking.decision_function(Xq_d), stacking.decision_function(Xq))


def test_hard_voting_passthrough_and_other_stack_methods(dev):
    """The remaining routes on four cheap learners: hard voting with ties, ``passthrough``, a ``decision_function`` and a ``predict``
    column, an explicit list of folds, {-1, 1} labels, the default final estimator."""
    X, y, Xq = _data()
    y = np.where(y == "pos", 1, -1)
    classes, t = R.encode(y)
    ests = [("lr", linear_model.LogisticRegression()), ("bnb", naive_bayes.BernoulliNB()), ("svc", svm.SVC()), ("tree", random_forest.DecisionTreeClassifier(max_depth=2))]
    hard = ensemble.VotingClassifier(ests, voting="hard").fit(X, y)
    preds = np.stack([est.predict(Xq) for est in hard.estimators_])
    counts, label = R.hard_vote(preds)
    assert np.array_equal(hard.predict(Xq), classes[label]) and set(hard.predict(Xq)) <= {-1, 1}
    assert np.array_equal(hard.transform(Xq), preds.T) and hard.transform(Xq).dtype == np.int64
    with pytest.raises(AttributeError, match="voting='hard'"):
        hard.predict_proba(Xq)
    w = _weights(4).tolist()
    assert np.array_equal(ensemble.VotingClassifier(ests, voting="hard", weights=w).fit(X, y).predict(Xq), classes[R.hard_vote(preds, w)[1]])
    pairs = [(tr[::-1].copy(), te) for tr, te in R.folds(t, 3)][::-1]
    for stack_method, want in (("auto", ["predict_proba", "predict_proba", "decision_function", "predict_proba"]), ("predict", ["predict"] * 4)):
        s = ensemble.StackingClassifier(ests, cv=pairs, stack_method=stack_method, passthrough=True).fit(X, y)
        assert s.stack_method_ == want and isinstance(s.final_estimator_, linear_model.LogisticRegression)
        meta = R.oof([est for _, est in ests], X, t, pairs, want, ensemble._clone)
        assert _same(s.oof_, np.hstack([meta, X]))
        assert _same(s.transform(Xq), R.transform(s.estimators_, want, Xq, passthrough=True))
        assert np.array_equal(s.predict(Xq), classes[(s.decision_function(Xq) > 0).astype(np.intp)])
    with pytest.raises(ValueError, match="does not implement"):
        ensemble.StackingClassifier(ests, stack_method="predict_proba").fit(X, y)
