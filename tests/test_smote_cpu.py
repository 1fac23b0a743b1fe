"""CPU: the numpy restatement of SMOTE, TomekLinks and SMOTETomek (tests/smote_numpy.py) -- its neighbour lists against scikit-learn, its
structure, Tomek links on hand-made sets, imbalanced-learn where that package is installed -- and the argument checks of
bbbp_amd.imbalance that need no GPU.  tests/test_gpu_smote.py holds the device to the restatement bit for bit."""
import numpy as np
import pytest

import smote_numpy as S
from bbbp_amd import imbalance as I

K, SEED = 5, 42


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("p", S.PROBLEMS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_class_neighbour_lists_equal_sklearn(p, dtype):
    from sklearn.neighbors import NearestNeighbors
    X, y = S.problem(*p, dtype=dtype)
    Xc = X[y == 1]
    assert S.gap(Xc, K) > 1
    sk = NearestNeighbors(n_neighbors=K + 1, algorithm="brute").fit(Xc).kneighbors(Xc, return_distance=False)
    assert np.array_equal(sk[:, 0], np.arange(len(Xc)))                  # no duplicate rows: column 0 is the row itself
    assert np.array_equal(sk[:, 1:], S.class_neighbours(Xc, K))


@pytest.mark.parametrize("p", S.PROBLEMS[:4])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_structure_of_the_restatement(p, dtype):
    X, y = S.problem(*p, dtype=dtype)
    n = len(y)
    record = []
    X_res, y_res = S.smote(X, y, K, SEED, record=record)
    assert X_res.dtype == X.dtype and y_res.dtype == y.dtype
    counts = np.bincount(y_res)
    assert counts[0] == counts[1] == n - p[2]
    assert np.array_equal(_bits(X_res[:n]), _bits(X)) and np.array_equal(y_res[:n], y)
    (c, rows, nbrs, steps), = record
    assert c == 1 and len(rows) == len(X_res) - n and np.all(y_res[n:] == 1)
    Xc = X[y == 1].astype(np.float64)
    nn = S.class_neighbours(X[y == 1], K)
    assert np.all((0 <= steps) & (steps < 1))
    assert all(nbrs[j] in nn[rows[j]] for j in range(len(rows)))
    a, b = Xc[rows], Xc[nbrs]
    want = (a + steps[:, None] * (b - a)).astype(X.dtype)                # recomputed in float64
    if dtype == "float64":
        assert np.array_equal(_bits(X_res[n:]), _bits(want))
    else:
        # float32 input: b - a is rounded to float32 first (at most 2^-24 |b - a| <= 2^-23 max|X| off, times s < 1), and both sides round
        # the sum to float32 (2^-24 max|X| each at most): within 2^-22 max|X| of the float64 expression, and bit-equal to the expression
        # with the float32 difference
        assert np.allclose(X_res[n:], want, rtol=0, atol=2.0 ** -22 * np.abs(Xc).max())
        d32 = (X[y == 1][nbrs] - X[y == 1][rows]).astype(np.float64)
        assert np.array_equal(_bits(X_res[n:]), _bits((a + steps[:, None] * d32).astype(np.float32)))


def test_strategies_give_the_stated_counts():
    X, y = S.problem(130, 5, 40, 2)
    assert np.bincount(S.smote(X, y, K, SEED, strategy={1: 70})[1]).tolist() == [90, 70]
    assert np.bincount(S.smote(X, y, K, SEED, strategy={0: 95, 1: 41})[1]).tolist() == [95, 41]
    assert np.bincount(S.smote(X, y, K, SEED, strategy=0.7)[1]).tolist() == [90, int(0.7 * 90 - 40) + 40]
    assert np.bincount(S.smote(X, y, K, SEED, strategy="minority")[1]).tolist() == [90, 90]
    X3, y3 = S.problem3(130, 5, 40, 2)
    assert np.bincount(y3).tolist() == [70, 40, 20]
    assert np.bincount(S.smote(X3, y3, K, SEED, strategy="minority")[1]).tolist() == [70, 40, 70]
    assert np.bincount(S.smote(X3, y3, K, SEED, strategy="not minority")[1]).tolist() == [70, 70, 20]
    assert np.bincount(S.smote(X3, y3, K, SEED, strategy="all")[1]).tolist() == [70, 70, 70]
    assert np.bincount(S.smote(X3, y3, K, SEED)[1]).tolist() == [70, 70, 70]


def test_an_int_seed_restarts_the_stream_per_class_and_an_instance_continues():
    X, y = S.problem3(130, 5, 40, 2)
    by_int, by_instance = [], []
    S.smote(X, y, K, SEED, record=by_int)
    S.smote(X, y, K, np.random.RandomState(SEED), record=by_instance)
    assert [r[0] for r in by_int] == [r[0] for r in by_instance] == [1, 2]
    fresh = np.random.RandomState(SEED)
    for c, rows, _, steps in by_int:                                     # each class starts at the head of the seed's stream
        rs = np.random.RandomState(SEED)
        n_c = int((y == c).sum())
        assert np.array_equal(rows, rs.randint(0, n_c * K, size=len(rows)) // K) and np.array_equal(steps, rs.uniform(size=len(rows)))
    for c, rows, _, steps in by_instance:                                # one stream runs through the classes
        n_c = int((y == c).sum())
        assert np.array_equal(rows, fresh.randint(0, n_c * K, size=len(rows)) // K) and np.array_equal(steps, fresh.uniform(size=len(rows)))
    assert np.array_equal(by_int[0][3], by_instance[0][3]) and not np.array_equal(by_int[1][3][:30], by_instance[1][3][:30])


def test_tomek_links_on_hand_made_sets():
    col = lambda *v: np.array(v, dtype=np.float64)[:, None]  # noqa: E731
    # a mutual pair of one class is not a link
    X, y = col(0.0, 0.1, 5.0, 9.0), np.array([0, 0, 1, 1])
    assert not S.tomek_members(X, y).any()
    # a chain a -> b <-> c: a's nearest is b, b and c are mutual and of different classes; only b and c are flagged
    X, y = col(0.0, 1.0, 1.5, 10.0, 10.2, 10.9), np.array([1, 0, 1, 0, 0, 0])
    assert S.tomek_members(X, y).tolist() == [False, True, True, False, False, False]
    # a cross-class pair: "all" loses both rows, "auto" only the majority's
    X, y = col(0.0, 0.1, 5.0, 5.3, 9.0, 9.4), np.array([0, 1, 0, 0, 0, 0])
    assert S.tomek_members(X, y).tolist() == [True, True, False, False, False, False]
    assert S.tomek(X, y, "all")[2].tolist() == [2, 3, 4, 5]
    assert S.tomek(X, y, "auto")[2].tolist() == [1, 2, 3, 4, 5]
    assert S.tomek(X, y, "majority")[2].tolist() == [1, 2, 3, 4, 5]
    assert S.tomek(X, y, "not majority")[2].tolist() == [0, 2, 3, 4, 5]
    assert S.tomek(X, y, [1])[2].tolist() == [0, 2, 3, 4, 5]


@pytest.mark.parametrize("p", S.PROBLEMS[:4])
def test_tomek_counts_of_the_problems(p):
    """The sets the GPU tests run Tomek on hold links: a comparison there cannot pass vacuously."""
    X, y = S.problem(*p)
    on_original, on_resampled = {65: (8, 14), 130: (20, 10), 257: (38, 40), 300: (42, 8)}[p[0]]
    assert int(S.tomek_members(X, y).sum()) == on_original
    assert int(S.tomek_members(*S.smote(X, y, K, SEED)).sum()) == on_resampled


@pytest.mark.parametrize("p", S.PROBLEMS[:4])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_restatement_equals_imbalanced_learn(p, dtype):
    """Skipped without the package.  Tie-free problems: dropping column 0 and leaving the row out by index select the same neighbours."""
    pytest.importorskip("imblearn")
    from imblearn.combine import SMOTETomek
    from imblearn.over_sampling import SMOTE
    from imblearn.under_sampling import TomekLinks
    X, y = S.problem(*p, dtype=dtype)
    X_res, y_res = SMOTE(random_state=SEED).fit_resample(X, y)
    want = S.smote(X, y, K, SEED)
    assert X_res.dtype == want[0].dtype and np.array_equal(_bits(X_res), _bits(want[0])) and np.array_equal(y_res, want[1])
    tl = TomekLinks()
    X_res, y_res = tl.fit_resample(X, y)
    want = S.tomek(X, y, "auto")
    assert np.array_equal(_bits(X_res), _bits(want[0])) and np.array_equal(y_res, want[1]) and np.array_equal(tl.sample_indices_, want[2])
    X_res, y_res = SMOTETomek(random_state=SEED).fit_resample(X, y)
    want = S.smote_tomek(X, y, K, SEED)
    assert np.array_equal(_bits(X_res), _bits(want[0])) and np.array_equal(y_res, want[1])


# ---- bbbp_amd.imbalance: the checks that run before anything touches a device --------------------------------------------------------
def test_argument_validation_without_a_gpu():
    X, y = S.problem(65, 3, 7, 1)
    for k in (0, 33, True, 2.0):
        with pytest.raises(ValueError, match="k_neighbors"):
            I.SMOTE(k_neighbors=k)
    for cls in (I.SMOTE, I.TomekLinks, I.SMOTETomek):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(device="cpu")
    with pytest.raises(ValueError, match="sampling_strategy"):
        I.SMOTE(sampling_strategy="majority")
    with pytest.raises(ValueError, match="sampling_strategy"):
        I.SMOTETomek(sampling_strategy="bogus")
    with pytest.raises(ValueError, match="sampling_strategy"):
        I.TomekLinks(sampling_strategy="minority")
    with pytest.raises(ValueError, match="sampling_strategy"):
        I.TomekLinks(sampling_strategy=0.5)
    with pytest.raises(ValueError, match="random_state"):
        I.SMOTE(random_state="42")
    X3, y3 = S.problem3(130, 5, 40, 2)
    with pytest.raises(ValueError, match="two classes"):
        I.SMOTE(sampling_strategy=0.8).fit_resample(X3, y3)
    with pytest.raises(ValueError, match="remove rows"):
        I.SMOTE(sampling_strategy=0.1).fit_resample(X, y)                # int(0.1 * 58 - 7) < 0
    with pytest.raises(ValueError, match="target count"):
        I.SMOTE(sampling_strategy={1: -3}).fit_resample(X, y)
    with pytest.raises(ValueError, match="would remove"):
        I.SMOTE(sampling_strategy={1: 3}).fit_resample(X, y)
    with pytest.raises(ValueError, match="does not hold"):
        I.SMOTE(sampling_strategy={7: 30}).fit_resample(X, y)
    with pytest.raises(ValueError, match="does not hold"):
        I.TomekLinks(sampling_strategy=[7]).fit_resample(X, y)
    with pytest.raises(ValueError, match="has 7 rows"):                  # n_c <= k, found before any launch
        I.SMOTE(k_neighbors=7).fit_resample(X, y)
    with pytest.raises(ValueError, match="has 7 rows"):
        I.SMOTETomek(smote=I.SMOTE(k_neighbors=8)).fit_resample(X, y)
    with pytest.raises(ValueError, match="one label per row"):
        I.SMOTE().fit_resample(X, y[:-1])
    with pytest.raises(ValueError, match="2-D"):
        I.SMOTE().fit_resample(X[:, 0], y)
    with pytest.raises(ValueError, match="smote must be"):
        I.SMOTETomek(smote=I.TomekLinks())
    with pytest.raises(ValueError, match="tomek must be"):
        I.SMOTETomek(tomek=I.SMOTE())


def test_strategy_resolution_equals_the_restatement():
    """The host bookkeeping of the module against the restatement's, on two and three classes and on string labels."""
    for X, y in (S.problem(130, 5, 40, 2), S.problem3(130, 5, 40, 2)):
        for labels in (y, np.array(["BBB+", "BBB-", "mid"])[y]):
            classes, ids = np.unique(labels, return_inverse=True)
            counts = np.bincount(ids)
            strategies = ["auto", "not majority", "minority", "not minority", "all", {classes[1]: 75}]
            if len(classes) == 2:
                strategies.append(0.9)
            for s in strategies:
                got = {classes[c]: m for c, m in I._smote_targets(s, classes, counts).items()}
                assert got == S.targets(labels, s) and list(got) == sorted(got), s
            for s in ("auto", "not minority", "not majority", "majority", "all", [classes[0]]):
                remove = I._tomek_remove(s, classes, counts)
                assert remove.dtype == np.uint8 and sorted(classes[remove.astype(bool)].tolist()) == sorted(S.remove_set(labels, s)), s


def test_the_two_entry_points_validate_their_arguments_before_touching_the_gpu():
    import ctypes
    from bbbp_amd import _lib
    L = _lib.lib()
    ERR_ARG = 1
    fake = ctypes.c_void_p(4096)                                         # never dereferenced: validation comes first
    ok = dict(Xc=fake, dt=1, ldx=8, n_c=10, nn=fake, idx=fake, steps=fake, k=5, n_new=4, d=8, out=fake, ldo=8)

    def synth(**kw):
        a = {**ok, **kw}
        return L.bbbp_smote_synth(None, a["Xc"], a["dt"], a["ldx"], a["n_c"], a["nn"], a["idx"], a["steps"], a["k"], a["n_new"], a["d"], a["out"], a["ldo"])

    for bad in (dict(Xc=None), dict(nn=None), dict(idx=None), dict(steps=None), dict(out=None), dict(k=0), dict(k=-1), dict(n_new=-1), dict(d=-1),
                dict(n_c=-1), dict(dt=2), dict(ldx=7), dict(ldo=7), dict(n_c=5)):
        assert synth(**bad) == ERR_ARG, bad
        assert b"smote_synth" in L.bbbp_last_error()
    assert synth(n_new=0) == 0                                           # nothing to do: no launch
    assert L.bbbp_tomek_links(None, None, fake, fake, 2, 10, fake) == ERR_ARG
    assert L.bbbp_tomek_links(None, fake, None, fake, 2, 10, fake) == ERR_ARG
    assert L.bbbp_tomek_links(None, fake, fake, None, 2, 10, fake) == ERR_ARG
    assert L.bbbp_tomek_links(None, fake, fake, fake, 2, 10, None) == ERR_ARG
    assert L.bbbp_tomek_links(None, fake, fake, fake, 2, -1, fake) == ERR_ARG
    assert L.bbbp_tomek_links(None, fake, fake, fake, 0, 10, fake) == ERR_ARG
    assert b"tomek_links" in L.bbbp_last_error()
    assert L.bbbp_tomek_links(None, fake, fake, fake, 2, 0, fake) == 0
