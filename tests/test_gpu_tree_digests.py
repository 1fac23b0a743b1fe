"""GPU: the tree learners fit and predict bit for bit what they did before csrc/rf.hip and csrc/gbt.hip shared csrc/tree_fit.h and
random_forest.py and gradient_boosting.py shared _tree_host.py.

tests/golden/tree_digests.json holds, group by group and for every case below, the SHA-256 of the raw bytes of the public results: every
array of ``trees_``, ``train_score_`` (boosted trees), ``weighted_n_node_samples_`` (regression forests) and ``decision_function`` /
``predict_proba`` / ``predict`` on the first 33 training rows.  It was recorded with tools/record_tree_digests.py from a checkout and build of
the commit BEFORE that refactor (`python tools/record_tree_digests.py --package-root <that checkout>`), never from the code under test.
The forests are also reproduced bit for bit by tests/rf_numpy.py and tests/rfr_numpy.py; the boosted trees are otherwise certified within
rounding allowances only (tests/gbt_replay.py, tests/gbr_replay.py), which a reordered sum could pass: equal digests close that gap.

Shapes are the smallest that reach each shared piece.  Boosted trees: 4 stages of depth 3 at learning rate 0.1 over d = 3 features, one
column rounded to one decimal so that real ties reach the lowest-feature and lowest-position rule; n = 256, 257 and 600 rows: one pass of
the 256-position scan, a second pass of a single position (the carry alone), three passes with segments that straddle passes;
``min_samples_leaf`` 1 and 3; one case of depth 1.  Forests: n = 257, d = 5, 3 trees, ``max_features=2``, with the bootstrap (the
compaction uses the shared rank) and without, and the one-tree ``DecisionTree*`` forms.  Inputs come from ``numpy.random.default_rng`` with
a fixed seed, rounded to float32 first."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from bbbp_amd import gradient_boosting as G
from bbbp_amd import random_forest as F

pytestmark = pytest.mark.gpu

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_digests.json")
HEAD = 33                          # training rows that are predicted
# (n, min_samples_leaf, max_depth)
BOOSTED = tuple((n, msl, 3) for n in (256, 257, 600) for msl in (1, 3)) + ((257, 1, 1),)
FOREST_N, FOREST_D = 257, 5
GROUPS = ("gbt", "gbr", "rf", "rfr")


@functools.lru_cache(maxsize=None)
def _problem(n, d):
    """(X float32 [n, d] with column 1 rounded to one decimal, two-class labels, float64 targets), unchanged between the cases."""
    rng = np.random.default_rng(20261020)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[:, 1] = np.round(X[:, 1], 1)
    noise = rng.standard_normal(n)
    signal = X[:, 0].astype(np.float64) + 0.5 * X[:, 1] - 0.25 * X[:, 2] * X[:, 0]
    labels = (signal + 0.5 * noise > 0.0).astype(np.int64)
    return X, labels, signal + 0.1 * noise


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _trees(cid, model, out):
    for key in sorted(model.trees_):
        out[f"{cid}-trees-{key}"] = _sha(model.trees_[key])


def _boosted(regression):
    out = {}
    for n, msl, depth in BOOSTED:
        X, labels, targets = _problem(n, 3)
        cid = f"{'gbr' if regression else 'gbt'}-n{n}-msl{msl}-depth{depth}"
        if regression:
            model = G.GradientBoostingRegressor(4, learning_rate=0.1, max_depth=depth, min_samples_leaf=msl).fit(X, targets)
            out[f"{cid}-predict"] = _sha(model.predict(X[:HEAD]))
        else:
            model = G.GradientBoostingClassifier(4, 0.1, depth, min_samples_leaf=msl).fit(X, labels)
            out[f"{cid}-decision"] = _sha(model.decision_function(X[:HEAD]))
        _trees(cid, model, out)
        out[f"{cid}-train_score"] = _sha(model.train_score_)
    return out


def _forests(regression):
    out = {}
    X, labels, targets = _problem(FOREST_N, FOREST_D)
    forest, tree = (F.RandomForestRegressor, F.DecisionTreeRegressor) if regression else (F.RandomForestClassifier, F.DecisionTreeClassifier)
    models = {f"boot{int(b)}": forest(3, max_features=2, bootstrap=b, random_state=7) for b in (True, False)}
    models["tree"] = tree(random_state=7)
    for name, model in models.items():
        cid = f"{'rfr' if regression else 'rf'}-n{FOREST_N}-{name}"
        model.fit(X, targets if regression else labels)
        _trees(cid, model, out)
        if regression:
            out[f"{cid}-weighted_n_node_samples"] = _sha(model.weighted_n_node_samples_)
            out[f"{cid}-predict"] = _sha(model.predict(X[:HEAD]))
        else:
            out[f"{cid}-predict_proba"] = _sha(model.predict_proba(X[:HEAD]))
    return out


def compute_digests(group):
    """{case id: SHA-256 of the result's bytes} of one group, with whatever package ``bbbp_amd`` resolves to."""
    return {"gbt": lambda: _boosted(False), "gbr": lambda: _boosted(True), "rf": lambda: _forests(False), "rfr": lambda: _forests(True)}[group]()


@pytest.mark.parametrize("group", GROUPS)
def test_results_are_bit_identical_to_the_recorded_commit(dev, group):
    got = compute_digests(group)
    with open(DIGESTS) as f:
        want = json.load(f)[group]
    assert sorted(got) == sorted(want), f"{group}: the case list differs from the recorded one"
    differ = [k for k in got if got[k] != want[k]]
    assert not differ, f"{group}: {len(differ)} of {len(got)} results differ from the recorded commit, first: {differ[:5]}"
