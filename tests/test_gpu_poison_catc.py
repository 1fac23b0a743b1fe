"""``bbbp_amd.cat.CatBoostClassifier`` from poisoned allocations: the 65 x 7 and 300 x 20 fits of ``tests/test_gpu_catc.py``, without and
with bootstrap weights, and a ``predict_proba``, with every output, work area, byte matrix and the weight table out of pools filled with
0x00, 0xFF and 0x7B (``tests/poison.py``), equal the clean fits bit for bit.  No kernel may depend on bytes it does not own (the second
row list and part table, the children's table, candidates of feature blocks, leaves beyond a tree's own and the columns of the weight
table beyond a problem's rows among them), no output may need zero-filling, and no guard band may be written."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from poison import FILLS, poisoned_allocations  # noqa: E402
from test_gpu_cat import KEYS, bits  # noqa: E402
from test_gpu_catc import assert_same_model, case, reference_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("temperature", [None, 0.5])
@pytest.mark.parametrize("name", ["n65", "n300"])
def test_fit_and_predict_under_poison(dev, monkeypatch, name, temperature):
    from bbbp_amd import cat
    X, t, params, ref = case(name, temperature)
    clean = cat.CatBoostClassifier(device=dev, **params).fit(X, t)
    assert_same_model(clean, ref)
    want = clean.predict_proba(X[:50])
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            clf = cat.CatBoostClassifier(device=dev, **params).fit(X, t)
            proba = clf.predict_proba(X[:50])
            torch.cuda.synchronize()
        # seven outputs and the work area of the fit, two of the prediction, the probabilities; the weight table
        assert pa.check() >= 10 + (temperature is not None), "the problem's allocations did not go through the pools"
        if temperature is not None:
            assert any(shape == (params["iterations"], len(X)) and dtype == torch.int32 for _, _, shape, dtype in pa.pools), "the weight table"
        pa.release()
        assert_same_model(clf, reference_of(clean), what=f"fill {fill:#04x}: ")
        assert all(clf.trees_[k].dtype == clean.trees_[k].dtype for k in KEYS) and np.array_equal(bits(proba), bits(want)), hex(fill)
