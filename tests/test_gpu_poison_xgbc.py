"""``bbbp_amd.xgb.XGBClassifier`` from poisoned allocations: the 65 x 7 and 257 x 9 fits of ``tests/test_gpu_xgbc.py``, with and without the
row and column draws, and a ``predict_proba``, with every output, work area, byte matrix and column mask out of pools filled with 0x00, 0xFF
and 0x7B (``tests/poison.py``), equal the clean ones bit for bit.  No kernel may depend on bytes it does not own (the ``r`` of rows, the slots
of leaves in the second row list, unused table slots, candidates and mask words among them), no output may need zero-filling, and no guard
band may be written."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from poison import FILLS, poisoned_allocations  # noqa: E402
from test_gpu_xgbc import KEYS, as_ref, assert_same_model, bits, case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["n65", "n257_bin16"])
@pytest.mark.parametrize("draws", [dict(), dict(subsample=0.8, colsample_bytree=0.8, random_state=3)], ids=["all", "sampled"])
def test_fit_and_predict_proba_under_poison(dev, monkeypatch, name, draws):
    from bbbp_amd import xgb
    X, y, params, ref = case(name)
    params = {**params, **draws}
    clean = xgb.XGBClassifier(device=dev, **params).fit(X, y)
    if not draws:
        assert_same_model(clean, ref)
    want = clean.predict_proba(X[:50])
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            clf = xgb.XGBClassifier(device=dev, **params).fit(X, y)
            proba = clf.predict_proba(X[:50])
            torch.cuda.synchronize()
        assert pa.check() >= 11 + bool(draws), "the problem's allocations did not go through the pools"
        pa.release()
        assert_same_model(clf, as_ref(clean), what=f"fill {fill:#04x}: ")
        assert all(clf.trees_[k].dtype == clean.trees_[k].dtype for k in KEYS) and np.array_equal(bits(proba), bits(want)), hex(fill)
