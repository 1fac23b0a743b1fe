"""``bbbp_amd.cat`` from poisoned allocations: the 65 x 7 and 300 x 20 fits of ``tests/test_gpu_cat.py`` with every output, work area and
byte matrix out of pools filled with 0x00, 0xFF and 0x7B (``tests/poison.py``) equal the clean fits bit for bit.  No kernel may depend on
bytes it does not own (the second row list and part table, the children's table, candidates of feature blocks and leaves beyond a tree's
own among them), no output may need zero-filling, and no guard band may be written."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from poison import FILLS, poisoned_allocations  # noqa: E402
from test_gpu_cat import KEYS, assert_same_model, bits, case, reference_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["n65", "n300"])
def test_fit_and_predict_under_poison(dev, monkeypatch, name):
    from bbbp_amd import cat
    X, y, params, ref = case(name)
    clean = cat.CatBoostRegressor(device=dev, **params).fit(X, y)
    assert_same_model(clean, ref)
    want = clean.predict(X[:50])
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            reg = cat.CatBoostRegressor(device=dev, **params).fit(X, y)
            pred = reg.predict(X[:50])
            torch.cuda.synchronize()
        assert pa.check() >= 8, "the problem's allocations did not go through the pools"
        pa.release()
        assert_same_model(reg, reference_of(clean), what=f"fill {fill:#04x}: ")
        assert all(reg.trees_[k].dtype == clean.trees_[k].dtype for k in KEYS) and np.array_equal(bits(pred), bits(want)), hex(fill)
