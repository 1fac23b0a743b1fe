"""``bbbp_amd.xgb`` from poisoned allocations: the 65 x 7 and 257 x 9 fits of ``tests/test_gpu_xgb.py`` with every output, work area and
byte matrix out of pools filled with 0x00, 0xFF and 0x7B (``tests/poison.py``) equal the clean fits bit for bit.  No kernel may depend on
bytes it does not own (the slots of leaves in the second row list, unused table slots and candidates among them), no output may need
zero-filling, and no guard band may be written."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from poison import FILLS, poisoned_allocations  # noqa: E402
from test_gpu_xgb import KEYS, assert_same_model, bits, case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["n65", "n257_bin16"])
def test_fit_and_predict_under_poison(dev, monkeypatch, name):
    from bbbp_amd import xgb
    X, y, params, ref = case(name)
    clean = xgb.XGBRegressor(device=dev, **params).fit(X, y)
    assert_same_model(clean, ref)
    want = clean.predict(X[:50])
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            reg = xgb.XGBRegressor(device=dev, **params).fit(X, y)
            pred = reg.predict(X[:50])
            torch.cuda.synchronize()
        assert pa.check() >= 10, "the problem's allocations did not go through the pools"
        pa.release()
        assert_same_model(reg, {**clean.trees_, "base_score": clean.base_score_, "train_margin": clean.train_margin_}, what=f"fill {fill:#04x}: ")
        assert all(reg.trees_[k].dtype == clean.trees_[k].dtype for k in KEYS) and np.array_equal(bits(pred), bits(want)), hex(fill)
