"""GPU: svm.PlattSVC with every ``torch.empty`` served from poisoned, guarded pools (tests/poison.py).

The out-of-fold vector, the sigmoid's (A, B) and its two counters, the probabilities and the solver's diagonal scratch are ``torch.empty``:
bbbp_svm_oof_decision writes every held-out row (the one-class rule fills the rest), bbbp_svm_platt_fit writes its four outputs whatever
they held, bbbp_svm_platt_proba writes both columns.  So under each fill a fit and a predict_proba must give the bits of an unpoisoned run --
a difference is a read of memory the kernels do not own -- and no guard band may be touched.  n = 65: one row past a wavefront."""
import numpy as np
import pytest
import torch

from bbbp_amd.svm import PlattSVC
from poison import FILLS, poisoned_allocations
import svc_oracle as O

pytestmark = pytest.mark.gpu


def _bits(model, Q):
    return (model.oof_decision_, model.probA_, model.probB_, np.array([model.platt_n_iter_, model.platt_status_, model.n_iter_, model.fit_status_]),
            model.alpha_, model.intercept_, model.support_, model.predict_proba(Q), model.predict_proba(torch.from_numpy(Q).cuda()).cpu().numpy(),
            model.predict_log_proba(Q))


@pytest.mark.parametrize("kind,folds", [("rbf", None), ("linear", None), ("rbf", "one-class")])
def test_fit_and_predict_proba_do_not_depend_on_the_fill(dev, monkeypatch, kind, folds):
    X, y = O.make_data(65, 7, 0.7, 1)
    Q, _ = O.make_data(65, 7, 0.7, 2)
    if folds == "one-class":                 # the first fold holds out every row of one class: libsvm's constant, written by index_fill
        pos = np.flatnonzero(y > 0)
        rest = np.flatnonzero(y <= 0)
        folds = [pos, rest[::2], rest[1::2]]
    want = _bits(PlattSVC(kernel=kind).fit(X, y, folds=folds), Q)
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _bits(PlattSVC(kernel=kind).fit(X, y, folds=folds), Q)
            torch.cuda.synchronize()
        assert pa.check() > 0, "no allocation went through the pools"
        pa.release()
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"fill {fill:#04x}: result {i} differs from the unpoisoned run"
