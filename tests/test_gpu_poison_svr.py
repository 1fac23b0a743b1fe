"""GPU: svm.SVR with every ``torch.empty`` served from poisoned, guarded pools (tests/poison.py).

The solver's state (alpha, G), its diagonal scratch and rho are ``torch.empty``: the contract of bbbp_svr_smo has the host initialise the
two flags only, and the first launch of a problem sets alpha = 0 and G = the linear term itself.  So under the fills 0xFF (NaN as float64,
-1 as a counter) and 0x7B a fit and a predict must give the bits of an unpoisoned run -- a difference is a read of memory the kernel does
not own -- and no guard band may be touched.  The sizes take the register forms with one and with two rows per thread and the
global-state form; the launches of 7 iterations make the state cross the launch boundary through the poisoned arrays."""
import numpy as np
import pytest
import torch

from bbbp_amd import svm
from bbbp_amd.svm import SVR
from poison import poisoned_allocations
import svr_oracle as O

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x7B)


def _bits(model, Q):
    return (model.alpha_, model.intercept_, model.support_, model.dual_coef_, model.support_vectors_, np.array([model.n_iter_, model.fit_status_]),
            model.predict(Q), model.predict_device(torch.from_numpy(Q).cuda()).cpu().numpy())


@pytest.mark.parametrize("n,d,kind,C,epsilon", [(130, 7, "rbf", 0.1, 0.5), (333, 100, "rbf", 1.0, 0.1), (200, 10, "linear", 0.1, 0.2), (1100, 20, "rbf", 1.0, 0.3)])
def test_fit_and_predict_do_not_depend_on_the_fill(dev, monkeypatch, n, d, kind, C, epsilon):
    X, t = O.make_data(n, d, 0.3, 1)
    Q, _ = O.make_data(65, d, 0.3, 2)
    want = _bits(SVR(kind, C, epsilon).fit(X, t), Q)
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _bits(SVR(kind, C, epsilon).fit(X, t), Q)
        assert pa.check() > 0, "no allocation went through the pools"
        pa.release()
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"fill {fill:#04x}: result {i} differs from the unpoisoned run"


@pytest.mark.parametrize("n", [130, 4100])
def test_state_crosses_the_launch_boundary_through_poisoned_arrays(dev, monkeypatch, n):
    """Launches of 7 iterations, 20 of them: the register form writes its state back and reads it again, the global-state form (4100
    rows) keeps it there; alpha, G and rho equal those of one launch of 140 iterations under no poison."""
    X, t = O.make_data(n, 20, 0.3, 1)
    K = svm.kernel_matrix(torch.from_numpy(X).cuda(), "rbf", O.gamma_scale(X))[0]
    td = torch.from_numpy(t).cuda()
    ref = svm._SvrProblem(K, td, 1.0, 0.1, 1e-3)
    want = svm._solve_svr([ref], max_iter=140, iters_per_launch=140)
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            pr = svm._SvrProblem(K, td, 1.0, 0.1, 1e-3)
            got = svm._solve_svr([pr], max_iter=140, iters_per_launch=7)
            torch.cuda.synchronize()
        assert pa.check() >= 4                                   # alpha, G, the diagonal scratch and rho
        pa.release()
        assert got == want == [(140, False)]
        assert torch.equal(pr.alpha, ref.alpha) and torch.equal(pr.grad, ref.grad) and torch.equal(pr.rho, ref.rho)
