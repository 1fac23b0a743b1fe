"""GPU batched trainer for the scikit-learn style MLP classifiers of the reference's model-selection stage.

Reference: ``Models/model_opt_maccs.py:133`` (``MLPClassifier(max_iter=2000, learning_rate_init=0.001, batch_size=32)``)
and ``:170-181`` (GridSearchCV over hidden_layer_sizes x activation x learning_rate_init x batch_size, cv=5: 270 fits on
``[n, 100]`` PCA features).  Every fit is tiny, the grid is embarrassingly parallel: one persistent work-group trains
one model (``csrc/mlp.hip``), all fits of a grid run in one launch per chunk of epochs.

The arithmetic is scikit-learn's, in float64; the row visiting order and the initial weights come from the estimator's
own ``RandomState`` stream (``_init_coef`` draws, then one ``sklearn.utils.shuffle`` of the index vector per epoch), so a
fit here follows the scikit-learn fit with the same ``random_state`` step for step (up to summation order inside the
matrix products).  Only the training-loss stopping rule (``early_stopping=False``, the reference's setting) and the
``adam`` solver are implemented -- that is what the reference uses.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _estimator, _lib, ops

_ACT = {"relu": 0, "tanh": 1}


@dataclass
class MLPConfig:
    """One fit: scikit-learn ``MLPClassifier`` hyper-parameters + the training rows (a CV fold) it sees."""
    hidden_layer_sizes: Sequence[int] = (100,)
    activation: str = "relu"
    learning_rate_init: float = 0.001
    batch_size: int = 200
    alpha: float = 1e-4
    max_iter: int = 200
    tol: float = 1e-4
    n_iter_no_change: int = 10
    beta_1: float = 0.9
    beta_2: float = 0.999
    epsilon: float = 1e-8
    random_state: int = 0
    train_rows: Optional[np.ndarray] = None          # row ids into X; None = all rows


@dataclass
class FittedMLP:
    config: MLPConfig
    coefs_: List[np.ndarray] = field(default_factory=list)
    intercepts_: List[np.ndarray] = field(default_factory=list)
    n_iter_: int = 0
    loss_: float = float("nan")
    best_loss_: float = float("inf")
    loss_curve_: List[float] = field(default_factory=list)
    converged_: bool = False                        # stopped by the tol rule (not by max_iter)
    _trainer: "GridMLPTrainer" = None
    _index: int = -1

    def predict_proba(self, X) -> np.ndarray:
        p1 = self._trainer._predict(self._index, X)
        return np.stack([1.0 - p1, p1], axis=1)

    def predict(self, X) -> np.ndarray:
        return (self._trainer._predict(self._index, X) > 0.5).astype(np.int64)


class GridMLPTrainer:
    """Trains many small MLP classifiers at once on one GPU.  ``X``: [n, n_features] float64, ``y``: [n] in {0, 1}."""

    def __init__(self, X, y, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GridMLPTrainer needs a GPU (no CPU fallback)")
        on_device = isinstance(X, torch.Tensor) and X.is_cuda      # a CUDA tensor stays where it is (ensemble: one upload for all learners);
        if not on_device:                                           # whatever else numpy can read, a CPU tensor included, goes the way it always went
            X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if len(X.shape) != 2 or y.shape != (X.shape[0],):
            raise ValueError(f"X must be [n, features] and y [n]; got {tuple(X.shape)} and {y.shape}")
        if not np.isin(y, (0.0, 1.0)).all():
            raise ValueError("y must be binary {0, 1} (binarise labels first, as MLPClassifier does)")
        self.n, self.n_features = (int(v) for v in X.shape)
        self.X = X.to(self.device, torch.float64).contiguous() if on_device else torch.from_numpy(X).to(self.device)
        self.y = torch.from_numpy(y).to(self.device)
        self._models_dev = None
        self._keep = []

    # ---- host replica of the estimator's RandomState protocol -------------------------------------------------------
    @staticmethod
    def _init_params(cfg: MLPConfig, units, rs):
        parts = []
        for fan_in, fan_out in zip(units[:-1], units[1:]):
            bound = np.sqrt(6.0 / (fan_in + fan_out))            # relu / tanh: factor 6 (sklearn _init_coef)
            parts.append(rs.uniform(-bound, bound, (fan_in, fan_out)).ravel())
            parts.append(rs.uniform(-bound, bound, fan_out))
        return np.concatenate(parts)

    def fit(self, configs: Sequence[MLPConfig], epochs_per_launch: int = 8) -> List[FittedMLP]:
        """Round 4 host side: (i) the fits sit in the device array in order of DECREASING cost (mini-batches per epoch x parameters): the
        work-groups of a launch are handed out in array order and a work-group is a whole CU, so the few fits that do not get a CU at once
        (270 fits, 256 CUs) are the cheapest ones instead of whatever the grid's order put last; (ii) the visiting orders of chunk k + 1 --
        every estimator's own RandomState stream, 270 x epochs shuffles of ~5000 rows on the host -- are drawn WHILE the GPU trains chunk k
        and travel as one pinned copy on a second stream (they used to sit between two launches: ~20 ms per epoch of the reference grid)."""
        L = _lib.lib()
        nm = len(configs)
        if nm == 0:
            return []
        dev = self.device
        E = int(epochs_per_launch)
        host, streams = [], {}
        for i, cfg in enumerate(configs):
            if cfg.activation not in _ACT:
                raise ValueError(f"activation {cfg.activation!r}: the reference grid uses relu and tanh")
            hidden = list(cfg.hidden_layer_sizes)
            if not 1 <= len(hidden) <= 3 or max(hidden) > 256 or min(hidden) < 1:
                raise ValueError("1 to 3 hidden layers of 1 to at most 256 units")
            if int(cfg.batch_size) < 1 or int(cfg.max_iter) < 1:
                raise ValueError("batch_size and max_iter must be at least 1")
            rows = np.arange(self.n) if cfg.train_rows is None else np.asarray(cfg.train_rows, dtype=np.int64)
            # the kernel gathers rows of X by these ids without a bounds check of its own
            if rows.ndim != 1 or rows.size < 1 or rows.min() < 0 or rows.max() >= self.n:
                raise ValueError(f"train_rows must be a non-empty vector of row ids in [0, {self.n})")
            n_train = len(rows)
            units = [self.n_features] + hidden + [1]
            # Fits that share (integer random_state, layer sizes, number of training rows) -- in the reference grid all folds, activations,
            # learning rates and batch sizes of one hidden_layer_sizes value: 90 of 270 -- consume ONE and the same RandomState stream:
            # identical initial parameters and identical shuffles.  The stream is run once per group (init: 270 -> 3 draws of up to 40 k
            # uniforms, 68 ms -> 1 ms on the bench box; shuffles: 270 -> 3 per epoch) and every member indexes its own rows with it.
            shared = isinstance(cfg.random_state, (int, np.integer))
            skey = (int(cfg.random_state), tuple(units), n_train) if shared else ("own", i)
            st = streams.get(skey)
            if st is None:
                rs = np.random.RandomState(cfg.random_state)
                st = streams[skey] = dict(rs=rs, p0=self._init_params(cfg, units, rs), idx=np.arange(n_train), orders={}, made=0)
            p0 = st["p0"]
            bs = min(int(cfg.batch_size), n_train)
            cost = -(-n_train // bs) * (len(p0) + 4000)          # mini-batches per epoch x (parameters + a per-update constant)
            host.append(dict(cfg=cfg, rows=rows, stream=st, units=units, p0=p0, bs=bs, n_train=n_train, cost=cost))
        slot_of = np.argsort([-h["cost"] for h in host], kind="stable")      # slot k of the device array holds fit slot_of[k]
        # one device buffer for every fit's visiting orders, two halves (the chunk being trained / the chunk being drawn)
        offs, tot = [], 0
        for k in range(nm):
            offs.append(tot); tot += E * host[slot_of[k]]["n_train"]
        orders_dev = torch.empty((2, tot), dtype=torch.int32, device=dev)
        orders_host = [torch.empty(tot, dtype=torch.int32).pin_memory() for _ in range(2)]
        # one device buffer per kind for ALL fits (270 fits x 7 small tensors were 1900 allocations and 270 host-to-device copies per fit() call)
        p_off, a_off, c_off, ptot, atot, ctot = [], [], [], 0, 0, 0
        for k in range(nm):
            h = host[slot_of[k]]
            p_off.append(ptot); ptot += len(h["p0"])
            a_off.append(atot); atot += h["bs"] * sum(h["units"][1:])
            c_off.append(ctot); ctot += h["cfg"].max_iter
        params_all = torch.from_numpy(np.concatenate([host[slot_of[k]]["p0"] for k in range(nm)])).to(dev)
        m_all, v_all, g_all = (torch.zeros(ptot, dtype=torch.float64, device=dev) for _ in range(3))
        act_all, delta_all = (torch.zeros(atot, dtype=torch.float64, device=dev) for _ in range(2))
        curve_all = torch.zeros(ctot, dtype=torch.float64, device=dev)
        self._buffers = (params_all, m_all, v_all, g_all, act_all, delta_all, curve_all)
        structs = (_lib.MlpModel * nm)()
        for k in range(nm):
            h = host[slot_of[k]]
            cfg, units, p0, bs, n_train = h["cfg"], h["units"], h["p0"], h["bs"], h["n_train"]
            np_, na = len(p0), bs * sum(units[1:])
            t = dict(params=params_all[p_off[k]:p_off[k] + np_], m=m_all[p_off[k]:p_off[k] + np_], v=v_all[p_off[k]:p_off[k] + np_],
                     g=g_all[p_off[k]:p_off[k] + np_], act=act_all[a_off[k]:a_off[k] + na], delta=delta_all[a_off[k]:a_off[k] + na],
                     curve=curve_all[c_off[k]:c_off[k] + cfg.max_iter])
            h["t"], h["slot"] = t, k
            s = structs[k]
            s.n_layers = len(units) - 1
            for q, u in enumerate(units):
                s.units[q] = u
            s.activation, s.batch_size, s.n_train = _ACT[cfg.activation], bs, n_train
            s.n_iter_no_change, s.max_iter = cfg.n_iter_no_change, cfg.max_iter
            s.lr_init, s.alpha, s.beta1, s.beta2, s.eps, s.tol = (cfg.learning_rate_init, cfg.alpha, cfg.beta_1, cfg.beta_2,
                                                                    cfg.epsilon, cfg.tol)
            s.params, s.adam_m, s.adam_v, s.grads = (t["params"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                                                     t["g"].data_ptr())
            s.act, s.delta, s.loss_curve = t["act"].data_ptr(), t["delta"].data_ptr(), t["curve"].data_ptr()
            s.order = orders_dev[0].data_ptr() + 4 * offs[k]
            s.t, s.best_loss, s.no_improve, s.n_iter, s.done = 0, float("inf"), 0, 0, 0
        nbytes = ctypes.sizeof(structs)
        models_dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        staging = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        copy_stream = torch.cuda.Stream(device=dev)

        def draw(half, live_slots, n_epochs):
            """the next n_epochs epochs' visiting orders of the live fits, from each estimator's own RandomState stream, into half `half`
            (never more than a fit has left to run)"""
            buf = orders_host[half].numpy()
            for k in live_slots:
                h = host[slot_of[k]]
                n_train = h["n_train"]
                todo = min(n_epochs, h["cfg"].max_iter - h["drawn"])
                st = h["stream"]
                for e in range(todo):
                    ae = h["drawn"] + e                       # absolute epoch of this fit = position in its group's stream
                    while st["made"] <= ae:
                        # == sample_idx = sklearn.utils.shuffle(sample_idx, random_state=rs): resample() shuffles arange(n)
                        # with the RandomState and indexes the array with it
                        perm = np.arange(n_train)
                        st["rs"].shuffle(perm)
                        st["idx"] = st["idx"][perm]
                        st["orders"][st["made"]] = st["idx"]
                        st["made"] += 1
                    buf[offs[k] + e * n_train: offs[k] + (e + 1) * n_train] = h["rows"][st["orders"][ae]]
                h["drawn"] += max(todo, 0)
            floors = {}
            for k in live_slots:                              # drop the epochs every live member of a group has passed
                h = host[slot_of[k]]
                floors[id(h["stream"])] = min(floors.get(id(h["stream"]), h["drawn"]), h["drawn"])
            for st in streams.values():
                floor = floors.get(id(st), st["made"])
                for ae in [a for a in st["orders"] if a < floor]:
                    del st["orders"][ae]
            with torch.cuda.stream(copy_stream):
                orders_dev[half].copy_(orders_host[half], non_blocking=True)

        # chunk sizes 1, 2, 4, ... E epochs: only the FIRST chunk's orders are drawn with the GPU idle (16 ms per epoch of the reference grid on
        # the host against 45 ms on the GPU: a chunk twice as long as the one being trained is still drawn in its shadow)
        live = list(range(nm))
        for h in host:
            h["drawn"] = 0
        chunk = 1
        draw(0, live, chunk)
        copy_stream.synchronize()
        half = 0
        while live:
            for k in live:
                structs[k].order = orders_dev[half].data_ptr() + 4 * offs[k]
            ctypes.memmove(staging.data_ptr(), ctypes.addressof(structs), nbytes)
            models_dev.copy_(staging, non_blocking=False)
            torch.cuda.current_stream(dev).wait_stream(copy_stream)
            _lib.check(L.bbbp_mlp_train_epochs(ops._stream(), models_dev.data_ptr(), nm, self.X.data_ptr(), self.y.data_ptr(),
                                               self.n_features, chunk), "bbbp_mlp_train_epochs")
            chunk = min(E, 2 * chunk)
            draw(half ^ 1, live, chunk)                    # host work + the copy run beside the kernel (fits that finish in this chunk: wasted, harmless)
            staging.copy_(models_dev)                      # synchronises with the kernel
            ctypes.memmove(ctypes.addressof(structs), staging.data_ptr(), nbytes)
            live = [k for k in live if not structs[k].done]
            half ^= 1
        copy_stream.synchronize()
        self._models_dev, self._structs = models_dev, structs
        self._keep = host
        self._orders = (orders_dev, orders_host)
        out = []
        params_host, curve_host = params_all.cpu().numpy(), curve_all.cpu().numpy()
        for i, h in enumerate(host):
            s, cfg, units = structs[h["slot"]], h["cfg"], h["units"]
            p = params_host[p_off[h["slot"]]:p_off[h["slot"]] + len(h["p0"])]
            coefs, inter, off = [], [], 0
            for fan_in, fan_out in zip(units[:-1], units[1:]):
                coefs.append(p[off:off + fan_in * fan_out].reshape(fan_in, fan_out).copy()); off += fan_in * fan_out
                inter.append(p[off:off + fan_out].copy()); off += fan_out
            curve = curve_host[c_off[h["slot"]]:c_off[h["slot"]] + s.n_iter].tolist()
            out.append(FittedMLP(config=cfg, coefs_=coefs, intercepts_=inter, n_iter_=int(s.n_iter), loss_=curve[-1] if curve else float("nan"),
                                 best_loss_=float(s.best_loss), loss_curve_=curve, converged_=bool(s.no_improve > cfg.n_iter_no_change),
                                 _trainer=self, _index=i))
        return out

    def _predict(self, index: int, X) -> np.ndarray:
        if self._models_dev is None:
            raise RuntimeError("predict before fit")
        return self._predict_device(index, torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(self.device)).cpu().numpy()

    def _predict_device(self, index: int, Xd):
        """P(class 1) of fit ``index`` for the float64 device rows ``Xd``: float64 [m] on the device."""
        if self._models_dev is None:
            raise RuntimeError("predict before fit")
        if Xd.dim() != 2 or Xd.shape[1] != self.n_features:
            raise ValueError(f"X must be [n, {self.n_features}]")
        Xd = Xd.to(self.device, torch.float64).contiguous()
        out = torch.empty(Xd.shape[0], dtype=torch.float64, device=self.device)
        max_units = max(self._keep[index]["units"][1:])
        _lib.check(_lib.lib().bbbp_mlp_predict_proba(ops._stream(), self._models_dev.data_ptr(), self._keep[index]["slot"], Xd.data_ptr(), Xd.shape[0],
                                                     self.n_features, max_units, out.data_ptr()), "bbbp_mlp_predict_proba")
        return out


def grid_search_cv(X, y, param_grid: dict, cv: int = 5, base: Optional[MLPConfig] = None, device="cuda", random_state: int = 0):
    """The reference's ``GridSearchCV(MLPClassifier(...), param_grid, cv=5, scoring='f1')`` (model_opt_maccs.py:183-184) as
    one batched GPU run: every (parameter point, fold) pair is one model.  Folds are scikit-learn's StratifiedKFold (what
    GridSearchCV uses for classifiers).  Returns (best_params, mean_f1 per point, all fitted models)."""
    from itertools import product
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold
    base = base or MLPConfig()
    keys = sorted(param_grid)
    points = [dict(zip(keys, vals)) for vals in product(*(param_grid[k] for k in keys))]
    folds = list(StratifiedKFold(n_splits=cv).split(X, y))
    configs = []
    for pt in points:
        for tr, _ in folds:
            kw = {**base.__dict__, **{k: v for k, v in pt.items() if k != "solver"}, "train_rows": tr, "random_state": random_state}
            configs.append(MLPConfig(**kw))
    trainer = GridMLPTrainer(X, y, device=device)
    fitted = trainer.fit(configs)
    scores = []
    X = np.asarray(X, dtype=np.float64); y = np.asarray(y)
    for pi in range(len(points)):
        f1 = [f1_score(y[te], fitted[pi * len(folds) + fi].predict(X[te])) for fi, (_, te) in enumerate(folds)]
        scores.append(float(np.mean(f1)))
    best = int(np.argmax(scores))
    return points[best], scores, fitted


# ---- the estimator: one fit of the trainer with scikit-learn's MLPClassifier surface -------------------------------------------------------
_MLP_DEFAULTS = dict(learning_rate="constant", power_t=0.5, shuffle=True, verbose=False, warm_start=False, momentum=0.9, nesterovs_momentum=True,
                     early_stopping=False, validation_fraction=0.1, beta_1=0.9, beta_2=0.999, epsilon=1e-8, max_fun=15000)


class MLPClassifier(_estimator.Params):
    """``MLPClassifier(hidden_layer_sizes=(100,), activation="relu", *, solver="adam", alpha=1e-4, batch_size="auto",
    learning_rate_init=0.001, max_iter=200, tol=1e-4, n_iter_no_change=10, random_state=0, device="cuda")``: scikit-learn's names for two
    classes, a thin estimator over ``GridMLPTrainer`` with one ``MLPConfig``.

    ``fit`` takes a numpy array or a CUDA tensor [n, d] (trained in float64) and labels with two distinct values; ``classes_[1]`` is the
    positive class.  ``batch_size="auto"`` is ``min(200, n)``.  It sets ``classes_``, ``coefs_``, ``intercepts_``, ``n_iter_``, ``loss_``,
    ``best_loss_``, ``loss_curve_`` and ``n_features_in_``.  ``predict_proba`` returns float64 [m, 2] as ``[1 - p, p]`` (numpy for numpy
    input, a CUDA tensor for a CUDA tensor); ``predict`` returns numpy labels, ``classes_[1]`` where ``p > 0.5``.  ``get_params`` /
    ``set_params`` make the estimator clonable, so ``ensemble.StackingClassifier`` takes it as a base learner.
    A fitted estimator predicts through the trainer that fitted it and keeps it: the trainer's float64 copy of the training matrix, and
    the models fitted beside it in the same batch (``ensemble`` fits six at once), stay on the device for the estimator's lifetime.

    Refused by name, being what the trainer does not implement: solvers other than ``"adam"``, activations other than ``"relu"`` and
    ``"tanh"``, more than three hidden layers or 256 units in one, ``early_stopping``, ``warm_start``, ``shuffle=False``, other values of
    ``beta_1``, ``beta_2``, ``epsilon``, a ``random_state`` that is not an int (the seed is part of the model), ``sample_weight``,
    ``partial_fit``, more than two classes, a device other than CUDA."""

    _who = "MLPClassifier"
    _params = ("hidden_layer_sizes", "activation", "solver", "alpha", "batch_size", "learning_rate_init", "max_iter", "tol", "n_iter_no_change",
               "random_state", "device")

    def __init__(self, hidden_layer_sizes=(100,), activation="relu", *, solver="adam", alpha=1e-4, batch_size="auto", learning_rate_init=0.001,
                 max_iter=200, tol=1e-4, n_iter_no_change=10, random_state=0, device="cuda", **other):
        from . import _tree_host
        who = self._who
        _tree_host.refuse_non_defaults(who, other, _MLP_DEFAULTS)
        if solver != "adam":
            raise NotImplementedError(f"{who}: solver={solver!r} is not supported (only 'adam')")
        if activation not in _ACT:
            raise NotImplementedError(f"{who}: activation={activation!r} is not supported (only {sorted(_ACT)})")
        hidden = [hidden_layer_sizes] if _tree_host.is_int(hidden_layer_sizes) else list(hidden_layer_sizes)
        if not all(_tree_host.is_int(h) for h in hidden) or not 1 <= len(hidden) <= 3 or min(hidden) < 1 or max(hidden) > 256:
            raise NotImplementedError(f"{who}: hidden_layer_sizes={hidden_layer_sizes!r} is not supported (1 to 3 hidden layers of 1 to 256 units)")
        if not (batch_size == "auto" if isinstance(batch_size, str) else (_tree_host.is_int(batch_size) and batch_size >= 1)):
            raise ValueError(f"{who}: batch_size must be 'auto' or an int >= 1, got {batch_size!r}")
        for name, value, low in (("alpha", alpha, 0.0), ("learning_rate_init", learning_rate_init, None), ("tol", tol, 0.0)):
            ok = isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool) and np.isfinite(value)
            if not ok or (value <= 0.0 if low is None else value < low):
                raise ValueError(f"{who}: {name} must be a finite number {'> 0' if low is None else '>= 0'}, got {value!r}")
        for name, value in (("max_iter", max_iter), ("n_iter_no_change", n_iter_no_change)):
            if not _tree_host.is_int(value) or value < 1:
                raise ValueError(f"{who}: {name} must be an int >= 1, got {value!r}")
        if not _tree_host.is_int(random_state) or not 0 <= random_state < 2 ** 32:
            raise NotImplementedError(f"{who}: random_state must be an int in [0, 2^32) (the seed is part of the model), got {random_state!r}")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: the fits run on the GPU (no CPU fallback)")
        # the parameters are kept as they were given, so that a clone is made of the same values
        self.hidden_layer_sizes, self.activation, self.solver, self.alpha, self.batch_size = hidden_layer_sizes, activation, solver, alpha, batch_size
        self.learning_rate_init, self.max_iter, self.tol, self.n_iter_no_change = learning_rate_init, max_iter, tol, n_iter_no_change
        self.random_state, self.device = random_state, device

    # ---- fit --------------------------------------------------------------------------------------------------------
    def _config(self, n_train, train_rows=None):
        from . import _tree_host
        hidden = [self.hidden_layer_sizes] if _tree_host.is_int(self.hidden_layer_sizes) else list(self.hidden_layer_sizes)
        bs = min(200, n_train) if isinstance(self.batch_size, str) else int(self.batch_size)
        return MLPConfig(hidden_layer_sizes=tuple(int(h) for h in hidden), activation=self.activation, learning_rate_init=float(self.learning_rate_init),
                         batch_size=bs, alpha=float(self.alpha), max_iter=int(self.max_iter), tol=float(self.tol),
                         n_iter_no_change=int(self.n_iter_no_change), random_state=int(self.random_state), train_rows=train_rows)

    @staticmethod
    def _fit_rows(clones, X, y, row_sets):
        """Fit ``clones[i]`` on the rows ``row_sets[i]`` (None: all) of ``X`` (numpy or a CUDA tensor) and ``y``: one trainer, one batch of
        fits, the rows gathered by the kernel (``MLPConfig.train_rows``).  Each fit equals the single ``fit`` on those rows."""
        from .linear_model import _binary_targets
        who = clones[0]._who
        if isinstance(y, torch.Tensor):
            y = y.detach().cpu().numpy()
        y = np.asarray(y)
        if len(X.shape) != 2 or X.shape[0] != len(y):
            raise ValueError(f"{who}: X must be [n, d] with one label per row, got {tuple(X.shape)} and {len(y)} labels")
        classes, t_all = _binary_targets(y, None, who)
        configs = []
        for c, rows in zip(clones, row_sets):
            rows = None if rows is None else np.asarray(rows, dtype=np.int64)
            # one label vector serves every fit: a row set must hold both classes of all rows
            if rows is not None and not np.array_equal(np.unique(y[rows]), classes):
                raise ValueError(f"{who}: a row set's classes {np.unique(y[rows])!r} differ from those of all rows {classes!r}")
            configs.append(c._config(len(y) if rows is None else len(rows), rows))
        trainer = GridMLPTrainer(X, t_all, device=clones[0].device)
        for c, fitted in zip(clones, trainer.fit(configs)):
            c._adopt(classes, fitted, int(X.shape[1]))
        return clones

    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError(f"{self._who}: sample_weight is not supported")
        self._fit_rows([self], X, y, [None])
        return self

    def partial_fit(self, X, y, classes=None):
        raise NotImplementedError(f"{self._who}: partial_fit is not supported")

    def _adopt(self, classes, fitted, n_features):
        self.classes_, self._fitted, self.n_features_in_ = classes, fitted, n_features
        self.coefs_, self.intercepts_, self.n_iter_ = fitted.coefs_, fitted.intercepts_, fitted.n_iter_
        self.loss_, self.best_loss_, self.loss_curve_ = fitted.loss_, fitted.best_loss_, fitted.loss_curve_
        self.n_layers_, self.out_activation_ = len(fitted.coefs_) + 1, "logistic"

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _p1(self, X):
        """(P(classes_[1]) float64 [m] on the device, was_numpy)."""
        if not hasattr(self, "_fitted"):
            raise RuntimeError(f"{self._who}: not fitted")
        was_numpy = not isinstance(X, torch.Tensor)
        trainer = self._fitted._trainer
        if was_numpy:
            X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64))
        elif not X.is_cuda:
            raise RuntimeError(f"{self._who}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU fallback)")
        if X.dim() != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError(f"{self._who}: the queries must be [m, {self.n_features_in_}], got shape {tuple(X.shape)}")
        with torch.cuda.device(trainer.device):
            return trainer._predict_device(self._fitted._index, X.to(trainer.device)), was_numpy

    def predict_proba(self, X):
        p, was_numpy = self._p1(X)
        out = torch.stack([1.0 - p, p], dim=1)
        return out.cpu().numpy() if was_numpy else out

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype: ``classes_[1]`` where P(``classes_[1]``) > 0.5 (scikit-learn's rule)."""
        p, _ = self._p1(X)
        return self.classes_[(p > 0.5).cpu().numpy().astype(np.intp)]
