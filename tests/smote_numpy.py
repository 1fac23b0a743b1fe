"""numpy restatement of imbalance.SMOTE, TomekLinks and SMOTETomek, written from imbalanced-learn's published source: the same draws on a
``numpy.random.RandomState`` in the same order, the same expression ``X[rows] + steps[:, None] * diffs`` with numpy's roundings, neighbours
from ``knn_oracle.knn(..., exclude_self=True)`` (a row left out by index, order (distance, index)).  tests/test_smote_cpu.py checks its
structure and, where imbalanced-learn is installed, pins it to that package; tests/test_gpu_smote.py holds the GPU to it bit for bit.

The GPU search selects with a centred expansion and is unique only where ``knn_oracle.min_gap_over_bound(...) > 1``: ``gap`` gives the
smallest ratio over a set, and every test that compares neighbour-dependent output asserts ``gap(...) > 1`` first."""
import numbers

import numpy as np

import knn_oracle

# (n, d, n_min, seed): tie-free under the search's bound for SMOTE at k = 5, seed 42, in float64 and float32, for the class searches and for
# the 1-NN search on the set Tomek sees (the original set and SMOTE's output); no duplicate rows.  The last one has no Tomek link on SMOTE's
# output, so it is not used for SMOTETomek.
PROBLEMS = [(65, 3, 7, 1), (130, 5, 40, 2), (257, 2, 64, 5), (300, 17, 100, 3), (1000, 100, 365, 4)]


def problem(n, d, n_min, seed, dtype="float64"):
    """Two classes: ``n_min`` rows of label 1, shifted by +0.5 in every column; every value exactly representable in float32."""
    X = knn_oracle.make_points(n, d, seed)
    y = np.zeros(n, dtype=np.int64)
    y[np.random.RandomState(seed + 5).permutation(n)[:n_min]] = 1
    X[y == 1] += 0.5
    return X.astype(np.float32).astype(dtype), y


def problem3(n, d, n_min, seed, dtype="float64", n_third=20):
    """``problem`` with a second minority (label 2) of ``n_third`` rows shifted by -0.5."""
    X = knn_oracle.make_points(n, d, seed)
    y = np.zeros(n, dtype=np.int64)
    perm = np.random.RandomState(seed + 5).permutation(n)
    y[perm[:n_min]] = 1
    y[perm[n_min:n_min + n_third]] = 2
    X[y == 1] += 0.5
    X[y == 2] -= 0.5
    return X.astype(np.float32).astype(dtype), y


def gap(X, k):
    """Smallest gap / bound over the rows of ``X`` searched for their ``k`` nearest other rows."""
    return float(knn_oracle.min_gap_over_bound(X, X, k, exclude_self=True).min())


def class_neighbours(Xc, k):
    return knn_oracle.knn(Xc, Xc, k, exclude_self=True)[1]


def _random_state(seed):
    return np.random.RandomState(seed) if isinstance(seed, numbers.Integral) else seed


def targets(y, strategy="auto"):
    """{class: n_new} in ascending class order, as imbalanced-learn resolves an over-sampler's ``sampling_strategy``."""
    classes, counts = np.unique(y, return_counts=True)
    stats = dict(zip(classes.tolist(), counts.tolist()))
    n_max = max(stats.values())
    maj, mino = max(stats, key=stats.get), min(stats, key=stats.get)
    if strategy in ("auto", "not majority"):
        return {c: n_max - m for c, m in stats.items() if c != maj}
    if strategy == "minority":
        return {mino: n_max - stats[mino]}
    if strategy == "not minority":
        return {c: n_max - m for c, m in stats.items() if c != mino}
    if strategy == "all":
        return {c: n_max - m for c, m in stats.items()}
    if isinstance(strategy, dict):
        return {c: strategy[c] - stats[c] for c in sorted(strategy)}
    assert len(stats) == 2
    return {c: int(strategy * n_max - m) for c, m in stats.items() if c != maj}


def smote(X, y, k=5, seed=42, strategy="auto", record=None):
    """(X_res, y_res).  ``record``, a list, receives (class, rows, neighbours, steps) per resampled class: synthetic row j of that class is
    ``Xc[rows[j]] + steps[j] * (Xc[neighbours[j]] - Xc[rows[j]])``, indices into the class's rows in their order in ``X``."""
    X_out, y_out = [X], [y]
    for c, n_new in targets(y, strategy).items():
        if n_new == 0:
            continue
        Xc = X[y == c]
        nn = class_neighbours(Xc, k)
        rs = _random_state(seed)                             # an int: a fresh stream per class; an instance continues
        idx = rs.randint(0, len(Xc) * k, size=n_new)
        steps = rs.uniform(size=n_new)
        rows, cols = idx // k, idx % k
        diffs = Xc[nn[rows, cols]] - Xc[rows]                # in X's dtype
        X_new = (Xc[rows] + steps[:, None] * diffs).astype(X.dtype)      # float64 arithmetic, one rounding to float32 for float32 input
        X_out.append(X_new)
        y_out.append(np.full(n_new, c, dtype=y.dtype))
        if record is not None:
            record.append((c, rows, nn[rows, cols], steps))
    return np.vstack(X_out), np.concatenate(y_out)


def tomek_members(X, y):
    """bool [n]: the rows that are members of a Tomek link."""
    nn1 = class_neighbours(X, 1)[:, 0]
    return (y[nn1] != y) & (nn1[nn1] == np.arange(len(y)))


def remove_set(y, strategy="auto"):
    classes, counts = np.unique(y, return_counts=True)
    maj, mino = classes[np.argmax(counts)], classes[np.argmin(counts)]
    if isinstance(strategy, str):
        return {"auto": [c for c in classes if c != mino], "not minority": [c for c in classes if c != mino],
                "not majority": [c for c in classes if c != maj], "majority": [maj], "all": list(classes)}[strategy]
    return list(strategy)


def tomek(X, y, remove="auto"):
    """(X_res, y_res, sample_indices): the link members whose class is in ``remove`` (a strategy name or a list of classes) are dropped."""
    drop = tomek_members(X, y) & np.isin(y, remove_set(y, remove))
    keep = np.flatnonzero(~drop)
    return X[keep], y[keep], keep


def smote_tomek(X, y, k=5, seed=42, strategy="auto"):
    X_res, y_res = smote(X, y, k, seed, strategy)
    return tomek(X_res, y_res, "all")[:2]
