"""CPU: the numpy restatement of the fit kernels' logic (tests/gbt_numpy.py) passes the replayer on the shapes that stress it: two rows,
one row past a power of two, depth 7 with tiny nodes, min_samples_leaf > 1, duplicate values, and a copied column for the tie rule."""
import numpy as np
import pytest

import gbt_numpy
import gbt_replay as R


@pytest.mark.parametrize("n,d,depth,mss,msl,lr,variant", [(2, 1, 1, 2, 1, 0.1, None), (65, 3, 3, 5, 1, 0.1, None), (257, 5, 7, 2, 1, 0.1, None),
                                                          (257, 5, 3, 10, 3, 0.01, "copy"), (257, 5, 5, 2, 1, 0.1, "decimals")])
def test_restated_kernels_pass_the_replayer(n, d, depth, mss, msl, lr, variant):
    X, y = R.make_data(n, d, seed=1, decimals=1 if variant == "decimals" else None)
    y = y.astype(np.float64)
    if variant == "copy":
        X[:, 3] = X[:, 1]
    trees, init, stages, scores = gbt_numpy.fit(X, y, 4, lr, depth, mss, msl)
    seen = R.replay(X, y, trees, init, lr, depth, mss, msl, raw_stages=stages, train_score=scores)
    assert seen["leaves"] == seen["splits"] + 4                       # four trees, each with one leaf more than splits
    if variant == "copy":
        split = trees["left"] >= 0
        assert not (trees["feature"][split] == 3).any()
    # level-order numbering: a split node's children are consecutive and come after it
    split = np.nonzero(trees["left"] >= 0)[0]
    assert (trees["right"][split] == trees["left"][split] + 1).all() and (trees["left"][split] > split).all()
