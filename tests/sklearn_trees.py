"""scikit-learn's fitted trees in the flat convention of ``trees_``, for the replayers (gbt_replay, gbr_replay, rf_replay, rfr_replay).

A restatement on the test side: it does not import the package's own flattening, since a certifier must not share code with what it
certifies."""
import numpy as np


def trees_of_sklearn(fitted):
    """The trees of a fitted scikit-learn booster (its one column of ``estimators_``), forest or single tree: absolute child indices, -1 at a
    leaf, ``root[t]`` the first node of tree t.  ``value`` is the last entry of every node's value: the node mean of a regression tree, the
    class-1 share of a two-class tree."""
    ests = list(np.ravel(fitted.estimators_)) if hasattr(fitted, "estimators_") else [fitted]
    left, right, feature, threshold, value, nns, root = [], [], [], [], [], [], [0]
    for est in ests:
        t, off = est.tree_, root[-1]
        left.append(np.where(t.children_left >= 0, t.children_left + off, -1))
        right.append(np.where(t.children_right >= 0, t.children_right + off, -1))
        feature.append(np.where(t.feature >= 0, t.feature, 0))
        threshold.append(t.threshold)
        value.append(t.value[:, 0, -1])
        nns.append(t.n_node_samples)
        root.append(off + t.node_count)
    cat = np.concatenate
    return dict(left=cat(left).astype(np.int32), right=cat(right).astype(np.int32), feature=cat(feature).astype(np.int32), threshold=cat(threshold),
                value=cat(value).astype(np.float64), n_node_samples=cat(nns).astype(np.int32), root=np.asarray(root, dtype=np.int32))
