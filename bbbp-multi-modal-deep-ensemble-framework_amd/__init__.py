"""bbbp-multi-modal-deep-ensemble-framework_amd: MI355X (gfx950) implementation of the neural hot path of
FengDushuo/BBBP-Multi-Modal-Deep-Ensemble-Framework (import it as ``bbbp_amd``).

Layout:  csrc/ (HIP kernels + the C ABI of include/bbbp_hip.h), _lib.py (ctypes binding), ops.py (tensor
front end), models.py (the reference's nn.Module interface), optim.py (fused AdamW), ensemble.py (stacked
predict surface of the regression scripts; StackingClassifier and VotingClassifier over the classifiers, assembled on the GPU), trees.py / boosters.py (random-forest and XGBoost prediction), preprocessing.py (float64 StandardScaler and PolynomialFeatures, the two steps in front of everything else), decomposition.py (float64 PCA), neighbors.py (float64 k-nearest neighbours), svm.py (float64 support-vector classification, its Platt-scaled class probabilities, and regression), linear_model.py (float64 logistic regression), gradient_boosting.py (boosted classification trees fitted by exact split search), random_forest.py (random-forest and decision-tree classifiers and regressors fitted by exact split search), isolation_forest.py (outlier forest of random trees on sub-samples, fitted and scored on the GPU), naive_bayes.py (Bernoulli naive Bayes on packed bits: batched fits, grid search and learning curve), imbalance.py (SMOTE, TomekLinks and SMOTETomek resampling between the PCA and the learners), xgb.py (XGBoost's hist trees, quantised to bytes and fitted on the GPU: XGBRegressor for the squared error and XGBClassifier for binary:logistic with row and column sampling, batched fold fits and the reference's randomized search; the model is a boosters.XGBTrees), cat.py (CatBoost's Plain boosting of symmetric trees for RMSE, made deterministic and fitted on the GPU: CatBoostRegressor and batched fold fits; the model is a boosters.CatBoostTrees), metrics.py (batched classification and regression scores: confusion counts, AUC pair counts and squared-error sums per column and row segment), _tree_host.py (what the tree learners' host sides share; csrc/tree_fit.h is the device counterpart), distributed.py (one
process per GPU, RCCL gradient all-reduce).
"""
from .models import (ConcatMixedInputModel, MixedDataset, MixedInputModel, MSELoss, TwoBranchConcatModel,
                     MultiHeadAttentionFusion, flatten_parameters, reference_nhead)  # noqa: F401
from . import ops  # noqa: F401
from . import preprocessing  # noqa: F401
from . import decomposition  # noqa: F401
from . import neighbors  # noqa: F401
from . import svm  # noqa: F401
from . import linear_model  # noqa: F401
from . import gradient_boosting  # noqa: F401
from . import random_forest  # noqa: F401
from . import isolation_forest  # noqa: F401
from . import naive_bayes  # noqa: F401
from . import imbalance  # noqa: F401
from . import metrics  # noqa: F401
from . import xgb  # noqa: F401
from . import cat  # noqa: F401

__all__ = ["ConcatMixedInputModel", "TwoBranchConcatModel", "MixedDataset", "MixedInputModel", "MSELoss", "MultiHeadAttentionFusion", "flatten_parameters", "reference_nhead", "ops", "preprocessing", "decomposition", "neighbors", "svm", "linear_model", "gradient_boosting", "random_forest", "isolation_forest", "naive_bayes", "imbalance", "metrics", "xgb", "cat"]
