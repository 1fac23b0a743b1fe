"""ctypes binding of libbbbp_hip.so (the C ABI declared in include/bbbp_hip.h).

The product path has NO fallback: if the library is missing, or a call fails, a RuntimeError is
raised.  Nothing here imports torch; device pointers arrive as integers.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BBBP_LIB", os.path.join(_HERE, "libbbbp_hip.so"))    # BBBP_LIB: A/B another build
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bbbp_hip.h")

_lib = None


class MixedDesc(Structure):
    """bbbp_mixed_desc (include/bbbp_hip.h)."""
    _fields_ = [("batch", c_int), ("fingerprint_size", c_int), ("nhead", c_int), ("num_layers", c_int),
                ("dim_feedforward", c_int), ("training", c_int), ("dropout_p", c_float), ("seed", c_uint64),
                ("need_input_grad", c_int), ("fusion", c_int), ("inference", c_int),
                ("world", c_int), ("rank", c_int), ("collective", c_void_p), ("collective_ctx", c_void_p)]


# bbbp_collective_fn (include/bbbp_hip.h): ctx, op, what, layer, send_off, recv_off, count, stream
CollectiveFn = ctypes.CFUNCTYPE(c_int, c_void_p, c_int, c_int, c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, c_void_p)


class GemmDesc(Structure):
    """bbbp_gemm_desc (include/bbbp_hip.h)."""
    _fields_ = [("transA", c_int), ("transB", c_int), ("M", c_int), ("N", c_int), ("K", c_int), ("alpha", c_float),
                ("A", c_void_p), ("lda", c_int), ("B", c_void_p), ("ldb", c_int), ("C", c_void_p), ("ldc", c_int),
                ("bias", c_void_p), ("residual", c_void_p), ("ldr", c_int), ("act", c_int),
                ("gate", c_void_p), ("ldg", c_int), ("gate_scale", c_float), ("batch", c_int),
                ("strideA", c_long), ("strideB", c_long), ("strideC", c_long), ("strideR", c_long), ("strideG", c_long),
                ("gate_after_residual", c_int), ("asum", c_void_p), ("drop_p", c_float), ("drop_seed", c_uint64)]


class MlpModel(Structure):
    """bbbp_mlp_model (include/bbbp_hip.h)."""
    _fields_ = [("n_layers", c_int), ("units", c_int * 5), ("activation", c_int), ("batch_size", c_int), ("n_train", c_int),
                ("n_iter_no_change", c_int), ("max_iter", c_int),
                ("lr_init", ctypes.c_double), ("alpha", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("tol", ctypes.c_double),
                ("params", c_void_p), ("adam_m", c_void_p), ("adam_v", c_void_p), ("grads", c_void_p),
                ("act", c_void_p), ("delta", c_void_p), ("order", c_void_p), ("loss_curve", c_void_p),
                ("t", c_long), ("best_loss", ctypes.c_double), ("no_improve", c_int), ("n_iter", c_int), ("done", c_int)]


class GemmF64cDesc(Structure):
    """bbbp_gemm_f64c_desc (include/bbbp_hip.h)."""
    _fields_ = [("layout", c_int), ("M", c_int), ("N", c_int), ("K", c_int),
                ("A", c_void_p), ("a_dtype", c_int), ("lda", c_long), ("B", c_void_p), ("b_dtype", c_int), ("ldb", c_long),
                ("a_shift", c_void_p), ("b_shift", c_void_p), ("row_scale", c_void_p),
                ("C", c_void_p), ("c_dtype", c_int), ("ldc", c_long), ("symmetric", c_int), ("split_k", c_int)]


class KnnDesc(Structure):
    """bbbp_knn_desc (include/bbbp_hip.h)."""
    _fields_ = [("m", c_int), ("n", c_int), ("d", c_int), ("k", c_int),
                ("Q", c_void_p), ("q_dtype", c_int), ("ldq", c_long), ("T", c_void_p), ("t_dtype", c_int), ("ldt", c_long),
                ("mu", c_void_p), ("q_norm", c_void_p), ("t_norm", c_void_p), ("dist", c_void_p), ("ind", c_void_p),
                ("exclude_self", c_int), ("slices", c_int)]


class SvmKernelDesc(Structure):
    """bbbp_svm_kernel_desc (include/bbbp_hip.h)."""
    _fields_ = [("n", c_int), ("d", c_int), ("kernel", c_int), ("gamma", c_double),
                ("X", c_void_p), ("x_dtype", c_int), ("ldx", c_long), ("mu", c_void_p), ("norms", c_void_p), ("K", c_void_p), ("ldk", c_long)]


class SvmProblem(Structure):
    """bbbp_svm_problem (include/bbbp_hip.h)."""
    _fields_ = [("K", c_void_p), ("ldk", c_long), ("rows", c_void_p), ("y", c_void_p), ("alpha", c_void_p), ("grad", c_void_p), ("diag", c_void_p),
                ("rho", c_void_p), ("n_iter", c_void_p), ("done", c_void_p), ("n", c_int), ("C", c_double), ("tol", c_double)]


class SvmDecisionDesc(Structure):
    """bbbp_svm_decision_desc (include/bbbp_hip.h)."""
    _fields_ = [("m", c_int), ("n_sv", c_int), ("d", c_int), ("kernel", c_int), ("gamma", c_double),
                ("Q", c_void_p), ("q_dtype", c_int), ("ldq", c_long), ("SV", c_void_p), ("sv_dtype", c_int), ("ldsv", c_long),
                ("mu", c_void_p), ("q_norm", c_void_p), ("sv_norm", c_void_p), ("coef", c_void_p), ("intercept", c_double), ("out", c_void_p),
                ("slices", c_int)]


class SvrProblem(Structure):
    """bbbp_svr_problem (include/bbbp_hip.h)."""
    _fields_ = [("K", c_void_p), ("ldk", c_long), ("rows", c_void_p), ("t", c_void_p), ("alpha", c_void_p), ("grad", c_void_p), ("diag", c_void_p),
                ("rho", c_void_p), ("n_iter", c_void_p), ("done", c_void_p), ("n", c_int), ("C", c_double), ("epsilon", c_double), ("tol", c_double)]


class SvmOofDesc(Structure):
    """bbbp_svm_oof_desc (include/bbbp_hip.h)."""
    _fields_ = [("K", c_void_p), ("ldk", c_long), ("n_rows", c_int), ("rows", c_void_p), ("y", c_void_p), ("alpha", c_void_p), ("rho", c_void_p),
                ("n", c_int), ("held", c_void_p), ("n_held", c_int), ("out", c_void_p)]


class SvmPlattProblem(Structure):
    """bbbp_svm_platt_problem (include/bbbp_hip.h)."""
    _fields_ = [("dec", c_void_p), ("y", c_void_p), ("n", c_int), ("ab", c_void_p), ("info", c_void_p)]


class LogregProblem(Structure):
    """bbbp_logreg_problem (include/bbbp_hip.h)."""
    _fields_ = [("X", c_void_p), ("x_dtype", c_int), ("ld", c_long), ("n", c_int), ("d", c_int), ("t", c_void_p), ("C", c_double), ("tol", c_double),
                ("fit_intercept", c_int), ("max_iter", c_int), ("theta", c_void_p), ("trial", c_void_p), ("state", c_void_p), ("flags", c_void_p)]


class RfTree(Structure):
    """bbbp_rf_tree (include/bbbp_hip.h)."""
    _fields_ = [("XT", c_void_p), ("order0", c_void_p), ("y", c_void_p), ("n", c_int), ("d", c_int), ("max_depth", c_int), ("min_samples_split", c_int),
                ("min_samples_leaf", c_int), ("max_features", c_int), ("bootstrap", c_int), ("tree_index", c_int), ("seed", c_uint64), ("work", c_void_p),
                ("left", c_void_p), ("right", c_void_p), ("feature", c_void_p), ("n_node_samples", c_void_p), ("threshold", c_void_p), ("value", c_void_p),
                ("value0", c_void_p), ("n_nodes", c_void_p)]


class GbtChain(Structure):
    """bbbp_gbt_chain (include/bbbp_hip.h)."""
    _fields_ = [("XT", c_void_p), ("order0", c_void_p), ("y", c_void_p), ("n", c_int), ("d", c_int), ("n_estimators", c_int), ("max_depth", c_int),
                ("min_samples_split", c_int), ("min_samples_leaf", c_int), ("learning_rate", c_double), ("init", c_double), ("work", c_void_p),
                ("left", c_void_p), ("right", c_void_p), ("feature", c_void_p), ("n_node_samples", c_void_p), ("threshold", c_void_p), ("value", c_void_p),
                ("tree_nodes", c_void_p), ("train_score", c_void_p), ("raw", c_void_p)]


class XgbProblem(Structure):
    """bbbp_xgb_problem (include/bbbp_hip.h)."""
    _fields_ = [("bins", c_void_p), ("cuts", c_void_p), ("y", c_void_p), ("n", c_int), ("d", c_int), ("cut_stride", c_int), ("n_estimators", c_int),
                ("max_depth", c_int), ("min_child_rows", c_int), ("reg_lambda", c_double), ("gamma", c_double), ("learning_rate", c_float),
                ("base_score", c_float), ("work", c_void_p), ("left", c_void_p), ("right", c_void_p), ("feature", c_void_p), ("cond", c_void_p),
                ("base_weight", c_void_p), ("loss_change", c_void_p), ("sum_hessian", c_void_p), ("tree_nodes", c_void_p), ("margin", c_void_p)]


class XgbcProblem(Structure):
    """bbbp_xgbc_problem (include/bbbp_hip.h)."""
    _fields_ = [("bins", c_void_p), ("cuts", c_void_p), ("y", c_void_p), ("n", c_int), ("d", c_int), ("cut_stride", c_int), ("n_estimators", c_int),
                ("max_depth", c_int), ("subsample_threshold", c_uint32), ("reg_lambda", c_double), ("gamma", c_double), ("min_child_weight", c_double),
                ("learning_rate", c_float), ("base_margin", c_float), ("seed", c_uint64), ("col_mask", c_void_p), ("col_mask_stride", c_int),
                ("work", c_void_p), ("left", c_void_p), ("right", c_void_p), ("feature", c_void_p), ("cond", c_void_p), ("base_weight", c_void_p),
                ("loss_change", c_void_p), ("sum_hessian", c_void_p), ("tree_nodes", c_void_p), ("margin", c_void_p)]


class CatProblem(Structure):
    """bbbp_cat_problem (include/bbbp_hip.h)."""
    _fields_ = [("bins", c_void_p), ("n_cuts", c_void_p), ("y", c_void_p), ("n", c_int), ("d", c_int), ("iterations", c_int), ("depth", c_int),
                ("l2_leaf_reg", c_double), ("learning_rate", c_double), ("bias", c_double), ("work", c_void_p), ("split_feature", c_void_p),
                ("split_bin", c_void_p), ("leaf_values", c_void_p), ("leaf_weights", c_void_p), ("tree_depth", c_void_p), ("approx", c_void_p)]


class CatcProblem(Structure):
    """bbbp_catc_problem (include/bbbp_hip.h)."""
    _fields_ = [("bins", c_void_p), ("n_cuts", c_void_p), ("t", c_void_p), ("weights", c_void_p), ("weight_stride", c_long), ("n", c_int), ("d", c_int),
                ("iterations", c_int), ("depth", c_int), ("l2_leaf_reg", c_double), ("learning_rate", c_double), ("bias", c_double), ("work", c_void_p),
                ("split_feature", c_void_p), ("split_bin", c_void_p), ("leaf_values", c_void_p), ("leaf_weights", c_void_p), ("tree_depth", c_void_p),
                ("approx", c_void_p)]


class EnsSource(Structure):
    """bbbp_ens_source (include/bbbp_hip.h)."""
    _fields_ = [("src", c_void_p), ("stride", c_long), ("col", c_long), ("rows", c_void_p), ("count", c_long), ("dst", c_long)]


class EnsColumn(Structure):
    """bbbp_ens_column (include/bbbp_hip.h)."""
    _fields_ = [("src", c_void_p), ("stride", c_long), ("col", c_long)]


_FP = c_void_p          # device float*
_PP = POINTER(c_void_p)  # host array of device pointers

ENCODER_ROWS_FWD_INPUTS = ("ctx", "xin", "wo", "bo", "g1", "be1", "w1", "b1", "w2", "b2", "g2", "be2")
ENCODER_ROWS_FWD_OUTPUTS = ("z1", "y1", "hff", "z2", "y2", "mean1", "rstd1", "mean2", "rstd2")
ENCODER_ROWS_BWD_INPUTS = ("z2", "mean2", "rstd2", "g2", "w2", "hff", "w1", "z1", "mean1", "rstd1", "g1", "wo")
ENCODER_ROWS_BWD_OUTPUTS = ("dz2", "dff", "dhff", "dy1", "dz1", "dsa", "dctx")


class EncoderRowsFwdDesc(Structure):
    """bbbp_encoder_rows_fwd_desc (include/bbbp_hip.h)."""
    _fields_ = ([("B", c_int), ("F", c_int), ("DFF", c_int), ("dropout_p", c_float), ("seed1", c_uint64), ("seed2", c_uint64), ("seed3", c_uint64)]
                + [(n, c_void_p) for n in ENCODER_ROWS_FWD_INPUTS]
                + [("wn", c_void_p), ("bn", c_void_p), ("outn", c_void_p), ("nn", c_int), ("ldn", c_int), ("actn", c_int)]
                + [(n, c_void_p) for n in ENCODER_ROWS_FWD_OUTPUTS])


class EncoderRowsBwdDesc(Structure):
    """bbbp_encoder_rows_bwd_desc (include/bbbp_hip.h)."""
    _fields_ = ([("B", c_int), ("F", c_int), ("DFF", c_int), ("dropout_p", c_float), ("seed1", c_uint64), ("seed3", c_uint64)]
                + [("dqkv_up", c_void_p), ("win_up", c_void_p), ("dz1_up", c_void_p), ("dyout", c_void_p)]
                + [(n, c_void_p) for n in ENCODER_ROWS_BWD_INPUTS] + [(n, c_void_p) for n in ENCODER_ROWS_BWD_OUTPUTS])

_SIGNATURES = {
    "bbbp_abi_version": (c_int, []),
    "bbbp_last_error": (c_char_p, []),
    "bbbp_gemm_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "bbbp_gemm_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, _FP, c_int, _FP, c_int, _FP, c_int,
                              _FP, _FP, c_int, c_int, c_int, c_long, c_long, c_long, c_long, c_void_p, c_size_t]),
    "bbbp_gemm_folds_asum": (c_int, [c_int, c_int, c_int, c_int]),
    "bbbp_gemm_f32_grouped": (c_int, [c_void_p, POINTER(GemmDesc), c_int, c_void_p, c_size_t]),
    "bbbp_gemm_kernel_form": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "bbbp_mixed_backward_wait_bucket": (c_int, [c_void_p, c_int]),
    "bbbp_mixed_backward_wait_released": (c_int, [c_void_p, c_int]),
    "bbbp_set_release_events": (c_int, [c_int]),
    "bbbp_mixed_bucket_param": (c_int, [POINTER(MixedDesc), c_int]),
    "bbbp_mixed_bucket_range": (c_int, [POINTER(MixedDesc), c_int, POINTER(c_int), POINTER(c_int)]),
    "bbbp_mixed_debug_ffn_gate": (c_int, [c_void_p, POINTER(MixedDesc), c_void_p, c_int, c_void_p]),
    "bbbp_mixed_debug_pool_mask": (c_int, [c_void_p, POINTER(MixedDesc), c_void_p, c_int, c_void_p]),
    "bbbp_set_graphs": (c_int, [c_int]),
    "bbbp_set_fused_head_bwd": (c_int, [c_int]),
    "bbbp_set_fused_encoder": (c_int, [c_int]),
    "bbbp_set_fold_outproj": (c_int, [c_int]),
    "bbbp_set_flash_attention": (c_int, [c_int]),
    "bbbp_attention_supported": (c_int, [c_int, c_int, c_int]),
    "bbbp_attention_keep_bytes": (c_size_t, [c_int, c_int, c_int]),
    "bbbp_attention_fwd": (c_int, [c_void_p, _FP, _FP, _FP, c_int, c_int, c_int, c_float, c_float, c_uint64, c_void_p]),
    "bbbp_attention_bwd": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_float, c_float, c_uint64, c_void_p]),
    "bbbp_attention_b3_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "bbbp_attention_b3_fwd": (c_int, [c_void_p, _FP, _FP, c_int, c_int, c_int, c_float, c_void_p, c_size_t]),
    "bbbp_outproj_fold_supported": (c_int, [c_int, c_int, c_int]),
    "bbbp_outproj_fold_fwd": (c_int, [c_void_p, c_int, c_int] + [_PP] * 7),
    "bbbp_outproj_fold_bwd": (c_int, [c_void_p, c_int, c_int] + [_FP] * 5 + [c_int] + [_FP] * 4),
    "bbbp_ln_param_grad": (c_int, [c_void_p, c_int] + [_PP] * 6 + [c_int, c_int]),
    "bbbp_encoder_rows_supported": (c_int, [c_int, c_int, c_int]),
    "bbbp_encoder_rows_fwd": (c_int, [c_void_p, POINTER(EncoderRowsFwdDesc)]),
    "bbbp_encoder_rows_bwd": (c_int, [c_void_p, POINTER(EncoderRowsBwdDesc)]),
    "bbbp_set_gemm_split_bf16": (c_int, [c_int]),
    "bbbp_set_gemm_fold_reduce": (c_int, [c_int]),
    "bbbp_gemm_split_bf16_phases": (c_int, [POINTER(c_uint64)]),
    "bbbp_gbt_predict": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                         c_void_p, c_void_p]),
    "bbbp_oblivious_predict": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                               c_double, c_double, c_void_p, c_void_p]),
    "bbbp_staged_count": (c_int, [c_int, c_int, c_int]),
    "bbbp_gbt_staged_predict": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                c_int, c_int, c_int, c_void_p, c_void_p, c_long]),
    "bbbp_oblivious_staged_predict": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                      c_double, c_double, c_int, c_int, c_int, c_void_p, c_void_p, c_long]),
    "bbbp_linear_layernorm_supported": (c_int, [c_int, c_int, c_int]),
    "bbbp_linear_layernorm_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_uint64]),
    "bbbp_layernorm_linear_supported": (c_int, [c_int, c_int, c_int]),
    "bbbp_layernorm_linear_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float,
                                  c_uint64, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int]),
    "bbbp_forest_groups": (c_int, [c_int]),
    "bbbp_forest_predict": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                    c_void_p, c_void_p]),
    "bbbp_mlp_train_epochs": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int]),
    "bbbp_mlp_predict_proba": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "bbbp_pca_col_mean": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_long, c_void_p]),
    "bbbp_gemm_f64c_workspace_bytes": (c_size_t, [POINTER(GemmF64cDesc)]),
    "bbbp_gemm_f64c": (c_int, [c_void_p, POINTER(GemmF64cDesc), c_void_p, c_size_t]),
    "bbbp_knn_row_norms": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    "bbbp_knn_workspace_bytes": (c_size_t, [POINTER(KnnDesc)]),
    "bbbp_knn_f64": (c_int, [c_void_p, POINTER(KnnDesc), c_void_p, c_size_t]),
    "bbbp_knn_vote": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p]),
    "bbbp_svm_kernel_matrix": (c_int, [c_void_p, POINTER(SvmKernelDesc)]),
    "bbbp_svm_smo": (c_int, [c_void_p, POINTER(SvmProblem), c_int, c_int]),
    "bbbp_svm_decision_workspace_bytes": (c_size_t, [POINTER(SvmDecisionDesc)]),
    "bbbp_svm_decision": (c_int, [c_void_p, POINTER(SvmDecisionDesc), c_void_p, c_size_t]),
    "bbbp_svr_smo": (c_int, [c_void_p, POINTER(SvrProblem), c_int, c_int]),
    "bbbp_svm_oof_decision": (c_int, [c_void_p, POINTER(SvmOofDesc), c_int]),
    "bbbp_svm_platt_fit": (c_int, [c_void_p, POINTER(SvmPlattProblem), c_int]),
    "bbbp_svm_platt_proba": (c_int, [c_void_p, c_void_p, c_long, c_double, c_double, c_void_p]),
    "bbbp_logreg_state_bytes":(c_size_t, [c_int, c_int]),
    "bbbp_logreg_state_layout": (c_int, [c_int, c_int, POINTER(c_long)]),
    "bbbp_logreg_rounds": (c_int, [c_void_p, POINTER(LogregProblem), c_int, c_int]),
    "bbbp_logreg_eval": (c_int, [c_void_p, POINTER(LogregProblem)]),
    "bbbp_logreg_decision": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_void_p]),
    "bbbp_gbt_fit_tree_capacity": (c_int, [c_int]),
    "bbbp_gbt_fit_work_bytes": (c_size_t, [c_int, c_int]),
    "bbbp_gbt_fit": (c_int, [c_void_p, POINTER(GbtChain), c_void_p, c_int]),
    "bbbp_gbr_fit": (c_int, [c_void_p, POINTER(GbtChain), c_void_p, c_int]),
    "bbbp_gbt_staged_decision": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                         c_double, c_double, c_void_p, c_int, c_void_p]),
    "bbbp_xgb_fit_tree_capacity": (c_int, [c_int, c_int]),
    "bbbp_xgb_fit_work_bytes": (c_size_t, [c_int, c_int]),
    "bbbp_xgb_bin": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "bbbp_xgb_fit": (c_int, [c_void_p, POINTER(XgbProblem), c_void_p, c_int, c_void_p]),
    "bbbp_xgb_fit_profile": (c_int, [c_int]),
    "bbbp_xgb_fit_last": (c_int, [POINTER(c_double), POINTER(c_long)]),
    "bbbp_xgbc_fit_tree_capacity": (c_int, [c_int, c_int]),
    "bbbp_xgbc_fit_work_bytes": (c_size_t, [c_int, c_int]),
    "bbbp_xgbc_fit": (c_int, [c_void_p, POINTER(XgbcProblem), c_void_p, c_int, c_void_p]),
    "bbbp_xgbc_proba": (c_int, [c_void_p, c_void_p, c_long, c_void_p]),
    "bbbp_cat_fit_work_bytes": (c_size_t, [c_int, c_int, c_int]),
    "bbbp_cat_fit": (c_int, [c_void_p, POINTER(CatProblem), c_void_p, c_int]),
    "bbbp_cat_fit_profile": (c_int, [c_int]),
    "bbbp_cat_fit_last": (c_int, [POINTER(c_double), POINTER(c_long)]),
    "bbbp_catc_fit_work_bytes": (c_size_t, [c_int, c_int, c_int]),
    "bbbp_catc_fit": (c_int, [c_void_p, POINTER(CatcProblem), c_void_p, c_int]),
    "bbbp_catc_fit_profile": (c_int, [c_int]),
    "bbbp_catc_fit_last": (c_int, [POINTER(c_double), POINTER(c_long)]),
    "bbbp_catc_proba": (c_int, [c_void_p, c_void_p, c_long, c_void_p]),
    "bbbp_rf_fit_tree_capacity": (c_int, [c_int]),
    "bbbp_rf_fit_work_bytes": (c_size_t, [c_int, c_int, c_int]),
    "bbbp_rf_hash": (c_uint64, [c_uint64, c_uint64]),
    "bbbp_rf_fit": (c_int, [c_void_p, POINTER(RfTree), c_void_p, c_int, c_void_p]),
    "bbbp_rf_predict_proba": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_int, c_int, c_void_p]),
    "bbbp_rf_fit_regression_work_bytes": (c_size_t, [c_int, c_int, c_int]),
    "bbbp_rf_fit_regression": (c_int, [c_void_p, POINTER(RfTree), c_void_p, c_int, c_void_p]),
    "bbbp_rf_predict_mean": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_void_p]),
    "bbbp_iforest_tree_capacity": (c_int, [c_int]),
    "bbbp_iforest_work_bytes": (c_size_t, [c_int]),
    "bbbp_iforest_fit": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p]),
    "bbbp_iforest_path_sum": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "bbbp_bnb_pack": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "bbbp_bnb_count": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bbbp_bnb_jll": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_long, c_int, c_long, c_void_p]),
    "bbbp_smote_synth": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_long]),
    "bbbp_tomek_links": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "bbbp_scaler_moments": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bbbp_scaler_apply": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_long, c_void_p]),
    "bbbp_poly_expand": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_void_p, c_long, c_void_p]),
    "bbbp_metrics_work_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "bbbp_metrics_confusion": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "bbbp_metrics_auc_pairs": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bbbp_metrics_sq_sums": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "bbbp_ens_meta_scatter": (c_int, [c_void_p, POINTER(EnsSource), c_void_p, c_int, POINTER(c_long), c_int, c_int, c_void_p, c_long]),
    "bbbp_ens_soft_vote": (c_int, [c_void_p, POINTER(EnsColumn), c_void_p, c_int, c_void_p, c_double, c_int, c_void_p, c_void_p]),
    "bbbp_ens_hard_vote": (c_int, [c_void_p, POINTER(EnsColumn), c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "bbbp_graph_stats": (c_int, [POINTER(c_long), POINTER(c_long)]),
    "bbbp_conv_last_clock": (c_int, [POINTER(c_uint64), POINTER(c_uint64)]),
    "bbbp_set_conv_winograd": (c_int, [c_int]),
    "bbbp_get_conv_winograd": (c_int, []),
    "bbbp_conv_kernel_form": (c_int, [c_int, c_int, c_int, c_int]),
    "bbbp_conv_winograd_phases": (c_int, [POINTER(c_uint64)]),
    "bbbp_conv_b3_phases": (c_int, [POINTER(c_uint64)]),
    "bbbp_conv3x3_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "bbbp_conv3x3_relu_pool_fwd": (c_int, [c_void_p, _FP, _FP, _FP, _FP, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_size_t]),
    "bbbp_conv3x3_relu_pool_bwd_data": (c_int, [c_void_p, _FP, c_void_p, _FP, _FP, c_int, c_int, c_int, c_int, c_int,
                                                c_void_p, c_size_t]),
    "bbbp_conv3x3_relu_pool_bwd_weight": (c_int, [c_void_p, _FP, _FP, c_void_p, _FP, _FP, c_int, c_int, c_int, c_int,
                                                  c_int, c_void_p, c_size_t]),
    "bbbp_layernorm_fwd": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_float, c_float, c_uint64]),
    "bbbp_layernorm_bwd": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_float, c_uint64]),
    "bbbp_softmax_fwd": (c_int, [c_void_p, _FP, _FP, c_long, c_int, c_float, c_uint64]),
    "bbbp_softmax_bwd": (c_int, [c_void_p, _FP, _FP, c_long, c_int, c_float, c_uint64]),
    "bbbp_dropout": (c_int, [c_void_p, _FP, _FP, c_long, c_float, c_uint64]),
    "bbbp_batchnorm1d_fwd": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_float, c_float, c_int]),
    "bbbp_batchnorm1d_bwd": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int]),
    "bbbp_batchnorm1d_bwd_relu": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int]),
    "bbbp_column_moments": (c_int, [c_void_p, _FP, _FP, _FP, _FP, c_int, c_int]),
    "bbbp_batchnorm1d_bwd_apply": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_long]),
    "bbbp_bias_act_bwd": (c_int, [c_void_p, _FP, c_int, _FP, c_int, _FP, c_int, c_int, c_int, c_float]),
    "bbbp_fusion_combine_fwd": (c_int, [c_void_p, _FP, _FP, _PP, _PP, _FP, _FP, c_int, c_int, c_int, c_int]),
    "bbbp_fusion_combine_bwd": (c_int, [c_void_p, _FP, _FP, _FP, _FP, _PP, _FP, _FP, _FP, c_int, c_int, c_int, c_int]),
    "bbbp_head_fwd": (c_int, [c_void_p, _FP, _PP, _PP, _PP, _PP] + [_FP] * 23 + [c_int] * 5),
    "bbbp_head_bwd": (c_int, [c_void_p] + [_FP] * 10 + [_PP, _PP] + [_FP] * 14 + [c_int] * 4),
    "bbbp_mse": (c_int, [c_void_p, _FP, _FP, _FP, _FP, c_int, c_float]),
    "bbbp_adamw_step": (c_int, [c_void_p, _FP, _FP, _FP, _FP, c_long, c_double, c_double, c_double, c_double, c_double, c_int,
                                c_double]),
    "bbbp_adamw_step_multi": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_double, c_double, c_double, c_double, c_double, c_int, c_double, c_void_p]),
    "bbbp_adamw_hyper_store": (c_int, [c_void_p, c_void_p, c_double, c_double, c_double, c_double, c_double, c_int, c_double]),
    "bbbp_set_seed_base": (c_int, [c_void_p]),
    "bbbp_mlp_profile": (c_int, [c_int, c_void_p]),
    "bbbp_mlp_profile_groups": (c_int, [c_void_p, c_int]),
    "bbbp_set_conv_wgrad_beside_encoder": (c_int, [c_int]),
    "bbbp_set_conv2_fwd_pipe": (c_int, [c_int]),
    "bbbp_adamw_step_deferred": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_long, c_double, c_double, c_double, c_double, c_double, c_int, c_double]),
    "bbbp_param_sync": (c_int, [c_void_p]),
    "bbbp_param_stream": (c_void_p, []),
    "bbbp_scale": (c_int, [c_void_p, _FP, c_long, c_float]),
    "bbbp_resize_bilinear_totensor": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, _FP, c_void_p, c_void_p, c_int, c_void_p,
                                              c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "bbbp_standardize_chunk": (c_int, [c_void_p, c_void_p, _FP, _FP, _FP, c_void_p, c_void_p, c_int, c_int, c_int]),
    "bbbp_set_partition": (c_int, [c_int, c_size_t]),
    "bbbp_set_comm_cus": (c_int, [c_int]),
    "bbbp_set_ln_absorb": (c_int, [c_int]),
    "bbbp_set_overlap": (c_int, [c_int]),
    "bbbp_profile_enable": (c_int, [c_int]),
    "bbbp_profile_select": (c_int, [ctypes.c_uint]),
    "bbbp_profile_num_sections": (c_int, []),
    "bbbp_profile_section_name": (c_char_p, [c_int]),
    "bbbp_profile_collect": (c_int, [POINTER(c_float), POINTER(c_int)]),
    "bbbp_profile_timeline": (c_int, [POINTER(c_int), POINTER(c_float), POINTER(c_float), c_int]),
    "bbbp_mixed_num_params": (c_int, [POINTER(MixedDesc)]),
    "bbbp_mixed_workspace_bytes": (c_size_t, [POINTER(MixedDesc)]),
    "bbbp_mixed_forward": (c_int, [c_void_p, POINTER(MixedDesc), _PP, _PP, _FP, _FP, _FP, c_void_p, c_size_t]),
    "bbbp_mixed_backward": (c_int, [c_void_p, POINTER(MixedDesc), _PP, _PP, _FP, _FP, _FP, c_void_p, c_size_t]),
}


def declared_symbols():
    """Every function name declared in include/bbbp_hip.h (used by the ABI test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bbbp_[a-z0-9_]+)\s*\(", text)))


def lib() -> ctypes.CDLL:
    """Load the HIP library, or fail loudly (there is no CPU fallback on the product path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  The BBBP hot path has no CPU fallback.")
    l = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(l, name)       # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = l
    return l


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().bbbp_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def ptr_array(ptrs):
    arr = (c_void_p * len(ptrs))(*ptrs)
    return arr
