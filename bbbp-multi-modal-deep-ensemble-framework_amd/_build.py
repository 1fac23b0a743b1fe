"""In-tree build of the HIP library (libbbbp_hip.so) for gfx950 with hipcc.

No torch headers are involved: the library is a plain C-ABI shared object (include/bbbp_hip.h)
that Python binds with ctypes, so the same .so serves any host language.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libbbbp_hip.so")
SOURCES = ["util.hip", "gemm.hip", "conv.hip", "conv_wino.hip", "conv_b3.hip", "conv_b3c1.hip", "rowops.hip", "engine.hip", "encoder.hip", "fold.hip", "attention.hip", "attention_b3.hip", "preprocess.hip", "mlp.hip", "head.hip", "forest.hip", "pca.hip", "knn.hip", "svm.hip", "svm_proba.hip", "svr.hip", "logreg.hip", "gbt.hip", "rf.hip", "iforest.hip", "bnb.hip", "smote.hip", "scaler.hip", "poly.hip", "metrics.hip", "xgb.hip", "xgbc.hip", "cat.hip", "catc.hip", "ensemble.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# per-source flags.  conv_b3c1.hip: the pooling epilogue takes maxima of accumulator registers; in IEEE mode every such operand first gets a
# quieting `v_max_f32 x, x, x` (two extra vector instructions per maximum in a kernel whose vector issue slots are the budget).  Without the
# IEEE bit and with finite-math NaN rules the maxima are single instructions; NaN inputs are outside this path's contract.
# svr.hip: the solver's results are pinned bit for bit to a numpy restatement, whose products and sums round one by one: no fused multiply-add
# may be formed from them.  iforest.hip: the same for a split's threshold, lo + (hi - lo) * u (tests/iforest_numpy.py).  bnb.hip: a joint log-likelihood is a chain of float64 additions
# pinned to tests/bnb_numpy.py; nothing in it is a product today, and the flag keeps a later edit from changing the bits.
# smote.hip: a synthetic row is base + step * (neighbour - base) with the product and the sum rounded one by one, as numpy rounds them
# (tests/smote_numpy.py); fused into one multiply-add the row differs in its last bit.
# svm_proba.hip: the sigmoid's argument A dec + B rounds as a product and a sum, as libsvm and tests/platt_numpy.py round it.
# metrics.hip: a squared-error sum adds d * d to its accumulator as a product and a sum (tests/metrics_numpy.py); fused, the MSE differs in its last bits.
# xgb.hip: a split's gain is (G_L * G_L / (H_L + lambda) + G_R * G_R / (H_R + lambda)) - G * G / (H + lambda) with every operation rounded on its
# own, and a leaf's value is one product, as tests/xgb_numpy.py rounds them; the fit is pinned to it bit for bit.
# xgbc.hip: the same for the classifier's gain and leaf value, and its sigmoid is a chain of float64 products and sums (a reduction, a Horner
# polynomial) that tests/xgbc_numpy.py rounds one by one; fused, a probability differs in its last bit and the trees follow.
# cat.hip: a candidate's score adds alpha * S and (alpha * alpha) * m per side, alpha = S / (m + lambda), and ends in (num * num) / den; a leaf's
# value is learning_rate * (S / (m + lambda)) and an approximation s + bias: every operation rounded on its own, as tests/cat_numpy.py rounds
# them; the fit is pinned to it bit for bit.
# catc.hip: the same for the classifier's score over weighted sums and its Newton leaf value learning_rate * (G / (H + lambda)), and its float64
# sigmoid is xgbc.hip's chain of products and sums, which tests/catc_numpy.py rounds one by one; fused, a probability differs in its last bit
# and the trees follow.
# ensemble.hip: a weighted soft vote is P_0 * w_0, then s + P_j * w_j, with every product and sum rounded on its own, as numpy's np.average rounds
# them (tests/ensemble_numpy.py); fused into one multiply-add the averaged probabilities differ in their last bit.
# scaler.hip: a column's squared sum adds t * t to its accumulator as a product and a sum, and the inverse transform is x * scale + mean with two
# roundings, as scikit-learn rounds them (tests/preprocessing_numpy.py); fused, the variance and the restored values differ in their last bits.
EXTRA_FLAGS = {"conv_b3c1.hip": ["-mno-amdgpu-ieee", "-fno-honor-nans"], "svr.hip": ["-ffp-contract=off"], "iforest.hip": ["-ffp-contract=off"],
               "bnb.hip": ["-ffp-contract=off"], "smote.hip": ["-ffp-contract=off"], "scaler.hip": ["-ffp-contract=off"], "svm_proba.hip": ["-ffp-contract=off"], "metrics.hip": ["-ffp-contract=off"],
               "xgb.hip": ["-ffp-contract=off"], "xgbc.hip": ["-ffp-contract=off"], "cat.hip": ["-ffp-contract=off"], "catc.hip": ["-ffp-contract=off"], "ensemble.hip": ["-ffp-contract=off"]}


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    """Compile every .hip under csrc/ for gfx950 and link libbbbp_hip.so.  Returns its path."""
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs.append(os.path.join(os.path.dirname(HERE), "include", "bbbp_hip.h"))
    hdrs = [h for h in hdrs if os.path.exists(h)]
    jobs = []
    objs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src, os.path.abspath(__file__)] + hdrs):
            jobs.append([HIPCC, *FLAGS, *EXTRA_FLAGS.get(s, []), "-I", os.path.join(os.path.dirname(HERE), "include"), "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print("[build]", " ".join(cmd[-4:]), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return r

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
