// Resampling of an imbalanced class table: SMOTE(random_state=42).fit_resample(X_reduced, y) of the classification stack
// (Models/model_opt_maccs.py, model_opt.py, model_opt_rdkit.py, ...) and SMOTETomek(random_state=42) of model_opt_20250130.py, the step
// between PCA and the eight learners.  The neighbour lists come from csrc/knn.hip and the random draws from the host's
// numpy.random.RandomState (bbbp_amd/imbalance.py); what is left is arithmetic that a numpy restatement pins bit for bit.
//
//   synth   one wave per synthetic row j: r = idx[j] / k is the base row, b = nn[r][idx[j] % k] its drawn neighbour, and the lanes stride
//           over the d columns of out[j][:] = Xc[r][:] + steps[j] * (Xc[b][:] - Xc[r][:]).  The difference, the product and the sum are
//           three separately rounded operations, as in numpy's `X[rows] + steps[:, None] * diffs`: for float64 rows all three in float64;
//           for float32 rows the difference in float32, then product and sum in float64 on the widened values and one rounding of the
//           sum to float32 (numpy's `.astype(float32)` of the float64 expression).  No fused multiply-add: the file is compiled with
//           -ffp-contract=off and the operations are written with the *_rn intrinsics.  Loads and stores are one element per lane, so
//           any base offset, leading dimension and d are fine; a row is 100 elements in the workload, two passes of a wave.
//           An index outside its array (a defect of the caller) reads nothing and yields a row of NaN.
//   tomek   one lane per row i: i is a member of a Tomek link when its nearest other row j = nn1[i] has another label and nn1[j] == i;
//           keep[i] = 0 when it is a member and its class is flagged for removal, else 1.  Every byte of keep is written.
// No atomics, no LDS, no flag to spin on.
#include "common.h"
#include "bbbp_hip.h"

namespace {

constexpr int SMOTE_THREADS = 256;
constexpr int SMOTE_WAVES = SMOTE_THREADS / 64;

struct SynthArgs {
    const void* X; long ldx; int n_c;
    const long *nn, *idx; const double* steps;
    int k, n_new, d;
    void* out; long ldo;
};

__device__ __forceinline__ double interpolate(double a, double b, double s) {
    return __dadd_rn(a, __dmul_rn(s, __dsub_rn(b, a)));
}
__device__ __forceinline__ float interpolate(float a, float b, double s) {
    const float diff = __fsub_rn(b, a);
    return (float)__dadd_rn((double)a, __dmul_rn(s, (double)diff));               // the conversion rounds to nearest even, once
}

template <typename T>
__global__ __launch_bounds__(SMOTE_THREADS) void smote_synth_kernel(SynthArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * SMOTE_WAVES + wave;                         // uniform over the wave, as is every branch below
    if (j >= a.n_new) return;
    T* out = static_cast<T*>(a.out) + (size_t)j * (size_t)a.ldo;
    const long id = a.idx[j];
    long r = -1, b = -1;
    if (id >= 0 && id < (long)a.n_c * a.k) {
        r = id / a.k;
        b = a.nn[r * a.k + id % a.k];
    }
    if (r < 0 || b < 0 || b >= a.n_c) {                                           // no index leaves its array; the host sees NaN, not a stale value
        for (int c = lane; c < a.d; c += 64) out[c] = (T)__builtin_nan("");
        return;
    }
    const T* xr = static_cast<const T*>(a.X) + (size_t)r * (size_t)a.ldx;
    const T* xb = static_cast<const T*>(a.X) + (size_t)b * (size_t)a.ldx;
    const double s = a.steps[j];
    for (int c = lane; c < a.d; c += 64) out[c] = interpolate(xr[c], xb[c], s);
}

__global__ __launch_bounds__(SMOTE_THREADS) void tomek_links_kernel(const long* nn1, const int* y, const unsigned char* remove, int n_classes, int n,
                                                                    unsigned char* keep) {
    const long i = (long)blockIdx.x * SMOTE_THREADS + threadIdx.x;
    if (i >= n) return;
    const long j = nn1[i];
    const int yi = y[i];
    unsigned char kept = 1;
    if (j >= 0 && j < n && (unsigned)yi < (unsigned)n_classes)                    // an index or a label outside its array is no link
        if (y[j] != yi && nn1[j] == i && remove[yi]) kept = 0;
    keep[i] = kept;
}

}  // namespace

extern "C" int bbbp_smote_synth(void* stream, const void* Xc, int x_dtype, long ldx, int n_c, const long* nn, const long* idx, const double* steps,
                                int k, int n_new, int d, void* out, long ldo) {
    BBBP_CHECK_ARG(n_c >= 0 && n_new >= 0 && d >= 0, "smote_synth: negative size (n_c %d, n_new %d, d %d)", n_c, n_new, d);
    BBBP_CHECK_ARG(k >= 1, "smote_synth: k %d must be positive", k);
    BBBP_CHECK_ARG(x_dtype == BBBP_DTYPE_F32 || x_dtype == BBBP_DTYPE_F64, "smote_synth: x_dtype %d is not a BBBP_DTYPE_*", x_dtype);
    BBBP_CHECK_ARG(ldx >= d && ldo >= d, "smote_synth: leading dimensions %ld and %ld below d %d", ldx, ldo, d);
    BBBP_CHECK_ARG(Xc && nn && idx && steps && out, "smote_synth: null pointer");
    if (n_new == 0 || d == 0) return BBBP_OK;
    BBBP_CHECK_ARG(n_c > k, "smote_synth: a class of %d rows has no %d neighbours per row", n_c, k);
    SynthArgs a{Xc, ldx, n_c, nn, idx, steps, k, n_new, d, out, ldo};
    const dim3 grid((unsigned)cdiv(n_new, SMOTE_WAVES)), block(SMOTE_THREADS);
    if (x_dtype == BBBP_DTYPE_F32) hipLaunchKernelGGL(smote_synth_kernel<float>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(smote_synth_kernel<double>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_tomek_links(void* stream, const long* nn1, const int* y, const unsigned char* remove, int n_classes, int n, unsigned char* keep) {
    BBBP_CHECK_ARG(n >= 0 && n_classes >= 1, "tomek_links: n %d must not be negative and n_classes %d must be positive", n, n_classes);
    BBBP_CHECK_ARG(nn1 && y && remove && keep, "tomek_links: null pointer");
    if (n == 0) return BBBP_OK;
    hipLaunchKernelGGL(tomek_links_kernel, dim3((unsigned)cdiv(n, SMOTE_THREADS)), dim3(SMOTE_THREADS), 0, static_cast<hipStream_t>(stream), nn1, y, remove,
                       n_classes, n, keep);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
