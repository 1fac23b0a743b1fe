// sklearn.preprocessing.StandardScaler in float64: the first step of every pipeline of the reference (Models/model_opt_maccs.py:104,
// Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest_fixed_1.py:105).  bbbp_amd/preprocessing.py holds the estimator; the
// arithmetic is scikit-learn 1.7's _incremental_mean_and_var followed by _is_constant_feature, every operation rounded on its own, and a
// numpy restatement (tests/preprocessing_numpy.py) pins both kernels bit for bit.
//
//   moments  one thread per column, 64 threads per work-group.  The order of a column's sums is fixed by the parity with numpy (rows one
//            after another), so the parallelism is d; consecutive lanes read consecutive columns of a row.  Two passes over the column:
//            S = sum x, then with T = S / n the sums of (x - T) and of (x - T) * (x - T).  Each pass loads MOM_BATCH rows before it adds
//            them, so that many loads are in flight ahead of the dependent chain of additions.  The merge with an earlier batch
//            (last_mean, last_var, last_n), the constant-column test and the square root follow in the same thread.  The first pass also
//            tests every element's exponent field: a NaN or an infinity sets the flag word (one vector atomic OR per offending thread).
//   apply    (x - mean) / scale or x * scale + mean over a 2-D grid, 64 x 4 threads, APPLY_ROWS rows per thread so that a column's mean and
//            scale are fetched once for them.  Where both bases are 16-byte aligned and both leading dimensions even, a thread moves two
//            columns per access; otherwise one.  Every element of the output is written, nothing else; the input is read in place.
// No fused multiply-add: the file is compiled with -ffp-contract=off and the operations are written with the *_rn intrinsics.  Division
// and square root of float64 are correctly rounded on gfx950.  No LDS, no flag to spin on.
#include "common.h"
#include "bbbp_hip.h"

namespace {

constexpr int MOM_THREADS = 64;
constexpr int MOM_BATCH = 16;
constexpr int APPLY_TX = 64, APPLY_TY = 4, APPLY_ROWS = 4;
constexpr unsigned APPLY_MAX_GRID_X = 1u << 20, APPLY_MAX_GRID_Y = 32768u;
constexpr double EPS = 2.220446049250313e-16;                                     // 2^-52

struct MomentsArgs {
    const double* X; long ldx; int n, d;
    const double *last_mean, *last_var; long last_n;
    double *mean, *var, *scale; int* flag;
};

static inline unsigned blocks(long work, long per_block) { return (unsigned)((work + per_block - 1) / per_block); }

__device__ __forceinline__ bool not_finite(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000ll) == 0x7ff0000000000000ll;
}

__global__ __launch_bounds__(MOM_THREADS) void scaler_moments_kernel(MomentsArgs a) {
#pragma clang fp contract(off)
    const long c = (long)blockIdx.x * MOM_THREADS + threadIdx.x;
    if (c >= a.d) return;
    const double* x = a.X + c;
    const size_t ld = (size_t)a.ldx;
    const int n = a.n;
    double v[MOM_BATCH];
    // pass 1: S = sum x, rows in order
    double S = 0.0;
    bool bad = false;
    int i = 0;
    for (; i + MOM_BATCH <= n; i += MOM_BATCH) {
#pragma unroll
        for (int r = 0; r < MOM_BATCH; ++r) v[r] = x[(size_t)(i + r) * ld];
#pragma unroll
        for (int r = 0; r < MOM_BATCH; ++r) {
            bad |= not_finite(v[r]);
            S = __dadd_rn(S, v[r]);
        }
    }
    for (; i < n; ++i) {
        const double t = x[(size_t)i * ld];
        bad |= not_finite(t);
        S = __dadd_rn(S, t);
    }
    if (bad) atomicOr(a.flag, 1);
    const double nd = (double)n;
    const double T = __ddiv_rn(S, nd);
    // pass 2: corr = sum (x - T), sq = sum (x - T) * (x - T)
    double corr = 0.0, sq = 0.0;
    i = 0;
    for (; i + MOM_BATCH <= n; i += MOM_BATCH) {
#pragma unroll
        for (int r = 0; r < MOM_BATCH; ++r) v[r] = x[(size_t)(i + r) * ld];
#pragma unroll
        for (int r = 0; r < MOM_BATCH; ++r) {
            const double t = __dsub_rn(v[r], T);
            corr = __dadd_rn(corr, t);
            sq = __dadd_rn(sq, __dmul_rn(t, t));
        }
    }
    for (; i < n; ++i) {
        const double t = __dsub_rn(x[(size_t)i * ld], T);
        corr = __dadd_rn(corr, t);
        sq = __dadd_rn(sq, __dmul_rn(t, t));
    }
    const double u_new = __dsub_rn(sq, __ddiv_rn(__dmul_rn(corr, corr), nd));
    double mean, u, N;
    if (a.last_n == 0) {
        N = nd;
        mean = __ddiv_rn(__dadd_rn(0.0, S), nd);
        u = u_new;
    } else {
        const double ln = (double)a.last_n;
        const double last_sum = __dmul_rn(a.last_mean[c], ln);
        N = (double)(a.last_n + (long)n);
        mean = __ddiv_rn(__dadd_rn(last_sum, S), N);
        const double r = __ddiv_rn(ln, nd);
        const double y = __dsub_rn(__ddiv_rn(last_sum, r), S);
        const double last_u = __dmul_rn(a.last_var ? a.last_var[c] : 0.0, ln);
        u = __dadd_rn(__dadd_rn(last_u, u_new), __dmul_rn(__ddiv_rn(r, N), __dmul_rn(y, y)));
    }
    const double var = __ddiv_rn(u, N);
    const double y = __dmul_rn(__dmul_rn(N, mean), EPS);
    const double bound = __dadd_rn(__dmul_rn(__dmul_rn(N, EPS), var), __dmul_rn(y, y));
    a.mean[c] = mean;
    a.var[c] = var;
    a.scale[c] = var <= bound ? 1.0 : __dsqrt_rn(var);
}

struct ApplyArgs {
    const double* X; long ldx; int n, d;
    const double *mean, *scale; int inverse;
    double* out; long ldo; int* flag;
};

__device__ __forceinline__ double apply_one(double x, double m, double s, bool has_m, bool has_s, bool inverse) {
    if (inverse) {
        if (has_s) x = __dmul_rn(x, s);
        if (has_m) x = __dadd_rn(x, m);
    } else {
        if (has_m) x = __dsub_rn(x, m);
        if (has_s) x = __ddiv_rn(x, s);
    }
    return x;
}

// V columns per thread: 2 needs both bases 16-byte aligned and both leading dimensions even
template <int V>
__global__ __launch_bounds__(APPLY_TX * APPLY_TY) void scaler_apply_kernel(ApplyArgs a) {
#pragma clang fp contract(off)
    const bool has_m = a.mean != nullptr, has_s = a.scale != nullptr, inverse = a.inverse != 0;
    const size_t ldx = (size_t)a.ldx, ldo = (size_t)a.ldo;
    bool bad = false;
    for (long c = ((long)blockIdx.y * APPLY_TX + threadIdx.x) * V; c < a.d; c += (long)gridDim.y * APPLY_TX * V) {
        const bool pair = V == 2 && c + 1 < a.d;                                  // the last column of an odd d goes alone
        const double m0 = has_m ? a.mean[c] : 0.0, s0 = has_s ? a.scale[c] : 1.0;
        const double m1 = has_m && pair ? a.mean[c + 1] : 0.0, s1 = has_s && pair ? a.scale[c + 1] : 1.0;
        for (long r0 = ((long)blockIdx.x * APPLY_TY + threadIdx.y) * APPLY_ROWS; r0 < a.n; r0 += (long)gridDim.x * APPLY_TY * APPLY_ROWS) {
#pragma unroll
            for (int k = 0; k < APPLY_ROWS; ++k) {
                const long r = r0 + k;
                if (r >= a.n) break;
                const double* src = a.X + (size_t)r * ldx + c;
                double* dst = a.out + (size_t)r * ldo + c;
                if (pair) {
                    const double2 x = *reinterpret_cast<const double2*>(src);
                    bad |= not_finite(x.x) | not_finite(x.y);
                    double2 o;
                    o.x = apply_one(x.x, m0, s0, has_m, has_s, inverse);
                    o.y = apply_one(x.y, m1, s1, has_m, has_s, inverse);
                    *reinterpret_cast<double2*>(dst) = o;
                } else {
                    const double x = *src;
                    bad |= not_finite(x);
                    *dst = apply_one(x, m0, s0, has_m, has_s, inverse);
                }
            }
        }
    }
    if (bad && a.flag) atomicOr(a.flag, 1);
}

}  // namespace

extern "C" int bbbp_scaler_moments(void* stream, const double* X, long ldx, int n, int d, const double* last_mean, const double* last_var, long last_n,
                                   double* mean, double* var, double* scale, int* flag) {
    BBBP_CHECK_ARG(n >= 1 && d >= 1, "scaler_moments: n %d and d %d must be positive", n, d);
    BBBP_CHECK_ARG(ldx >= d, "scaler_moments: leading dimension %ld below d %d", ldx, d);
    BBBP_CHECK_ARG(last_n >= 0, "scaler_moments: last_n %ld must not be negative", last_n);
    BBBP_CHECK_ARG(last_n == 0 || last_mean, "scaler_moments: last_n %ld needs last_mean", last_n);
    BBBP_CHECK_ARG(X && mean && var && scale && flag, "scaler_moments: null pointer");
    BBBP_CHECK_ARG(((uintptr_t)X & 7) == 0, "scaler_moments: X is not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    BBBP_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    MomentsArgs a{X, ldx, n, d, last_mean, last_var, last_n, mean, var, scale, flag};
    hipLaunchKernelGGL(scaler_moments_kernel, dim3(blocks(d, MOM_THREADS)), dim3(MOM_THREADS), 0, st, a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_scaler_apply(void* stream, const double* X, long ldx, int n, int d, const double* mean, const double* scale, int inverse,
                                 double* out, long ldo, int* flag) {
    BBBP_CHECK_ARG(n >= 0 && d >= 0, "scaler_apply: negative size (n %d, d %d)", n, d);
    BBBP_CHECK_ARG(ldx >= d && ldo >= d, "scaler_apply: leading dimensions %ld and %ld below d %d", ldx, ldo, d);
    BBBP_CHECK_ARG(inverse == 0 || inverse == 1, "scaler_apply: inverse %d is neither 0 nor 1", inverse);
    BBBP_CHECK_ARG(X && out, "scaler_apply: null pointer");
    BBBP_CHECK_ARG((((uintptr_t)X | (uintptr_t)out) & 7) == 0, "scaler_apply: X or out is not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flag) BBBP_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (n == 0 || d == 0) return BBBP_OK;
    const bool wide = (((uintptr_t)X | (uintptr_t)out) & 15) == 0 && ((ldx | ldo) & 1) == 0 && d >= 2;
    const int v = wide ? 2 : 1;
    unsigned gx = blocks(n, APPLY_TY * APPLY_ROWS), gy = blocks(d, APPLY_TX * v);
    if (gx > APPLY_MAX_GRID_X) gx = APPLY_MAX_GRID_X;
    if (gy > APPLY_MAX_GRID_Y) gy = APPLY_MAX_GRID_Y;
    ApplyArgs a{X, ldx, n, d, mean, scale, inverse, out, ldo, flag};
    const dim3 grid(gx, gy), block(APPLY_TX, APPLY_TY);
    if (wide) hipLaunchKernelGGL(scaler_apply_kernel<2>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(scaler_apply_kernel<1>, grid, block, 0, st, a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
