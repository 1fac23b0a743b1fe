// sklearn.preprocessing.PolynomialFeatures on dense float64 rows: the step between the two PCAs and the IsolationForest of the regression
// feature scripts (Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest_fixed_1.py:129: degree 2, interaction_only, no bias, 60
// components -> 1830 columns).  bbbp_amd/preprocessing.py builds the table of factor indices once per fit, in scikit-learn's column order.
//
//   expand   out[r][p] for the table row (f0, f1, f2), -1 for an absent factor: 1.0 when f0 is absent (the bias column), else x[f0], times
//            x[f1] when present, times x[f2] when present -- (x_k * x_j) * x_i for scikit-learn's column (i, j, k), i <= j <= k, one float64
//            product after another, each rounded once (tests/preprocessing_numpy.py pins the result bit for bit).  A work-group of 256
//            threads takes a tile of POLY_ROWS rows and a run of POLY_CHUNK output columns: it stages the rows' d inputs in LDS, then its
//            threads stride over the output columns -- a table row is fetched once and serves every row of the tile, and consecutive lanes
//            write consecutive columns.  Where the tile's inputs exceed POLY_LDS_DOUBLES the factors are read from global memory instead.
//            Every index is 64-bit.  A degree-1 column that is NaN or infinite sets the flag word (every input is one), by a vector atomic
//            OR.  A factor index outside [-1, d) (a defect of the caller) reads nothing and yields NaN.  Every element of the output is
//            written, nothing else.
#include "common.h"
#include "bbbp_hip.h"

namespace {

constexpr int POLY_THREADS = 256;
constexpr int POLY_ROWS = 8;
constexpr int POLY_CHUNK = 1024;                       // output columns per work-group and pass
constexpr int POLY_LDS_DOUBLES = 4096;                 // 32 KB: d <= 512 is staged
constexpr unsigned POLY_MAX_GRID_X = 1u << 20, POLY_MAX_GRID_Y = 32768u;

struct PolyArgs {
    const double* X; long ldx; int n, d;
    const int* table; int P;
    double* out; long ldo; int* flag;
};

static inline unsigned blocks(long work, long per_block) { return (unsigned)((work + per_block - 1) / per_block); }

template <bool STAGED>
__global__ __launch_bounds__(POLY_THREADS) void poly_expand_kernel(PolyArgs a) {
#pragma clang fp contract(off)
    __shared__ double xs[STAGED ? POLY_LDS_DOUBLES : 1];
    const int d = a.d;
    const size_t ldx = (size_t)a.ldx, ldo = (size_t)a.ldo;
    bool bad = false;
    for (long r0 = (long)blockIdx.x * POLY_ROWS; r0 < a.n; r0 += (long)gridDim.x * POLY_ROWS) {          // uniform over the work-group
        const int rows = (int)(a.n - r0 < POLY_ROWS ? a.n - r0 : POLY_ROWS);
        if (STAGED) {
            __syncthreads();                                                                            // the previous tile's readers are done
            for (int e = threadIdx.x; e < rows * d; e += POLY_THREADS) {
                const int r = e / d, c = e - r * d;
                xs[e] = a.X[(size_t)(r0 + r) * ldx + c];
            }
            __syncthreads();
        }
        for (long p0 = (long)blockIdx.y * POLY_CHUNK; p0 < a.P; p0 += (long)gridDim.y * POLY_CHUNK) {
            const long p_end = p0 + POLY_CHUNK < a.P ? p0 + POLY_CHUNK : a.P;
            for (long p = p0 + threadIdx.x; p < p_end; p += POLY_THREADS) {
                const int f0 = a.table[p * 3], f1 = a.table[p * 3 + 1], f2 = a.table[p * 3 + 2];
                const bool ok = f0 >= -1 && f0 < d && f1 >= -1 && f1 < d && f2 >= -1 && f2 < d && (f0 >= 0 || (f1 < 0 && f2 < 0));
                const bool linear = f0 >= 0 && f1 < 0 && f2 < 0;
#pragma unroll
                for (int r = 0; r < POLY_ROWS; ++r) {
                    if (r >= rows) break;
                    double v;
                    if (!ok) v = __builtin_nan("");
                    else if (f0 < 0) v = 1.0;
                    else {
                        const double* x = STAGED ? xs + r * d : a.X + (size_t)(r0 + r) * ldx;
                        v = x[f0];
                        if (f1 >= 0) v = __dmul_rn(v, x[f1]);
                        if (f2 >= 0) v = __dmul_rn(v, x[f2]);
                        if (linear) bad |= (__double_as_longlong(v) & 0x7ff0000000000000ll) == 0x7ff0000000000000ll;
                    }
                    a.out[(size_t)(r0 + r) * ldo + (size_t)p] = v;
                }
            }
        }
    }
    if (bad && a.flag) atomicOr(a.flag, 1);
}

}  // namespace

extern "C" int bbbp_poly_expand(void* stream, const double* X, long ldx, int n, int d, const int* table, int P, double* out, long ldo, int* flag) {
    BBBP_CHECK_ARG(n >= 0 && d >= 1 && P >= 1, "poly_expand: n %d must not be negative, d %d and P %d must be positive", n, d, P);
    BBBP_CHECK_ARG(ldx >= d && ldo >= P, "poly_expand: leading dimensions %ld and %ld below d %d and P %d", ldx, ldo, d, P);
    BBBP_CHECK_ARG(X && table && out, "poly_expand: null pointer");
    BBBP_CHECK_ARG((((uintptr_t)X | (uintptr_t)out) & 7) == 0, "poly_expand: X or out is not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flag) BBBP_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (n == 0) return BBBP_OK;
    unsigned gx = blocks(n, POLY_ROWS), gy = blocks(P, POLY_CHUNK);
    if (gx > POLY_MAX_GRID_X) gx = POLY_MAX_GRID_X;
    if (gy > POLY_MAX_GRID_Y) gy = POLY_MAX_GRID_Y;
    PolyArgs a{X, ldx, n, d, table, P, out, ldo, flag};
    const dim3 grid(gx, gy), block(POLY_THREADS);
    if ((long)d * POLY_ROWS <= POLY_LDS_DOUBLES) hipLaunchKernelGGL(poly_expand_kernel<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(poly_expand_kernel<false>, grid, block, 0, st, a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
