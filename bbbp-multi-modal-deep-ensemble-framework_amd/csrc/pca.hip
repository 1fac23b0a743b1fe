// PCA on the float64 matrix pipe (v_mfma_f64_16x16x4_f64): the column means and the four centred products of decomposition.PCA.
//
//   bbbp_pca_col_mean   float64 column means of a float32 / float64 [n][d] matrix, fixed summation order.
//   bbbp_gemm_f64c      C[M,N] = sum_k (A(m,k) - sa) (B(n,k) - sb), float64 accumulate, operands float32 or float64, both k-contiguous (NT) or
//                       both k-major (TN).  The shift is subtracted per element in float64 when the operand is staged -- never algebraically
//                       (X X^T - n mu mu^T cancels catastrophically for features with large means).
//
// Unlike the MLP trainer (mlp.hip), whose operands are L2-resident, these operands stream from HBM (K up to 49 152, inputs of hundreds of
// MB): the product of a 64 x 64 tile over a slab of K is f64_tile_product (f64_tile.h: the staging pipeline, the LDS image, the clamping
// of ragged M / N / K and the order of summation are described there).
// Order of summation is fixed -- k ascending inside a slab, slabs ascending in the reduce launch -- so a call is bit-reproducible.
// symmetric: only tiles on or below the diagonal run, only elements with row >= col are kept, and each is written to (row, col) and
// (col, row): the result is bitwise symmetric by construction.
#include "f64_tile.h"

namespace {

constexpr int MAX_SPLIT = 256;

// What one launch looks like; the launcher and bbbp_gemm_f64c_workspace_bytes both ask pca_gemm_plan.
struct PcaGemmPlan {
    int tiles_m, tiles_n;
    long ntiles;                // tiles that run (the lower triangle when symmetric)
    int split;                  // K slabs (1: straight to C, no workspace)
    int chunks_per_slab;        // k chunks per slab
    size_t slab_bytes;          // split * M * N doubles when split > 1
};

// Tiles are 64 x 64 whatever the shape and layout (one kernel form, both layouts stage the same LDS image).  The slab count fills the
// chip: about four work-groups per CU (all resident at 36 KB of LDS each), but no slab shorter than 16 chunks (256 k: the reduce pass must stay small beside the product).
// `forced` > 0 overrides (tests).
PcaGemmPlan pca_gemm_plan(int M, int N, int K, int symmetric, int ncu, int forced) {
    PcaGemmPlan pl;
    pl.tiles_m = cdiv(M, F64_TILE);
    pl.tiles_n = cdiv(N, F64_TILE);
    pl.ntiles = symmetric ? (long)pl.tiles_m * (pl.tiles_m + 1) / 2 : (long)pl.tiles_m * pl.tiles_n;
    const int nch = cdiv(K, F64_CHUNK);
    int split = forced;
    if (split <= 0) {
        const long want = 4L * ncu / pl.ntiles;
        split = (int)(want < 1 ? 1 : want);
        if (split > nch / 16) split = nch / 16;
        if (split > 64) split = 64;
        if (split < 1) split = 1;
    }
    pl.split = split;
    pl.chunks_per_slab = cdiv(nch, split);
    pl.slab_bytes = split > 1 ? (size_t)split * M * N * sizeof(double) : 0;
    return pl;
}

struct PcaGemmParams {
    const void* A; const void* B;
    const double* a_shift; const double* b_shift; const double* row_scale;
    void* C; double* slabs;
    long lda, ldb, ldc;
    int M, N, K;
    int symmetric, c_f32;
    int tiles_m, tiles_n, split, chunks_per_slab;
    long ntiles;
};

// One element of C: row scale, float32 or float64 store, mirrored when symmetric.  The fields of PcaGemmParams come by value: through a
// reference to the kernel argument the compiler orders every store behind all outstanding loads.
__device__ __forceinline__ void store_c(const double* row_scale, void* Cv, long ldc, int c_f32, int symmetric, int row, int col, double v) {
    if (row_scale) v *= row_scale[row];
    if (c_f32) {
        float* C = static_cast<float*>(Cv);
        C[(size_t)row * ldc + col] = (float)v;
        if (symmetric && row != col) C[(size_t)col * ldc + row] = (float)v;
    } else {
        double* C = static_cast<double*>(Cv);
        C[(size_t)row * ldc + col] = v;
        if (symmetric && row != col) C[(size_t)col * ldc + row] = v;
    }
}

template <bool TN, bool AF32, bool BF32>
__global__ __launch_bounds__(F64_THREADS) void pca_gemm_kernel(PcaGemmParams p) {
    __shared__ double lds[F64_TILE_LDS];            // the staging buffers of f64_tile_product
    const long bx = blockIdx.x;
    const long tile = bx % p.ntiles;
    const int slab = (int)(bx / p.ntiles);
    int tm, tn;
    if (p.symmetric) {                               // tile -> (tm, tn) with tn <= tm, row by row of the lower triangle
        tm = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
        while ((long)(tm + 1) * (tm + 2) / 2 <= tile) ++tm;
        while ((long)tm * (tm + 1) / 2 > tile) --tm;
        tn = (int)(tile - (long)tm * (tm + 1) / 2);
    } else {
        tm = (int)(tile / p.tiles_n);
        tn = (int)(tile % p.tiles_n);
    }
    const int m0 = tm * F64_TILE, n0 = tn * F64_TILE;
    const int nch = (p.K + F64_CHUNK - 1) / F64_CHUNK;
    int c0 = slab * p.chunks_per_slab, c1 = c0 + p.chunks_per_slab;
    if (c1 > nch) c1 = nch;

    const F64Frag f;
    f64x4 acc[2][2];
    f64_tile_product<TN, AF32, BF32>(lds, f, p.A, p.lda, m0, p.M, p.a_shift, p.B, p.ldb, n0, p.N, p.b_shift, p.K, c0, c1, acc);

    double* slab_out = p.split > 1 ? p.slabs + (size_t)slab * p.M * p.N : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = f.row(i, r, m0), col = f.col(j, n0);
                if (row >= p.M || col >= p.N || (p.symmetric && row < col)) continue;
                if (slab_out) { slab_out[(size_t)row * p.N + col] = acc[i][j][r]; continue; }
                store_c(p.row_scale, p.C, p.ldc, p.c_f32, p.symmetric, row, col, acc[i][j][r]);
            }
}

// slabs summed in slab order, then the same store_c as the single-pass kernel
__global__ __launch_bounds__(256) void pca_reduce_kernel(PcaGemmParams p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)p.M * p.N;
    if (idx >= total) return;
    const int row = (int)(idx / p.N), col = (int)(idx % p.N);
    if (p.symmetric && row < col) return;
    double v = 0.0;
    for (int s = 0; s < p.split; ++s) v += p.slabs[(size_t)s * total + idx];
    store_c(p.row_scale, p.C, p.ldc, p.c_f32, p.symmetric, row, col, v);
}

// Column means: a work-group of 1024 threads owns 64 columns; wave g sums rows g, g + 16, g + 32, ... of them in float64 (a wave reads 64
// consecutive elements of a row), the 16 partial sums of a column are added in wave order.  Non-finite inputs propagate into the sum.
template <bool F32>
__global__ __launch_bounds__(1024) void pca_col_mean_kernel(const void* X, long n, int d, long ld, double* mean) {
    __shared__ double part[16][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (col < d)
        for (long r = g; r < n; r += 16) s += ld_elem<F32>(X, r * ld + col);
    part[g][lane] = s;
    __syncthreads();
    if (g == 0 && col < d) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += part[w][lane];
        mean[col] = t / (double)n;
    }
}

// descriptor checks shared by the launcher and the workspace query (no pointer is dereferenced)
int check_desc(const bbbp_gemm_f64c_desc* d, bool need_pointers) {
    BBBP_CHECK_ARG(d != nullptr, "bbbp_gemm_f64c: null descriptor");
    BBBP_CHECK_ARG(d->layout == BBBP_F64C_NT || d->layout == BBBP_F64C_TN, "bbbp_gemm_f64c: layout %d is neither NT (0) nor TN (1)", d->layout);
    BBBP_CHECK_ARG(d->M > 0 && d->N > 0 && d->K > 0, "bbbp_gemm_f64c: M, N, K must be positive (got %d, %d, %d)", d->M, d->N, d->K);
    BBBP_CHECK_ARG(dtype_ok(d->a_dtype) && dtype_ok(d->b_dtype) && dtype_ok(d->c_dtype),
                   "bbbp_gemm_f64c: unknown dtype (a %d, b %d, c %d): 0 = float32, 1 = float64", d->a_dtype, d->b_dtype, d->c_dtype);
    BBBP_CHECK_ARG(d->split_k >= 0 && d->split_k <= MAX_SPLIT, "bbbp_gemm_f64c: split_k %d outside [0, %d]", d->split_k, MAX_SPLIT);
    if (d->symmetric) {
        BBBP_CHECK_ARG(d->M == d->N, "bbbp_gemm_f64c: symmetric needs M == N (got %d, %d)", d->M, d->N);
        BBBP_CHECK_ARG(d->row_scale == nullptr, "bbbp_gemm_f64c: symmetric excludes row_scale");
        if (need_pointers)
            BBBP_CHECK_ARG(d->A == d->B && d->lda == d->ldb && d->a_dtype == d->b_dtype && d->a_shift == d->b_shift,
                           "bbbp_gemm_f64c: symmetric needs B = A with the same leading dimension, dtype and shift");
    }
    if (need_pointers) {
        BBBP_CHECK_ARG(d->A && d->B && d->C, "bbbp_gemm_f64c: null operand");
        const long mina = d->layout == BBBP_F64C_NT ? d->K : d->M, minb = d->layout == BBBP_F64C_NT ? d->K : d->N;
        BBBP_CHECK_ARG(d->lda >= mina && d->ldb >= minb && d->ldc >= d->N, "bbbp_gemm_f64c: leading dimension too small (lda %ld, ldb %ld, ldc %ld)",
                       d->lda, d->ldb, d->ldc);
    }
    return BBBP_OK;
}

}  // namespace

extern "C" size_t bbbp_gemm_f64c_workspace_bytes(const bbbp_gemm_f64c_desc* d) {
    if (check_desc(d, false) != BBBP_OK) return 0;
    return pca_gemm_plan(d->M, d->N, d->K, d->symmetric, bbbp_num_cus(), d->split_k).slab_bytes;
}

extern "C" int bbbp_gemm_f64c(void* stream, const bbbp_gemm_f64c_desc* d, void* workspace, size_t workspace_bytes) {
    if (int rc = check_desc(d, true)) return rc;
    const PcaGemmPlan pl = pca_gemm_plan(d->M, d->N, d->K, d->symmetric, bbbp_num_cus(), d->split_k);
    if (pl.slab_bytes && (!workspace || workspace_bytes < pl.slab_bytes)) {
        bbbp_set_error("bbbp_gemm_f64c: workspace of %zu bytes, %zu needed", workspace_bytes, pl.slab_bytes);
        return BBBP_ERR_WORKSPACE;
    }
    BBBP_CHECK_ARG(pl.ntiles * pl.split <= 0x7fffffffL, "bbbp_gemm_f64c: %ld tiles x %d slabs exceed the grid", pl.ntiles, pl.split);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PcaGemmParams p;
    p.A = d->A; p.B = d->B; p.a_shift = d->a_shift; p.b_shift = d->b_shift; p.row_scale = d->row_scale;
    p.C = d->C; p.slabs = pl.split > 1 ? static_cast<double*>(workspace) : nullptr;
    p.lda = d->lda; p.ldb = d->ldb; p.ldc = d->ldc;
    p.M = d->M; p.N = d->N; p.K = d->K;
    p.symmetric = d->symmetric ? 1 : 0; p.c_f32 = d->c_dtype == BBBP_DTYPE_F32;
    p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.split = pl.split; p.chunks_per_slab = pl.chunks_per_slab; p.ntiles = pl.ntiles;
    void (*k)(PcaGemmParams) = nullptr;
    with_bools(d->a_dtype == BBBP_DTYPE_F32, d->b_dtype == BBBP_DTYPE_F32, [&](auto A, auto B) {
        k = d->layout == BBBP_F64C_TN ? pca_gemm_kernel<true, A.value, B.value> : pca_gemm_kernel<false, A.value, B.value>;
    });
    hipLaunchKernelGGL(k, dim3((unsigned)(pl.ntiles * pl.split)), dim3(F64_THREADS), 0, st, p);
    BBBP_CHECK_LAUNCH();
    if (pl.split > 1) {
        const size_t total = (size_t)d->M * d->N;
        hipLaunchKernelGGL(pca_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p);
        BBBP_CHECK_LAUNCH();
    }
    return BBBP_OK;
}

extern "C" int bbbp_pca_col_mean(void* stream, const void* X, int dtype, long n, int d, long ld, double* mean) {
    BBBP_CHECK_ARG(X && mean, "bbbp_pca_col_mean: null pointer");
    BBBP_CHECK_ARG(dtype_ok(dtype), "bbbp_pca_col_mean: unknown dtype %d: 0 = float32, 1 = float64", dtype);
    BBBP_CHECK_ARG(n > 0 && d > 0 && ld >= d, "bbbp_pca_col_mean: need n > 0, d > 0, ld >= d (got %ld, %d, %ld)", n, d, ld);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == BBBP_DTYPE_F32) hipLaunchKernelGGL(pca_col_mean_kernel<true>, dim3(cdiv(d, 64)), dim3(1024), 0, st, X, n, d, ld, mean);
    else hipLaunchKernelGGL(pca_col_mean_kernel<false>, dim3(cdiv(d, 64)), dim3(1024), 0, st, X, n, d, ld, mean);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
