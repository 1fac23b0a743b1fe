// PCA on the float64 matrix pipe (v_mfma_f64_16x16x4_f64): the column means and the four centred products of decomposition.PCA.
//
//   bbbp_pca_col_mean   float64 column means of a float32 / float64 [n][d] matrix, fixed summation order.
//   bbbp_gemm_f64c      C[M,N] = sum_k (A(m,k) - sa) (B(n,k) - sb), float64 accumulate, operands float32 or float64, both k-contiguous (NT) or
//                       both k-major (TN).  The shift is subtracted per element in float64 when the operand is staged -- never algebraically
//                       (X X^T - n mu mu^T cancels catastrophically for features with large means).
//
// Unlike the MLP trainer (mlp.hip), whose operands are L2-resident, these operands stream from HBM (K up to 49 152, inputs of hundreds of
// MB): a 64 x 64 work-group tile, four waves of 32 x 32 (2 x 2 MFMA tiles: 32 accumulator registers), K in chunks of 16 through two LDS
// buffers.  Chunk c + 1 travels global -> registers while chunk c's MFMAs run; conversion to float64 and the shift happen once, on the way
// from the registers to LDS, not per MFMA use.  LDS image: [row][k] float64 with rows of 18 (two pad elements): the 32 lanes of a
// ds_read_b64 group (16 rows x 2 k) then fall on 32 distinct 8-byte bank pairs (slot = 18 row + k mod 32: the even slots for k even, the odd ones for k odd).
// Ragged M / N / K: indices are clamped for the load and the staged value is zeroed where k is out of range; rows and columns beyond the
// extent hold clamped copies and are never stored.
// Order of summation is fixed -- k ascending inside a slab, slabs ascending in the reduce launch -- so a call is bit-reproducible.
// symmetric: only tiles on or below the diagonal run, only elements with row >= col are kept, and each is written to (row, col) and
// (col, row): the result is bitwise symmetric by construction.
#include "common.h"
#include "bbbp_hip.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int PT = 64;          // work-group tile (rows and columns)
constexpr int PK = 16;          // k per staged chunk
constexpr int PS = PK + 2;      // LDS row length in doubles
constexpr int PTHREADS = 256;
constexpr int PER = PT * PK / PTHREADS;      // elements per thread per operand per chunk (4)
constexpr int MAX_SPLIT = 256;

// What one launch looks like; the launcher and bbbp_gemm_f64c_workspace_bytes both ask pca_gemm_plan.
struct PcaGemmPlan {
    int tiles_m, tiles_n;
    long ntiles;                // tiles that run (the lower triangle when symmetric)
    int split;                  // K slabs (1: straight to C, no workspace)
    int chunks_per_slab;        // PK-chunks per slab
    size_t slab_bytes;          // split * M * N doubles when split > 1
};

// Tiles are 64 x 64 whatever the shape and layout (one kernel form, both layouts stage the same LDS image).  The slab count fills the
// chip: about four work-groups per CU (all resident at 36 KB of LDS each), but no slab shorter than 16 chunks (256 k: the reduce pass must stay small beside the product).
// `forced` > 0 overrides (tests).
PcaGemmPlan pca_gemm_plan(int M, int N, int K, int symmetric, int ncu, int forced) {
    PcaGemmPlan pl;
    pl.tiles_m = cdiv(M, PT);
    pl.tiles_n = cdiv(N, PT);
    pl.ntiles = symmetric ? (long)pl.tiles_m * (pl.tiles_m + 1) / 2 : (long)pl.tiles_m * pl.tiles_n;
    const int nch = cdiv(K, PK);
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

template <bool F32>
__device__ __forceinline__ double ld_elem(const void* p, long i) {
    if (F32) return (double)static_cast<const float*>(p)[i];
    return static_cast<const double*>(p)[i];
}

// One operand's share of a chunk for this thread: PER raw elements (float64 after conversion) in registers.
//   NT (k-contiguous): thread t holds row t >> 2, k = 4 (t & 3) .. + 3 (16 / 32 contiguous bytes per thread, whole 64 / 128-byte row
//       segments per 4 threads);
//   TN (k-major): thread t holds row t & 63 (a wave reads 64 consecutive elements of one k), k = (t >> 6) + 4 j.
template <bool TN, bool F32>
__device__ __forceinline__ void fetch(const void* base, long ld, int row0, int extent, int k0, int K, double (&v)[PER]) {
    const int t = threadIdx.x;
    if (TN) {
        const int r = row0 + (t & 63), rc = r < extent ? r : extent - 1;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = k0 + (t >> 6) + 4 * j, kc = k < K ? k : K - 1;
            v[j] = ld_elem<F32>(base, (long)kc * ld + rc);
        }
    } else {
        const int r = row0 + (t >> 2), rc = r < extent ? r : extent - 1;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = k0 + PER * (t & 3) + j, kc = k < K ? k : K - 1;
            v[j] = ld_elem<F32>(base, (long)rc * ld + kc);
        }
    }
}

// registers -> LDS image [row][k], shift subtracted in float64, zero where k >= K
template <bool TN>
__device__ __forceinline__ void stage(double* lds, const double (&v)[PER], const double* shift, int row0, int extent, int k0, int K) {
    const int t = threadIdx.x;
    if (TN) {
        const int lr = t & 63, r = row0 + lr, rc = r < extent ? r : extent - 1;
        const double s = shift ? shift[rc] : 0.0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int lk = (t >> 6) + 4 * j;
            lds[lr * PS + lk] = (k0 + lk < K) ? v[j] - s : 0.0;
        }
    } else {
        const int lr = t >> 2;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int lk = PER * (t & 3) + j, k = k0 + lk, kc = k < K ? k : K - 1;
            const double s = shift ? shift[kc] : 0.0;
            lds[lr * PS + lk] = (k < K) ? v[j] - s : 0.0;
        }
    }
}

template <bool TN, bool AF32, bool BF32>
__global__ __launch_bounds__(PTHREADS) void pca_gemm_kernel(PcaGemmParams p) {
    __shared__ double lds[2][2][PT * PS];           // [buffer][operand][row][k]
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
    const int m0 = tm * PT, n0 = tn * PT;
    const int nch = (p.K + PK - 1) / PK;
    int c0 = slab * p.chunks_per_slab, c1 = c0 + p.chunks_per_slab;
    if (c1 > nch) c1 = nch;

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int q = lane & 15, kq = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

    if (c0 < c1) {
        double ra[PER], rb[PER];
        fetch<TN, AF32>(p.A, p.lda, m0, p.M, c0 * PK, p.K, ra);
        fetch<TN, BF32>(p.B, p.ldb, n0, p.N, c0 * PK, p.K, rb);
        stage<TN>(lds[0][0], ra, p.a_shift, m0, p.M, c0 * PK, p.K);
        stage<TN>(lds[0][1], rb, p.b_shift, n0, p.N, c0 * PK, p.K);
        __syncthreads();
        for (int c = c0; c < c1; ++c) {
            const int cur = (c - c0) & 1;
            const bool more = c + 1 < c1;
            if (more) {                              // chunk c + 1: global -> registers while chunk c's MFMAs run
                fetch<TN, AF32>(p.A, p.lda, m0, p.M, (c + 1) * PK, p.K, ra);
                fetch<TN, BF32>(p.B, p.ldb, n0, p.N, (c + 1) * PK, p.K, rb);
            }
            const double* As = lds[cur][0];
            const double* Bs = lds[cur][1];
#pragma unroll
            for (int kk = 0; kk < PK; kk += 4) {
                double a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = As[(wm + 16 * i + q) * PS + kk + kq];
#pragma unroll
                for (int j = 0; j < 2; ++j) b[j] = Bs[(wn + 16 * j + q) * PS + kk + kq];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (more) {                              // the other buffer was last read before the barrier that ended chunk c - 1
                stage<TN>(lds[cur ^ 1][0], ra, p.a_shift, m0, p.M, (c + 1) * PK, p.K);
                stage<TN>(lds[cur ^ 1][1], rb, p.b_shift, n0, p.N, (c + 1) * PK, p.K);
            }
            __syncthreads();
        }
    }

    // epilogue.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
    double* slab_out = p.split > 1 ? p.slabs + (size_t)slab * p.M * p.N : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + 16 * i + kq + 4 * r, col = n0 + wn + 16 * j + q;
                if (row >= p.M || col >= p.N || (p.symmetric && row < col)) continue;
                double v = acc[i][j][r];
                if (slab_out) { slab_out[(size_t)row * p.N + col] = v; continue; }
                if (p.row_scale) v *= p.row_scale[row];
                if (p.c_f32) {
                    float* C = static_cast<float*>(p.C);
                    C[(size_t)row * p.ldc + col] = (float)v;
                    if (p.symmetric && row != col) C[(size_t)col * p.ldc + row] = (float)v;
                } else {
                    double* C = static_cast<double*>(p.C);
                    C[(size_t)row * p.ldc + col] = v;
                    if (p.symmetric && row != col) C[(size_t)col * p.ldc + row] = v;
                }
            }
}

// slabs summed in slab order, then the epilogue of the single-pass kernel
__global__ __launch_bounds__(256) void pca_reduce_kernel(PcaGemmParams p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)p.M * p.N;
    if (idx >= total) return;
    const int row = (int)(idx / p.N), col = (int)(idx % p.N);
    if (p.symmetric && row < col) return;
    double v = 0.0;
    for (int s = 0; s < p.split; ++s) v += p.slabs[(size_t)s * total + idx];
    if (p.row_scale) v *= p.row_scale[row];
    if (p.c_f32) {
        float* C = static_cast<float*>(p.C);
        C[(size_t)row * p.ldc + col] = (float)v;
        if (p.symmetric && row != col) C[(size_t)col * p.ldc + row] = (float)v;
    } else {
        double* C = static_cast<double*>(p.C);
        C[(size_t)row * p.ldc + col] = v;
        if (p.symmetric && row != col) C[(size_t)col * p.ldc + row] = v;
    }
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

bool dtype_ok(int t) { return t == BBBP_DTYPE_F32 || t == BBBP_DTYPE_F64; }

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

typedef void (*PcaKernel)(PcaGemmParams);
template <bool TN>
PcaKernel pick(int af32, int bf32) {
    if (af32) return bf32 ? pca_gemm_kernel<TN, true, true> : pca_gemm_kernel<TN, true, false>;
    return bf32 ? pca_gemm_kernel<TN, false, true> : pca_gemm_kernel<TN, false, false>;
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
    const int af32 = d->a_dtype == BBBP_DTYPE_F32, bf32 = d->b_dtype == BBBP_DTYPE_F32;
    PcaKernel k = d->layout == BBBP_F64C_TN ? pick<true>(af32, bf32) : pick<false>(af32, bf32);
    hipLaunchKernelGGL(k, dim3((unsigned)(pl.ntiles * pl.split)), dim3(PTHREADS), 0, st, p);
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
