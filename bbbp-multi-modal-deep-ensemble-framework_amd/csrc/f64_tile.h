// The staged float64 tile product on v_mfma_f64_16x16x4_f64, shared by the centred GEMM (pca.hip), the kNN search (knn.hip), the SVC kernel
// matrix (svm.hip) and the weighted Gram matrix of the logistic regression (logreg.hip, which also scales A per k):
//     acc[64 x 64] += sum_k (A(m,k) - sa) (B(n,k) - sb)     over the 16-wide k chunks [c0, c1)
// Operands stream from HBM, float32 or float64, both k-contiguous (NT) or both k-major (TN).  A 64 x 64 work-group tile is run by four
// waves of 32 x 32 (2 x 2 MFMA tiles: 32 accumulator registers).  K goes in chunks of 16 through two LDS buffers: chunk c + 1 travels
// global -> registers while chunk c's MFMAs run; conversion to float64 and the shift happen once, on the way from the registers to LDS,
// not per MFMA use.  The shift is subtracted per element in float64, never algebraically.
// LDS image: [buffer][operand][row][k] float64 with rows of 18 (two pad elements): the 32 lanes of a ds_read_b64 group (16 rows x 2 k)
// then fall on 32 distinct 8-byte bank pairs (slot = 18 row + k mod 32: the even slots for k even, the odd ones for k odd).
// Ragged extents: row and k indices are clamped into the matrix for the load and the staged value is zeroed where k is out of range;
// rows and columns beyond the extent hold clamped copies, which the caller's epilogue never uses.
// Order of summation: k ascending, four k per MFMA, whatever the chunk range's start -- an element's sum over [c0, c1) depends only on
// its two rows and the range, which is what makes the callers' results bit-reproducible and independent of their slab / slice counts.
#pragma once
#include "common.h"
#include "bbbp_hip.h"
#include <type_traits>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int F64_TILE = 64;            // work-group tile (rows and columns)
constexpr int F64_CHUNK = 16;           // k per staged chunk
constexpr int F64_ROW = F64_CHUNK + 2;  // LDS row length in doubles
constexpr int F64_THREADS = 256;
constexpr int F64_PER = F64_TILE * F64_CHUNK / F64_THREADS;      // elements per thread per operand per chunk (4)
constexpr int F64_OPERAND = F64_TILE * F64_ROW;                  // doubles of one operand's chunk in LDS
constexpr int F64_TILE_LDS = 2 * 2 * F64_OPERAND;                // doubles of the two double buffers

inline bool dtype_ok(int t) { return t == BBBP_DTYPE_F32 || t == BBBP_DTYPE_F64; }

// f(A, B) with two runtime flags as std::true_type / std::false_type: pick a kernel instantiation by operand dtypes
template <class F>
void with_bools(bool a, bool b, F&& f) {
    if (a) b ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    else b ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

template <bool F32>
__device__ __forceinline__ double ld_elem(const void* p, long i) {
    if (F32) return (double)static_cast<const float*>(p)[i];
    return static_cast<const double*>(p)[i];
}

// One operand's share of a chunk for this thread: F64_PER raw elements (float64 after conversion) in registers.
//   NT (k-contiguous): thread t holds row t >> 2, k = 4 (t & 3) .. + 3 (16 / 32 contiguous bytes per thread, whole 64 / 128-byte row
//       segments per 4 threads);
//   TN (k-major): thread t holds row t & 63 (a wave reads 64 consecutive elements of one k), k = (t >> 6) + 4 j.
template <bool TN, bool F32>
__device__ __forceinline__ void fetch(const void* base, long ld, int row0, int extent, int k0, int K, double (&v)[F64_PER]) {
    const int t = threadIdx.x;
    if (TN) {
        const int r = row0 + (t & 63), rc = r < extent ? r : extent - 1;
#pragma unroll
        for (int j = 0; j < F64_PER; ++j) {
            const int k = k0 + (t >> 6) + 4 * j, kc = k < K ? k : K - 1;
            v[j] = ld_elem<F32>(base, (long)kc * ld + rc);
        }
    } else {
        const int r = row0 + (t >> 2), rc = r < extent ? r : extent - 1;
#pragma unroll
        for (int j = 0; j < F64_PER; ++j) {
            const int k = k0 + F64_PER * (t & 3) + j, kc = k < K ? k : K - 1;
            v[j] = ld_elem<F32>(base, (long)rc * ld + kc);
        }
    }
}

// registers -> LDS image [row][k], shift subtracted in float64, zero where k >= K.  The shift runs over the operand's rows (TN) or over
// k (NT: row0 and extent are not used).  KSCALE (TN only): the shifted value is multiplied by kscale[k], one factor per k -- the weighted
// Gram matrix X^T diag(w) X of logreg.hip.
template <bool TN, bool KSCALE = false>
__device__ __forceinline__ void stage(double* lds, const double (&v)[F64_PER], const double* shift, int row0, int extent, int k0, int K,
                                      const double* kscale = nullptr) {
    static_assert(TN || !KSCALE, "the per-k scale is staged in the TN form only");
    const int t = threadIdx.x;
    if (TN) {
        const int lr = t & 63, r = row0 + lr, rc = r < extent ? r : extent - 1;
        const double s = shift ? shift[rc] : 0.0;
#pragma unroll
        for (int j = 0; j < F64_PER; ++j) {
            const int lk = (t >> 6) + 4 * j;
            if (KSCALE) {
                const int k = k0 + lk, kc = k < K ? k : K - 1;
                lds[lr * F64_ROW + lk] = (k < K) ? (v[j] - s) * kscale[kc] : 0.0;
            } else {
                lds[lr * F64_ROW + lk] = (k0 + lk < K) ? v[j] - s : 0.0;
            }
        }
    } else {
        const int lr = t >> 2;
#pragma unroll
        for (int j = 0; j < F64_PER; ++j) {
            const int lk = F64_PER * (t & 3) + j, k = k0 + lk, kc = k < K ? k : K - 1;
            const double s = shift ? shift[kc] : 0.0;
            lds[lr * F64_ROW + lk] = (k < K) ? v[j] - s : 0.0;
        }
    }
}

// Where this thread's accumulator elements lie in the 64 x 64 tile.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg;
// acc[i][j][r] is element (row(i, r), col(j)), from the tile's origin when row0 / col0 are given.  The A / B fragment of MFMA tile i / j is LDS row wm / wn + 16 i + q at k + kq.
struct F64Frag {
    int wm, wn, q, kq;
    __device__ __forceinline__ F64Frag() {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        wm = (wave >> 1) * 32; wn = (wave & 1) * 32; q = lane & 15; kq = lane >> 4;
    }
    __device__ __forceinline__ int row(int i, int r, int row0 = 0) const { return row0 + wm + 16 * i + kq + 4 * r; }
    __device__ __forceinline__ int col(int j, int col0 = 0) const { return col0 + wn + 16 * j + q; }
};

// acc = the tile product over chunks [c0, c1) (zero when the range is empty).  All 256 threads call it with their F64Frag; `lds` holds
// F64_TILE_LDS doubles.  It returns behind the barrier that ends the last chunk: nobody reads `lds` any more and the caller may reuse it.
// AKSCALE: operand A is multiplied by a_kscale[k] (K doubles) after its shift; without it a_kscale is not read.
template <bool TN, bool AF32, bool BF32, bool AKSCALE = false>
__device__ __forceinline__ void f64_tile_product(double* lds, const F64Frag& f, const void* A, long lda, int a_row0, int a_extent, const double* a_shift,
                                                 const void* B, long ldb, int b_row0, int b_extent, const double* b_shift, int K, int c0,
                                                 int c1, f64x4 (&acc)[2][2], const double* a_kscale = nullptr) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    if (c0 >= c1) return;
    double ra[F64_PER], rb[F64_PER];
    fetch<TN, AF32>(A, lda, a_row0, a_extent, c0 * F64_CHUNK, K, ra);
    fetch<TN, BF32>(B, ldb, b_row0, b_extent, c0 * F64_CHUNK, K, rb);
    stage<TN, AKSCALE>(lds, ra, a_shift, a_row0, a_extent, c0 * F64_CHUNK, K, a_kscale);
    stage<TN>(lds + F64_OPERAND, rb, b_shift, b_row0, b_extent, c0 * F64_CHUNK, K);
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
        const int cur = (c - c0) & 1;
        const bool more = c + 1 < c1;
        if (more) {                              // chunk c + 1: global -> registers while chunk c's MFMAs run
            fetch<TN, AF32>(A, lda, a_row0, a_extent, (c + 1) * F64_CHUNK, K, ra);
            fetch<TN, BF32>(B, ldb, b_row0, b_extent, (c + 1) * F64_CHUNK, K, rb);
        }
        const double* As = lds + cur * (2 * F64_OPERAND);
        const double* Bs = As + F64_OPERAND;
#pragma unroll
        for (int kk = 0; kk < F64_CHUNK; kk += 4) {
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[(f.wm + 16 * i + f.q) * F64_ROW + kk + f.kq];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[(f.wn + 16 * j + f.q) * F64_ROW + kk + f.kq];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) {                              // the other buffer was last read before the barrier that ended chunk c - 1
            double* nx = lds + (cur ^ 1) * (2 * F64_OPERAND);
            stage<TN, AKSCALE>(nx, ra, a_shift, a_row0, a_extent, (c + 1) * F64_CHUNK, K, a_kscale);
            stage<TN>(nx + F64_OPERAND, rb, b_shift, b_row0, b_extent, (c + 1) * F64_CHUNK, K);
        }
        __syncthreads();
    }
}

}  // namespace
