// Batched scores: evaluate_model of the classification scripts (Models/model_maccs.py, model_opt*.py: accuracy, balanced accuracy,
// precision, recall, F1, MCC, Cohen's kappa and ROC AUC per fitted model) and mean_squared_error / r2_score of the regression scripts.
// Seven of the eight classification scores are functions of the four confusion counts and the AUC with ties is the Mann-Whitney pair
// count, so the device computes integers and the host (bbbp_amd/metrics.py) a dozen float64 expressions.  M columns (models, grid points)
// and G row segments (folds: row i carries the prediction of the fold whose test set holds it) are scored by one call.
//
//   confusion  grid (row tile, column).  A wave takes 64 rows: one ballot of the truth, one of the prediction, one per segment present
//              among the 64 rows, and lanes 0..3 each popcount one of the four mask combinations into the wave's own LDS counters.  The
//              waves' counters are added in a last step; a row tile is 16 384 rows, so the reference's shapes are one tile and one launch.
//   pairs      grid (tile of 256 rows, column).  A lane holds one row; the work-group stages the column 256 rows at a time in LDS (score
//              as float64 and a key: the segment of a negative row, -1 otherwise) and every lane that holds a positive row adds
//              (s_j < s_i) + (s_j <= s_i) over the staged rows whose key is its segment.  Every lane reads the same LDS word: a broadcast.
//              Float comparisons, not bit patterns: -0.0 == 0.0.  Quadratic: n^2 / 256 tile passes per column; at the reference's 7 807
//              rows that is 1.6e7 pairs per column.  No sort, no row limit, exact for any n.
//   sum        partial slabs of the row tiles added per output word (integers: no order to fix, and no zero-filled output to rely on).
//   sq_sums    one work-group per (column, segment) plus one per segment for y_true's own sums: a lane-strided sequential sum, the
//              shuffle tree, then the waves in ascending order.  The file is compiled with -ffp-contract=off: d * d + acc is a product
//              and a sum, as tests/metrics_numpy.py rounds them.
// No atomics, no cooperative launch.
#include "common.h"
#include "bbbp_hip.h"

#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_MAX_G = BBBP_METRICS_MAX_GROUPS;
static_assert(BBBP_METRICS_PAIR_ROWS == MT_THREADS, "a lane of the pair kernel holds one row");
static_assert(BBBP_METRICS_TILE_ROWS % MT_THREADS == 0, "a row tile is whole passes of the work-group");

__device__ __forceinline__ double load_value(const void* p, int dtype, size_t at) {
    if (dtype == BBBP_DTYPE_F32) return (double)static_cast<const float*>(p)[at];
    if (dtype == BBBP_DTYPE_F64) return static_cast<const double*>(p)[at];
    return (double)static_cast<const unsigned char*>(p)[at];
}
// the segment of row i, or -1 for a row that is left out
__device__ __forceinline__ int segment_of(const int* seg, long i, int G) {
    const int s = seg ? seg[i] : 0;
    return (unsigned)s < (unsigned)G ? s : -1;
}

// ---- confusion counts ---------------------------------------------------------------------------------------------------------------------
struct ConfArgs {
    const void* pred; int dtype; long ld; int M, n;
    const double* thr; const unsigned char* y01; const int* seg; int G;
    long long* out; int* flag;
};
__global__ __launch_bounds__(MT_THREADS) void metrics_confusion_kernel(ConfArgs a) {
    __shared__ int cnt[MT_WAVES][MT_MAX_G][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < MT_WAVES * MT_MAX_G * 4; k += MT_THREADS) (&cnt[0][0][0])[k] = 0;
    __syncthreads();
    const int m = blockIdx.y;
    const long r0 = (long)blockIdx.x * BBBP_METRICS_TILE_ROWS;
    const long r1 = r0 + BBBP_METRICS_TILE_ROWS < (long)a.n ? r0 + BBBP_METRICS_TILE_ROWS : (long)a.n;
    const bool bytes = a.dtype == BBBP_METRICS_DTYPE_U8;
    const double thr = bytes ? 0.0 : a.thr[m];
    bool bad = false;
    for (long base = r0 + wave * 64; base < r1; base += MT_THREADS) {                // uniform over the wave
        const long i = base + lane;
        const int s = i < r1 ? segment_of(a.seg, i, a.G) : -1;
        bool t = false, p = false;
        if (s >= 0) {
            t = a.y01[i] != 0;
            const size_t at = (size_t)m * (size_t)a.ld + (size_t)i;
            if (bytes) {
                p = static_cast<const unsigned char*>(a.pred)[at] != 0;
            } else {
                const double v = load_value(a.pred, a.dtype, at);
                if (!isfinite(v)) bad = true;
                p = v > thr;
            }
        }
        const u64 bt = __ballot(t), bp = __ballot(p);
        u64 rest = __ballot(s >= 0);
        while (rest) {                                                               // one pass per segment present among the 64 rows
            const int g = __shfl(s, __builtin_ctzll(rest));
            const u64 mg = __ballot(s == g);
            rest &= ~mg;
            if (lane < 4) cnt[wave][g][lane] += __popcll(mg & ((lane & 2) ? bt : ~bt) & ((lane & 1) ? bp : ~bp));   // tn, fp, fn, tp
        }
    }
    if (bad) *a.flag = 1;
    __syncthreads();
    long long* out = a.out + ((size_t)blockIdx.x * (size_t)a.M + (size_t)m) * (size_t)a.G * 4;
    for (int k = threadIdx.x; k < a.G * 4; k += MT_THREADS) {
        long long s = 0;
        for (int w = 0; w < MT_WAVES; ++w) s += cnt[w][k >> 2][k & 3];
        out[k] = s;
    }
}

// ---- AUC pair counts ------------------------------------------------------------------------------------------------------------------------
struct PairArgs {
    const void* score; int dtype; long ld; int M, n;
    const unsigned char* y01; const int* seg; int G;
    long long* part;
};
__global__ __launch_bounds__(MT_THREADS) void metrics_pair_kernel(PairArgs a) {
    __shared__ double sc[MT_THREADS];
    __shared__ int key[MT_THREADS];
    __shared__ long long red[MT_WAVES][MT_MAX_G][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < MT_WAVES * MT_MAX_G * 4; k += MT_THREADS) (&red[0][0][0])[k] = 0;
    const int m = blockIdx.y;
    const size_t col = (size_t)m * (size_t)a.ld;
    const long i = (long)blockIdx.x * MT_THREADS + threadIdx.x;
    const int s = i < a.n ? segment_of(a.seg, i, a.G) : -1;
    double si = 0.0;
    bool pos = false;
    if (s >= 0) {
        si = load_value(a.score, a.dtype, col + (size_t)i);
        pos = a.y01[i] != 0;
    }
    const int mykey = pos ? s : -2;                                                  // -2: matches no staged key
    u64 acc = 0;
    for (long j0 = 0; j0 < a.n; j0 += MT_THREADS) {
        const long j = j0 + threadIdx.x;
        const int sj = j < a.n ? segment_of(a.seg, j, a.G) : -1;
        const bool neg = sj >= 0 && a.y01[j] == 0;
        __syncthreads();                                                             // the previous tile has been read (and, first, red is zero)
        sc[threadIdx.x] = sj >= 0 ? load_value(a.score, a.dtype, col + (size_t)j) : 0.0;
        key[threadIdx.x] = neg ? sj : -1;
        __syncthreads();
        if (mykey >= 0) {
            unsigned add = 0;
#pragma unroll 8
            for (int jj = 0; jj < MT_THREADS; ++jj) {
                const double v = sc[jj];
                add += key[jj] == mykey ? (unsigned)(v < si) + (unsigned)(v <= si) : 0u;
            }
            acc += add;
        }
    }
    const u64 bpos = __ballot(pos), bbad = __ballot(s >= 0 && !isfinite(si));
    u64 rest = __ballot(s >= 0);
    while (rest) {
        const int g = __shfl(s, __builtin_ctzll(rest));
        const u64 mg = __ballot(s == g);
        rest &= ~mg;
        u64 v = s == g ? acc : 0;
        for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) {
            red[wave][g][0] = (long long)v;
            red[wave][g][1] = __popcll(mg & bpos);
            red[wave][g][2] = __popcll(mg & ~bpos);
            red[wave][g][3] = __popcll(mg & bbad);
        }
    }
    __syncthreads();
    long long* out = a.part + ((size_t)blockIdx.x * (size_t)a.M + (size_t)m) * (size_t)a.G * 4;
    for (int k = threadIdx.x; k < a.G * 4; k += MT_THREADS) {
        long long t = 0;
        for (int w = 0; w < MT_WAVES; ++w) t += red[w][k >> 2][k & 3];
        out[k] = t;
    }
}

// out[k] = sum over the tiles of part[tile][k]
__global__ __launch_bounds__(MT_THREADS) void metrics_sum_kernel(const long long* part, long tiles, long words, long long* out) {
    const long k = (long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (k >= words) return;
    long long s = 0;
    for (long t = 0; t < tiles; ++t) s += part[(size_t)t * (size_t)words + (size_t)k];
    out[k] = s;
}

// ---- squared-error sums -----------------------------------------------------------------------------------------------------------------------
struct SqArgs {
    const void* pred; int dtype; long ld; int M, n;
    const double* y; const int* seg; int G;
    double *sse, *ystat; int* flag;
};
// The work-group's sum of one value per lane, in the fixed order of the header comment; every lane receives it.
__device__ __forceinline__ double block_sum(double v, double* slots) {
    for (int off = 32; off; off >>= 1) v = v + __shfl_down(v, off);
    __syncthreads();                                                                 // slots of an earlier sum have been read
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slots[0];
    for (int w = 1; w < MT_WAVES; ++w) s = s + slots[w];
    return s;
}
__global__ __launch_bounds__(MT_THREADS) void metrics_sq_kernel(SqArgs a) {
#pragma clang fp contract(off)
    __shared__ double slots[MT_WAVES];
    const int g = blockIdx.y, m = blockIdx.x;
    bool bad = false;
    if (m < a.M) {
        const size_t col = (size_t)m * (size_t)a.ld;
        double acc = 0.0;
        for (long i = threadIdx.x; i < a.n; i += MT_THREADS) {
            if (segment_of(a.seg, i, a.G) != g) continue;
            const double p = load_value(a.pred, a.dtype, col + (size_t)i);
            if (!isfinite(p)) bad = true;
            const double d = a.y[i] - p;
            const double q = d * d;
            acc = acc + q;
        }
        const double total = block_sum(acc, slots);
        if (threadIdx.x == 0) a.sse[(size_t)m * (size_t)a.G + (size_t)g] = total;
    } else {                                                                         // y_true's own sums, once per segment
        double acc = 0.0, cnt = 0.0;
        for (long i = threadIdx.x; i < a.n; i += MT_THREADS) {
            if (segment_of(a.seg, i, a.G) != g) continue;
            const double yv = a.y[i];
            if (!isfinite(yv)) bad = true;
            acc = acc + yv;
            cnt = cnt + 1.0;                                                         // exact: counts stay below 2^53
        }
        const double sum = block_sum(acc, slots), count = block_sum(cnt, slots);
        const double mean = count > 0.0 ? sum / count : 0.0;
        acc = 0.0;
        for (long i = threadIdx.x; i < a.n; i += MT_THREADS) {
            if (segment_of(a.seg, i, a.G) != g) continue;
            const double d = a.y[i] - mean;
            const double q = d * d;
            acc = acc + q;
        }
        const double ss = block_sum(acc, slots);
        if (threadIdx.x == 0) {
            double* o = a.ystat + 3 * (size_t)g;
            o[0] = sum;
            o[1] = ss;
            o[2] = count;
        }
    }
    if (bad) *a.flag = 1;
}

inline long conf_tiles(int n) { return ((long)n + BBBP_METRICS_TILE_ROWS - 1) / BBBP_METRICS_TILE_ROWS; }
inline long pair_tiles(int n) { return ((long)n + BBBP_METRICS_PAIR_ROWS - 1) / BBBP_METRICS_PAIR_ROWS; }

int check_common(const char* who, int dtype, bool bytes_ok, long ld, int M, int n, int G, const int* seg) {
    BBBP_CHECK_ARG(n >= 1 && M >= 1, "%s: n >= 1 and n_columns >= 1 must hold, got n %d n_columns %d", who, n, M);
    BBBP_CHECK_ARG(M <= BBBP_METRICS_MAX_COLUMNS, "%s: n_columns %d exceeds BBBP_METRICS_MAX_COLUMNS %d", who, M, BBBP_METRICS_MAX_COLUMNS);
    BBBP_CHECK_ARG(G >= 1 && G <= BBBP_METRICS_MAX_GROUPS, "%s: n_groups %d outside 1..BBBP_METRICS_MAX_GROUPS %d", who, G, BBBP_METRICS_MAX_GROUPS);
    BBBP_CHECK_ARG(seg || G == 1, "%s: %d segments without a segment array", who, G);
    BBBP_CHECK_ARG(dtype == BBBP_DTYPE_F32 || dtype == BBBP_DTYPE_F64 || (bytes_ok && dtype == BBBP_METRICS_DTYPE_U8),
                   "%s: dtype %d is not supported here", who, dtype);
    BBBP_CHECK_ARG(ld >= n || M == 1, "%s: row stride %ld below n %d", who, ld, n);
    return BBBP_OK;
}

int sum_slabs(hipStream_t st, const long long* part, long tiles, long words, long long* out) {
    hipLaunchKernelGGL(metrics_sum_kernel, dim3((unsigned)((words + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS), 0, st, part, tiles, words, out);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

}  // namespace

extern "C" size_t bbbp_metrics_work_bytes(int what, int n_columns, int n, int n_groups) {
    if (n < 1 || n_columns < 1 || n_groups < 1) return 0;
    const long tiles = what == 1 ? pair_tiles(n) : conf_tiles(n);
    if (what != 1 && tiles == 1) return 0;
    return (size_t)tiles * (size_t)n_columns * (size_t)n_groups * 4 * sizeof(long long);
}

extern "C" int bbbp_metrics_confusion(void* stream, const void* pred, int dtype, long ld, int n_columns, int n, const double* thr,
                                      const unsigned char* y01, const int* seg, int n_groups, long long* counts, void* work, int* flag) {
    if (int rc = check_common("metrics_confusion", dtype, true, ld, n_columns, n, n_groups, seg)) return rc;
    BBBP_CHECK_ARG(pred && y01 && counts && flag, "metrics_confusion: null pointer");
    BBBP_CHECK_ARG(thr || dtype == BBBP_METRICS_DTYPE_U8, "metrics_confusion: scores need one threshold per column");
    const long tiles = conf_tiles(n);
    BBBP_CHECK_ARG(tiles == 1 || work, "metrics_confusion: %d rows are %ld row tiles and need the work slabs", n, tiles);
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long* part = tiles == 1 ? counts : static_cast<long long*>(work);
    ConfArgs a{pred, dtype, ld, n_columns, n, thr, y01, seg, n_groups, part, flag};
    hipLaunchKernelGGL(metrics_confusion_kernel, dim3((unsigned)tiles, (unsigned)n_columns), dim3(MT_THREADS), 0, st, a);
    BBBP_CHECK_LAUNCH();
    if (tiles > 1) return sum_slabs(st, part, tiles, (long)n_columns * n_groups * 4, counts);
    return BBBP_OK;
}

extern "C" int bbbp_metrics_auc_pairs(void* stream, const void* score, int dtype, long ld, int n_columns, int n, const unsigned char* y01,
                                      const int* seg, int n_groups, long long* out, void* work) {
    if (int rc = check_common("metrics_auc_pairs", dtype, true, ld, n_columns, n, n_groups, seg)) return rc;
    BBBP_CHECK_ARG(score && y01 && out && work, "metrics_auc_pairs: null pointer");
    const long tiles = pair_tiles(n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PairArgs a{score, dtype, ld, n_columns, n, y01, seg, n_groups, static_cast<long long*>(work)};
    hipLaunchKernelGGL(metrics_pair_kernel, dim3((unsigned)tiles, (unsigned)n_columns), dim3(MT_THREADS), 0, st, a);
    BBBP_CHECK_LAUNCH();
    return sum_slabs(st, a.part, tiles, (long)n_columns * n_groups * 4, out);
}

extern "C" int bbbp_metrics_sq_sums(void* stream, const void* pred, int dtype, long ld, int n_columns, int n, const double* y, const int* seg,
                                    int n_groups, double* sse, double* ystat, int* flag) {
    if (int rc = check_common("metrics_sq_sums", dtype, false, ld, n_columns, n, n_groups, seg)) return rc;
    BBBP_CHECK_ARG(pred && y && sse && ystat && flag, "metrics_sq_sums: null pointer");
    SqArgs a{pred, dtype, ld, n_columns, n, y, seg, n_groups, sse, ystat, flag};
    hipLaunchKernelGGL(metrics_sq_kernel, dim3((unsigned)n_columns + 1, (unsigned)n_groups), dim3(MT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
