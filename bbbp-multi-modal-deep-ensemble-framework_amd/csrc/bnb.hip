// Bernoulli naive Bayes on bits: BernoulliNB() of the classification stack (Models/model_maccs.py:257-267, model_opt_20250130.py:507-510),
// searched over alpha x binarize under five folds and drawn as a learning curve.  A fit is counting -- how many rows of a row subset and a
// class have feature j above a threshold -- and a prediction adds one table entry per set bit, so the binarised matrix is packed into bits
// once and every fold, every learning-curve prefix and every threshold is a popcount pass over the same words.  alpha never reaches the
// device: the log tables are formed on the host from the integer counts (bbbp_amd/naive_bayes.py).
//
//   pack    a work-group stages a tile of 64 rows x 64 features in LDS (coalesced along the features) and ballots it twice per threshold:
//           lane = feature gives the row-major word [t][row][f / 64], lane = row the feature-major word [t][feature][row / 64].  Lanes
//           past n or d vote 0, so the padding bits of the last word of a row or a plane are written as 0 by the kernel that owns them.
//           A NaN or an infinity raises the flag (every lane that sees one stores the same 1: no atomic).
//   count   one wave per (pair of mask and threshold, class, feature): popcll(plane & mask) over the words, lanes striding by 64, then a
//           shuffle reduction.  Integer arithmetic: the order is free.  The class counts are further items of the same launch (the mask's
//           own popcount).  The grid is sized from the items, not from n: a word vector of the reference's 6 246 rows is 98 words, less
//           than two passes of one wave, so a second wave per item (and the LDS step that would join them) would idle.
//   jll     one lane per (problem, query row): the row's words in ascending order, a table entry added per set bit, lowest bit first,
//           then the constant.  Every float64 addition is rounded once and in that order (the file is compiled with -ffp-contract=off
//           although nothing here is a product), so tests/bnb_numpy.py reproduces a result bit for bit.
// No atomics, no cooperative launch, no flag to spin on.
#include "common.h"
#include "bbbp_hip.h"

#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int BNB_THREADS = 256;
constexpr int BNB_WAVES = BNB_THREADS / 64;
constexpr int BNB_TILE = 64;

inline long words_of(long bits) { return (bits + 63) / 64; }

// ---- pack ---------------------------------------------------------------------------------------------------------------------------
struct PackArgs {
    const void* X; int dtype; long ld; int n, d, T;
    const double* thr; u64* planes; u64* rowwords; int* flag;
};
__global__ __launch_bounds__(BNB_THREADS) void bnb_pack_kernel(PackArgs a) {
    __shared__ double tile[BNB_TILE][BNB_TILE + 1];           // float32 values are held exactly; the pad keeps column reads off one bank
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.x * BNB_TILE;
    const int f0 = (int)blockIdx.y * BNB_TILE;
    const long W = ((long)a.n + 63) / 64;
    const int Wd = (a.d + 63) / 64;
    const bool f_in = f0 + lane < a.d;
    bool bad = false;
    for (int r = wave; r < BNB_TILE; r += BNB_WAVES) {
        const long row = r0 + r;
        double v = 0.0;
        if (row < a.n && f_in) {
            const size_t at = (size_t)row * (size_t)a.ld + (size_t)(f0 + lane);
            v = a.dtype == BBBP_DTYPE_F32 ? (double)static_cast<const float*>(a.X)[at] : static_cast<const double*>(a.X)[at];
            if (!isfinite(v)) { bad = true; v = 0.0; }
        }
        tile[r][lane] = v;
    }
    if (bad) *a.flag = 1;
    __syncthreads();
    for (int t = 0; t < a.T; ++t) {
        // numpy's rule for `X > threshold` with a Python float: the threshold takes the array's dtype first
        const double thr = a.dtype == BBBP_DTYPE_F32 ? (double)(float)a.thr[t] : a.thr[t];
        for (int r = wave; r < BNB_TILE; r += BNB_WAVES) {                       // lane = feature: a word of the row-major layout
            const long row = r0 + r;
            const u64 word = __ballot(row < a.n && f_in && tile[r][lane] > thr);
            if (a.rowwords && lane == 0 && row < a.n) a.rowwords[((size_t)t * (size_t)a.n + (size_t)row) * (size_t)Wd + blockIdx.y] = word;
        }
        for (int f = wave; f < BNB_TILE; f += BNB_WAVES) {                       // lane = row: a word of the feature-major layout
            const u64 word = __ballot(r0 + lane < a.n && f0 + f < a.d && tile[lane][f] > thr);
            if (a.planes && lane == 0 && f0 + f < a.d) a.planes[((size_t)t * (size_t)a.d + (size_t)(f0 + f)) * (size_t)W + blockIdx.x] = word;
        }
    }
}

// ---- count --------------------------------------------------------------------------------------------------------------------------
struct CountArgs {
    const u64* planes; int n, d, T;
    const u64* masks; int M;
    const int *pair_mask, *pair_thr; int P;
    int *feature_count, *class_count;
};
__global__ __launch_bounds__(BNB_THREADS) void bnb_count_kernel(CountArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long item = (long)blockIdx.x * BNB_WAVES + wave;                       // uniform over the wave, as is every branch below
    const long W = ((long)a.n + 63) / 64;
    const long feature_items = (long)a.P * 2 * a.d, items = feature_items + 2L * a.M;
    if (item >= items) return;
    const u64 *plane = nullptr, *mask;
    int* out;
    if (item < feature_items) {
        const int j = (int)(item % a.d), c = (int)((item / a.d) & 1);
        const long p = item / (2L * a.d);
        const int m = a.pair_mask[p], t = a.pair_thr[p];
        out = a.feature_count + item;
        if ((unsigned)m >= (unsigned)a.M || (unsigned)t >= (unsigned)a.T) {      // a pair that points outside the batch: no read, a count nobody can take for one
            if (lane == 0) *out = -1;
            return;
        }
        plane = a.planes + ((size_t)t * (size_t)a.d + (size_t)j) * (size_t)W;
        mask = a.masks + ((size_t)m * 2 + (size_t)c) * (size_t)W;
    } else {
        const long k = item - feature_items;                                      // (mask, class)
        mask = a.masks + (size_t)k * (size_t)W;
        out = a.class_count + k;
    }
    int acc = 0;
    for (long w = lane; w < W; w += 64) acc += __popcll(plane ? (plane[w] & mask[w]) : mask[w]);
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) *out = acc;
}

// ---- joint log-likelihood -------------------------------------------------------------------------------------------------------------
struct JllArgs {
    const u64* rowwords; int n, d, T;
    const double *w, *c; const long* desc; const int* rows;
    long n_row_entries, n_out; double* out;
};
__global__ __launch_bounds__(BNB_THREADS) void bnb_jll_kernel(JllArgs a) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.y;
    const long* ds = a.desc + 4 * p;
    const long t = ds[0], row_begin = ds[1], m = ds[2], out_begin = ds[3];
    const long i = (long)blockIdx.x * BNB_THREADS + threadIdx.x;
    if (i >= m || out_begin < 0 || out_begin + m > a.n_out) return;              // the second and third cannot happen with a checked batch
    double* out = a.out + 2 * (out_begin + i);
    long r = i;
    bool ok = t >= 0 && t < a.T;
    if (row_begin >= 0) {
        ok = ok && row_begin + m <= a.n_row_entries;
        if (ok) r = a.rows[row_begin + i];
    }
    if (!ok || r < 0 || r >= a.n) {                                              // no index leaves its array; the host sees NaN, not a stale value
        out[0] = out[1] = __builtin_nan("");
        return;
    }
    const int Wd = (a.d + 63) / 64;
    const u64* words = a.rowwords + ((size_t)t * (size_t)a.n + (size_t)r) * (size_t)Wd;
    const double *w0 = a.w + (size_t)p * 2 * (size_t)a.d, *w1 = w0 + a.d;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < Wd; ++k) {
        u64 word = words[k];
        while (word) {
            const int j = k * 64 + __builtin_ctzll(word);
            if (j >= a.d) break;                                                 // the padding bits are 0 in words of bbbp_bnb_pack; others are not trusted
            s0 += w0[j];
            s1 += w1[j];
            word &= word - 1;
        }
    }
    out[0] = s0 + a.c[2 * p];
    out[1] = s1 + a.c[2 * p + 1];
}

}  // namespace

extern "C" int bbbp_bnb_pack(void* stream, const void* X, int x_dtype, long ld, int n, int d, const double* thresholds, int n_thresholds,
                             unsigned long long* planes, unsigned long long* rowwords, int* flag) {
    BBBP_CHECK_ARG(n >= 1 && d >= 1, "bnb_pack: n >= 1 and d >= 1 must hold, got n %d d %d", n, d);
    BBBP_CHECK_ARG(d <= BBBP_BNB_MAX_D, "bnb_pack: d %d exceeds BBBP_BNB_MAX_D %d", d, BBBP_BNB_MAX_D);
    BBBP_CHECK_ARG(x_dtype == BBBP_DTYPE_F32 || x_dtype == BBBP_DTYPE_F64, "bnb_pack: x_dtype %d is not a BBBP_DTYPE_*", x_dtype);
    BBBP_CHECK_ARG(ld >= d, "bnb_pack: leading dimension %ld below d %d", ld, d);
    BBBP_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= BBBP_BNB_MAX_THRESHOLDS, "bnb_pack: n_thresholds %d outside 1..BBBP_BNB_MAX_THRESHOLDS %d",
                   n_thresholds, BBBP_BNB_MAX_THRESHOLDS);
    BBBP_CHECK_ARG(X && thresholds && flag && (planes || rowwords), "bnb_pack: null pointer (X, thresholds, flag and one of the two layouts are needed)");
    PackArgs a{X, x_dtype, ld, n, d, n_thresholds, thresholds, planes, rowwords, flag};
    hipLaunchKernelGGL(bnb_pack_kernel, dim3((unsigned)words_of(n), (unsigned)words_of(d)), dim3(BNB_THREADS), 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_bnb_count(void* stream, const unsigned long long* planes, int n, int d, int n_thresholds, const unsigned long long* masks,
                              int n_masks, const int* pair_mask, const int* pair_threshold, int n_pairs, int* feature_count, int* class_count) {
    BBBP_CHECK_ARG(n >= 1 && d >= 1, "bnb_count: n >= 1 and d >= 1 must hold, got n %d d %d", n, d);
    BBBP_CHECK_ARG(d <= BBBP_BNB_MAX_D, "bnb_count: d %d exceeds BBBP_BNB_MAX_D %d", d, BBBP_BNB_MAX_D);
    BBBP_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= BBBP_BNB_MAX_THRESHOLDS, "bnb_count: n_thresholds %d outside 1..BBBP_BNB_MAX_THRESHOLDS %d",
                   n_thresholds, BBBP_BNB_MAX_THRESHOLDS);
    BBBP_CHECK_ARG(n_masks >= 1 && n_pairs >= 1, "bnb_count: n_masks and n_pairs must be positive, got %d and %d", n_masks, n_pairs);
    const long items = (long)n_pairs * 2 * d + 2L * n_masks;
    BBBP_CHECK_ARG(n_masks <= BBBP_BNB_MAX_PROBLEMS && n_pairs <= BBBP_BNB_MAX_PROBLEMS && items <= BBBP_BNB_MAX_ITEMS,
                   "bnb_count: %d masks, %d pairs and %ld counts exceed BBBP_BNB_MAX_PROBLEMS %d or BBBP_BNB_MAX_ITEMS %ld", n_masks, n_pairs, items,
                   BBBP_BNB_MAX_PROBLEMS, (long)BBBP_BNB_MAX_ITEMS);
    BBBP_CHECK_ARG(planes && masks && pair_mask && pair_threshold && feature_count && class_count, "bnb_count: null pointer");
    CountArgs a{planes, n, d, n_thresholds, masks, n_masks, pair_mask, pair_threshold, n_pairs, feature_count, class_count};
    hipLaunchKernelGGL(bnb_count_kernel, dim3((unsigned)((items + BNB_WAVES - 1) / BNB_WAVES)), dim3(BNB_THREADS), 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_bnb_jll(void* stream, const unsigned long long* rowwords, int n, int d, int n_thresholds, const double* w, const double* c,
                            const long* problems, int n_problems, const int* rows, long n_row_entries, int max_rows, long n_out, double* out) {
    BBBP_CHECK_ARG(n >= 1 && d >= 1, "bnb_jll: n >= 1 and d >= 1 must hold, got n %d d %d", n, d);
    BBBP_CHECK_ARG(d <= BBBP_BNB_MAX_D, "bnb_jll: d %d exceeds BBBP_BNB_MAX_D %d", d, BBBP_BNB_MAX_D);
    BBBP_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= BBBP_BNB_MAX_THRESHOLDS, "bnb_jll: n_thresholds %d outside 1..BBBP_BNB_MAX_THRESHOLDS %d",
                   n_thresholds, BBBP_BNB_MAX_THRESHOLDS);
    BBBP_CHECK_ARG(n_problems >= 1 && n_problems <= BBBP_BNB_MAX_PROBLEMS, "bnb_jll: n_problems %d outside 1..BBBP_BNB_MAX_PROBLEMS %d", n_problems,
                   BBBP_BNB_MAX_PROBLEMS);
    BBBP_CHECK_ARG(max_rows >= 1 && n_out >= max_rows, "bnb_jll: max_rows %d must be positive and n_out %ld at least that", max_rows, n_out);
    BBBP_CHECK_ARG(n_row_entries >= 0 && (rows || n_row_entries == 0), "bnb_jll: %ld row entries without a row array", n_row_entries);
    BBBP_CHECK_ARG(rowwords && w && c && problems && out, "bnb_jll: null pointer");
    JllArgs a{rowwords, n, d, n_thresholds, w, c, problems, rows, n_row_entries, n_out, out};
    hipLaunchKernelGGL(bnb_jll_kernel, dim3((unsigned)cdiv(max_rows, BNB_THREADS), (unsigned)n_problems), dim3(BNB_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
