// Brute-force k-nearest-neighbour search in float64 (Euclidean), fused: the [m][n] distance matrix is never formed in HBM.
//
//   bbbp_knn_row_norms  sum_k (x_k - mu_k)^2 per row in float64, fixed order; ORs 1 into a device word when a row's sum is not finite.
//   bbbp_knn_f64        the k nearest training rows of every query: search (distance + selection), merge of the slice lists, refine.
//   bbbp_knn_vote       class probabilities and the arg-max class from a prefix of the neighbour lists (uniform or 1 / distance weights).
//
// Search.  One work-group owns 64 queries and walks a contiguous slice of the training rows in tiles of 64.  Per tile the Gram block
// (Q - mu)(T - mu)^T is one f64_tile_product (f64_tile.h: v_mfma_f64_16x16x4_f64, the staging pipeline, the shift subtracted at staging,
// clamped loads for ragged m / n / d).  The shift matters: s = |q|^2 + |t|^2 - 2 q.t cancels against the squared norms, so the expansion
// runs on centred rows, whose norms are of the order of the distances.
// Selection.  Every query keeps its k best (s, index) sorted in LDS ([slot][query]: the 64 lanes of the inserting wave touch 64
// consecutive words).  The total order is "smaller s, then smaller training index".  In the tile epilogue each thread compares its 16
// accumulator elements with the k-th entry of their query (one compare in the common case); survivors go to a 64 x 65 tile that reuses
// the staging buffers, and set a bit in a per-query mask (LDS atomic OR).  Wave 0 then inserts the survivors, one lane per query.
// The k best of a set under a total order do not depend on the order of insertion, and s of a pair depends only on the two rows (every
// pair runs the same k loop and the same epilogue expression): lists are bit-identical for every slice count and from call to call.
// Slices.  ceil(m / 64) work-groups may not fill the chip: the training rows are cut into S slices (knn_plan), every (query tile, slice)
// writes a partial list [S][m][k] to the workspace and a merge launch (one wave per query, lane = slice, k rounds of a wave-wide minimum)
// combines them in the same order.
// Refine.  One wave per query recomputes the squared distance of the k kept rows by direct differences sum_k (q_k - t_k)^2 (lane l sums
// k = l, l + 64, ..., then a fixed butterfly), sorts by (distance, index) and writes sqrt: a duplicate of the query gets exactly 0.0 and
// returned distances carry a relative error, not the expansion's absolute one.
#include "f64_tile.h"
#include <math.h>

namespace {

constexpr int KMAX = 32;         // largest list
constexpr int KSLICES = 64;      // largest slice count: one lane per slice in the merge
constexpr int KTP = F64_TILE + 1;      // row length of the survivor tile
static_assert(F64_TILE * KTP <= F64_TILE_LDS, "the survivor tile must fit in the staging buffers");
constexpr int NO_INDEX = 0x7fffffff;

// What one search looks like; the launcher and bbbp_knn_workspace_bytes both ask knn_plan.
struct KnnPlan {
    int tiles_q;
    int slices;                  // 1: lists go straight to the output, no workspace
    int rows_per_slice;
    size_t partial_bytes;        // slices * m * k (double + int) when slices > 1
};

// About two work-groups per CU (62 KB of LDS each), but no slice shorter than four tiles (256 rows: the merge must stay small beside the
// search).  `forced` > 0 overrides (tests).
KnnPlan knn_plan(int m, int n, int k, int ncu, int forced) {
    KnnPlan pl;
    pl.tiles_q = cdiv(m, F64_TILE);
    int s = forced;
    if (s <= 0) {
        const long want = 2L * ncu / pl.tiles_q;
        s = (int)(want < 1 ? 1 : want);
        if (s > n / (4 * F64_TILE)) s = n / (4 * F64_TILE);
        if (s > KSLICES) s = KSLICES;
        if (s < 1) s = 1;
    }
    pl.slices = s;
    pl.rows_per_slice = cdiv(n, s);
    pl.partial_bytes = s > 1 ? (size_t)s * m * k * (sizeof(double) + sizeof(int)) : 0;
    return pl;
}

struct KnnParams {
    const void* Q; const void* T;
    const double* mu; const double* q_norm; const double* t_norm;
    double* dist; long long* ind;             // [m][k]
    double* part_s; int* part_i;              // [slices][m][k] when slices > 1
    long ldq, ldt;
    int m, n, d, k;
    int exclude_self, tiles_q, slices, rows_per_slice;
};

// (s, i) before (t, j) in the total order
__device__ __forceinline__ bool before(double s, int i, double t, int j) { return s < t || (s == t && i < j); }

template <bool QF32, bool TF32>
__global__ __launch_bounds__(F64_THREADS) void knn_search_kernel(KnnParams p) {
    __shared__ double lds[F64_TILE_LDS];            // the staging buffers; between two tiles: the survivor tile [query][KTP]
    __shared__ double best_s[KMAX * F64_TILE];      // [slot][query], sorted
    __shared__ int best_i[KMAX * F64_TILE];
    __shared__ unsigned survivors[F64_TILE * 2];    // [query][half]: bit c of half h = training row 32 h + c of the tile survived
    const int tq = blockIdx.x % p.tiles_q, slice = blockIdx.x / p.tiles_q;
    const int m0 = tq * F64_TILE;
    const int r0 = slice * p.rows_per_slice;
    const long rend = (long)r0 + p.rows_per_slice;
    const int r1 = rend < p.n ? (int)rend : p.n;      // an empty slice (r0 >= n) runs no tile and writes unfilled lists
    const int nch = max((p.d + F64_CHUNK - 1) / F64_CHUNK, 1);      // d > 0: never the product's empty-range exit
    const int k = p.k;

    for (int i = threadIdx.x; i < KMAX * F64_TILE; i += F64_THREADS) { best_s[i] = INFINITY; best_i[i] = NO_INDEX; }
    if (threadIdx.x < F64_TILE * 2) survivors[threadIdx.x] = 0u;
    __syncthreads();

    const F64Frag f;

    for (int n0 = r0; n0 < r1; n0 += F64_TILE) {
        f64x4 acc[2][2];
        f64_tile_product<false, QF32, TF32>(lds, f, p.Q, p.ldq, m0, p.m, p.mu, p.T, p.ldt, n0, p.n, p.mu, p.d, 0, nch, acc);

        // Tile epilogue.  Nobody reads the staging buffers any more (the barrier that ends the product): survivors go to lds as
        // [query][KTP].
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lrow = f.row(i, r), row = m0 + lrow;
                if (row >= p.m) continue;
                const double qn = p.q_norm[row];
                const double thr_s = best_s[(k - 1) * F64_TILE + lrow];
                const int thr_i = best_i[(k - 1) * F64_TILE + lrow];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int lcol = f.col(j), col = n0 + lcol;
                    if (col >= r1 || (p.exclude_self && col == row)) continue;
                    const double s = (qn + p.t_norm[col]) - 2.0 * acc[i][j][r];
                    if (!before(s, col, thr_s, thr_i)) continue;
                    lds[lrow * KTP + lcol] = s;
                    atomicOr(&survivors[lrow * 2 + (lcol >> 5)], 1u << (lcol & 31));
                }
            }
        __syncthreads();
        if (threadIdx.x < F64_TILE) {                // wave 0: lane = query, insertion from the tail
            const int lrow = threadIdx.x;
            for (int h = 0; h < 2; ++h) {
                unsigned bits = survivors[lrow * 2 + h];
                survivors[lrow * 2 + h] = 0u;
                while (bits) {
                    const int lcol = 32 * h + __ffs(bits) - 1;
                    bits &= bits - 1;
                    const double s = lds[lrow * KTP + lcol];
                    const int col = n0 + lcol;
                    if (!before(s, col, best_s[(k - 1) * F64_TILE + lrow], best_i[(k - 1) * F64_TILE + lrow])) continue;
                    int j = k - 1;
                    while (j > 0 && before(s, col, best_s[(j - 1) * F64_TILE + lrow], best_i[(j - 1) * F64_TILE + lrow])) {
                        best_s[j * F64_TILE + lrow] = best_s[(j - 1) * F64_TILE + lrow];
                        best_i[j * F64_TILE + lrow] = best_i[(j - 1) * F64_TILE + lrow];
                        --j;
                    }
                    best_s[j * F64_TILE + lrow] = s;
                    best_i[j * F64_TILE + lrow] = col;
                }
            }
        }
        __syncthreads();                             // before the next tile stages over the survivor tile
    }

    if (threadIdx.x < F64_TILE && m0 + threadIdx.x < p.m) {
        const int lrow = threadIdx.x;
        const size_t row = (size_t)m0 + lrow;
        if (p.slices > 1) {
            const size_t o = ((size_t)slice * p.m + row) * k;
            for (int j = 0; j < k; ++j) { p.part_s[o + j] = best_s[j * F64_TILE + lrow]; p.part_i[o + j] = best_i[j * F64_TILE + lrow]; }
        } else {
            for (int j = 0; j < k; ++j) { p.dist[row * k + j] = best_s[j * F64_TILE + lrow]; p.ind[row * k + j] = best_i[j * F64_TILE + lrow]; }
        }
    }
}

// One wave per query, lane = slice.  k rounds: every lane offers the head of its list, a butterfly finds the first in the total order
// (all lanes agree: the order is total and training indices are distinct across slices), the lane that held it advances.
__global__ __launch_bounds__(256) void knn_merge_kernel(KnnParams p) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= p.m) return;                          // whole waves leave together
    const int k = p.k;
    const bool live = lane < p.slices;
    const size_t o = live ? ((size_t)lane * p.m + row) * k : 0;
    int pos = 0;
    for (int j = 0; j < k; ++j) {
        const bool has = live && pos < k;
        const double s = has ? p.part_s[o + pos] : INFINITY;
        const int i = has ? p.part_i[o + pos] : NO_INDEX;
        double bs = s;
        int bi = i;
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) {
            const double os = __shfl_xor(bs, w);
            const int oi = __shfl_xor(bi, w);
            if (before(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (has && i == bi && i != NO_INDEX) ++pos;
        if (lane == 0) { p.dist[row * k + j] = bs; p.ind[row * k + j] = bi; }
    }
}

// One wave per query: squared distances of the k kept rows by direct differences, sorted by (distance, index), sqrt.
template <bool QF32, bool TF32>
__global__ __launch_bounds__(256) void knn_refine_kernel(KnnParams p) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= p.m) return;
    const int k = p.k;
    double mine = INFINITY;
    int mine_i = NO_INDEX;
    for (int j = 0; j < k; ++j) {
        const long long t = p.ind[row * k + j];      // the same address in every lane
        double r = NAN;
        if (t >= 0 && t < p.n) {                     // an unfilled slot (fewer than k finite candidates) stays NaN and sorts last
            r = 0.0;
            for (int c = lane; c < p.d; c += 64) {
                const double df = ld_elem<QF32>(p.Q, row * p.ldq + c) - ld_elem<TF32>(p.T, t * p.ldt + c);
                r += df * df;
            }
#pragma unroll
            for (int w = 1; w < 64; w <<= 1) r += __shfl_xor(r, w);
        }
        if (lane == j) { mine = r == r ? r : INFINITY; mine_i = (t >= 0 && t < p.n) ? (int)t : NO_INDEX; }
    }
    int rank = 0;
    for (int j = 0; j < k; ++j) {
        const double os = __shfl(mine, j);
        const int oi = __shfl(mine_i, j);
        if (before(os, oi, mine, mine_i) || (os == mine && oi == mine_i && j < lane)) ++rank;
    }
    if (lane < k) {
        const bool ok = mine_i != NO_INDEX;
        p.dist[row * k + rank] = ok ? sqrt(mine) : NAN;
        p.ind[row * k + rank] = ok ? (long long)mine_i : -1LL;
    }
}

// One wave per row: lane l sums k = l, l + 64, ..., then a fixed butterfly (every lane ends with the same bits).
template <bool F32>
__global__ __launch_bounds__(256) void knn_row_norm_kernel(const void* X, long n, int d, long ld, const double* mu, double* norms, int* flag) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    double r = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double v = ld_elem<F32>(X, row * ld + c) - (mu ? mu[c] : 0.0);
        r += v * v;
    }
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) r += __shfl_xor(r, w);
    if (lane == 0) {
        norms[row] = r;
        if (!(fabs(r) <= 1.79769313486231570815e+308)) atomicOr(flag, 1);
    }
}

// One thread per query.  Class weights are accumulated in neighbour order, class by class (no indexed private array).
__global__ __launch_bounds__(256) void knn_vote_kernel(const double* dist, const long long* ind, long m, int k, int kk, const int* labels,
                                                       long n, int n_classes, int by_distance, double* proba, int* pred) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= m) return;
    const double* ds = dist + row * k;
    const long long* is = ind + row * k;
    bool any_zero = false;
    if (by_distance)
        for (int j = 0; j < kk; ++j) any_zero = any_zero || ds[j] == 0.0;
    double total = 0.0, top = -1.0;
    int arg = 0;
    for (int c = 0; c < n_classes; ++c) {
        double w = 0.0;
        for (int j = 0; j < kk; ++j) {
            if (is[j] < 0 || is[j] >= n || labels[is[j]] != c) continue;      // an unfilled slot votes for nothing
            w += !by_distance ? 1.0 : any_zero ? (ds[j] == 0.0 ? 1.0 : 0.0) : 1.0 / ds[j];
        }
        proba[row * n_classes + c] = w;
        total += w;
        if (w > top) { top = w; arg = c; }
    }
    if (total == 0.0) total = 1.0;
    for (int c = 0; c < n_classes; ++c) proba[row * n_classes + c] /= total;
    pred[row] = arg;
}

// descriptor checks shared by the launcher and the workspace query (no pointer is dereferenced)
int check_desc(const bbbp_knn_desc* d, bool need_pointers) {
    BBBP_CHECK_ARG(d != nullptr, "bbbp_knn_f64: null descriptor");
    BBBP_CHECK_ARG(d->m > 0 && d->n > 0 && d->d > 0, "bbbp_knn_f64: m, n, d must be positive (got %d, %d, %d)", d->m, d->n, d->d);
    BBBP_CHECK_ARG(d->n <= 0x7fffffff - F64_TILE, "bbbp_knn_f64: n %d leaves no room for the last tile's indices", d->n);
    BBBP_CHECK_ARG(d->k >= 1 && d->k <= KMAX, "bbbp_knn_f64: k %d outside [1, %d]", d->k, KMAX);
    const int avail = d->exclude_self ? d->n - 1 : d->n;
    BBBP_CHECK_ARG(d->k <= avail, "bbbp_knn_f64: k %d exceeds the %d training rows a query can be given", d->k, avail);
    BBBP_CHECK_ARG(dtype_ok(d->q_dtype) && dtype_ok(d->t_dtype), "bbbp_knn_f64: unknown dtype (q %d, t %d): 0 = float32, 1 = float64", d->q_dtype,
                   d->t_dtype);
    BBBP_CHECK_ARG(d->slices >= 0 && d->slices <= KSLICES, "bbbp_knn_f64: slices %d outside [0, %d]", d->slices, KSLICES);
    if (d->exclude_self) BBBP_CHECK_ARG(d->m == d->n, "bbbp_knn_f64: exclude_self needs Q = T (m %d, n %d)", d->m, d->n);
    if (need_pointers) {
        BBBP_CHECK_ARG(d->Q && d->T && d->q_norm && d->t_norm && d->dist && d->ind, "bbbp_knn_f64: null pointer");
        BBBP_CHECK_ARG(d->ldq >= d->d && d->ldt >= d->d, "bbbp_knn_f64: leading dimension too small (ldq %ld, ldt %ld, d %d)", d->ldq, d->ldt, d->d);
        if (d->exclude_self)
            BBBP_CHECK_ARG(d->Q == d->T && d->ldq == d->ldt && d->q_dtype == d->t_dtype,
                           "bbbp_knn_f64: exclude_self needs Q = T with the same leading dimension and dtype");
    }
    return BBBP_OK;
}

}  // namespace

extern "C" size_t bbbp_knn_workspace_bytes(const bbbp_knn_desc* d) {
    if (check_desc(d, false) != BBBP_OK) return 0;
    return knn_plan(d->m, d->n, d->k, bbbp_num_cus(), d->slices).partial_bytes;
}

extern "C" int bbbp_knn_f64(void* stream, const bbbp_knn_desc* d, void* workspace, size_t workspace_bytes) {
    if (int rc = check_desc(d, true)) return rc;
    const KnnPlan pl = knn_plan(d->m, d->n, d->k, bbbp_num_cus(), d->slices);
    if (pl.partial_bytes && (!workspace || workspace_bytes < pl.partial_bytes)) {
        bbbp_set_error("bbbp_knn_f64: workspace of %zu bytes, %zu needed", workspace_bytes, pl.partial_bytes);
        return BBBP_ERR_WORKSPACE;
    }
    BBBP_CHECK_ARG((long)pl.tiles_q * pl.slices <= 0x7fffffffL, "bbbp_knn_f64: %d query tiles x %d slices exceed the grid", pl.tiles_q, pl.slices);
    hipStream_t st = static_cast<hipStream_t>(stream);
    KnnParams p;
    p.Q = d->Q; p.T = d->T; p.mu = d->mu; p.q_norm = d->q_norm; p.t_norm = d->t_norm;
    p.dist = d->dist; p.ind = d->ind;
    p.part_s = pl.slices > 1 ? static_cast<double*>(workspace) : nullptr;
    p.part_i = pl.slices > 1 ? reinterpret_cast<int*>(p.part_s + (size_t)pl.slices * d->m * d->k) : nullptr;
    p.ldq = d->ldq; p.ldt = d->ldt;
    p.m = d->m; p.n = d->n; p.d = d->d; p.k = d->k;
    p.exclude_self = d->exclude_self ? 1 : 0;
    p.tiles_q = pl.tiles_q; p.slices = pl.slices; p.rows_per_slice = pl.rows_per_slice;
    void (*search)(KnnParams) = nullptr;
    void (*refine)(KnnParams) = nullptr;
    with_bools(d->q_dtype == BBBP_DTYPE_F32, d->t_dtype == BBBP_DTYPE_F32, [&](auto Q, auto T) {
        search = knn_search_kernel<Q.value, T.value>;
        refine = knn_refine_kernel<Q.value, T.value>;
    });
    const unsigned per_wave = (unsigned)(((long)d->m + 3) / 4);
    hipLaunchKernelGGL(search, dim3((unsigned)(pl.tiles_q * pl.slices)), dim3(F64_THREADS), 0, st, p);
    BBBP_CHECK_LAUNCH();
    if (pl.slices > 1) {
        hipLaunchKernelGGL(knn_merge_kernel, dim3(per_wave), dim3(256), 0, st, p);
        BBBP_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(refine, dim3(per_wave), dim3(256), 0, st, p);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_knn_row_norms(void* stream, const void* X, int dtype, long n, int d, long ld, const double* mu, double* norms, int* nonfinite) {
    BBBP_CHECK_ARG(X && norms && nonfinite, "bbbp_knn_row_norms: null pointer");
    BBBP_CHECK_ARG(dtype_ok(dtype), "bbbp_knn_row_norms: unknown dtype %d: 0 = float32, 1 = float64", dtype);
    BBBP_CHECK_ARG(n > 0 && n <= 0x7fffffffL && d > 0 && ld >= d, "bbbp_knn_row_norms: need 0 < n < 2^31, d > 0, ld >= d (got %ld, %d, %ld)", n, d, ld);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)((n + 3) / 4);
    if (dtype == BBBP_DTYPE_F32) hipLaunchKernelGGL(knn_row_norm_kernel<true>, dim3(grid), dim3(256), 0, st, X, n, d, ld, mu, norms, nonfinite);
    else hipLaunchKernelGGL(knn_row_norm_kernel<false>, dim3(grid), dim3(256), 0, st, X, n, d, ld, mu, norms, nonfinite);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_knn_vote(void* stream, const double* dist, const long long* ind, long m, int k, int kk, const int* labels, long n, int n_classes,
                             int weights, double* proba, int* pred) {
    BBBP_CHECK_ARG(dist && ind && labels && proba && pred, "bbbp_knn_vote: null pointer");
    BBBP_CHECK_ARG(m > 0 && m <= 0x7fffffffL, "bbbp_knn_vote: m %ld outside [1, 2^31)", m);
    BBBP_CHECK_ARG(k >= 1 && k <= KMAX && kk >= 1 && kk <= k, "bbbp_knn_vote: need 1 <= kk <= k <= %d (got kk %d, k %d)", KMAX, kk, k);
    BBBP_CHECK_ARG(n > 0, "bbbp_knn_vote: n %ld must be positive", n);
    BBBP_CHECK_ARG(n_classes >= 1 && n_classes <= 32, "bbbp_knn_vote: n_classes %d outside [1, 32]", n_classes);
    BBBP_CHECK_ARG(weights == BBBP_KNN_UNIFORM || weights == BBBP_KNN_DISTANCE, "bbbp_knn_vote: weights %d is neither uniform (0) nor distance (1)",
                   weights);
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dist, ind, m, k, kk, labels,
                       n, n_classes, weights == BBBP_KNN_DISTANCE, proba, pred);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
