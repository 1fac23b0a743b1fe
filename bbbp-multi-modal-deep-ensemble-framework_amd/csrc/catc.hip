// Boosted oblivious (symmetric) classification trees for Logloss, fitted on the GPU: the CatBoost learner of the classification stack
// (CatBoostClassifier(iterations=500, learning_rate=0.03, depth=10, l2_leaf_reg=5, bagging_temperature=0.5, loss_function="Logloss"),
// Models/model_opt_20250130.py:413-457).  cat.hip's fit with another loss and a weighted structure search; that file's bits are pinned and it
// is not touched, so this one stands on its own, in the same shape (bbbp_amd/cat.py states the algorithm, tests/catc_numpy.py restates it
// in numpy; the fit equals it bit for bit).  What differs from cat.hip:
//   the loss       t in {0, 1}; per row s = the float64 sum of its leaf values in tree order, a = s + bias, p = sigmoid64(a) (IEEE
//                  operations only), g = t - p, h = p (1 - p).  Per tree k = 27 - ilogb(max |g|), q = llrint(ldexp(g, k)) (|q| <= 2^28) and
//                  r = max(1, llrint(ldexp(h, 48))) (r <= 2^46)
//   the weights    tree t gives row i the Bayesian-bootstrap weight w = weights[t * weight_stride + i], fixed point with 16 fraction bits,
//                  1 <= w < 2^22, drawn by the host; without a table every w is 2^16.  A row carries qw = q w
//   the sums       a part carries QW = sum qw, MW = sum w and its row count.  |qw| < 2^28 * 2^22 = 2^50 and n <= 8 192 = 2^13, so
//                  |QW| < 2^63 and MW < 2^35: both are exact 64-bit integers in any order.  S = ldexp((double)QW, -(k + 16)) and
//                  M = ldexp((double)MW, -16) take the places of cat.hip's S and m in a side's terms.  A side is empty iff it holds no
//                  row iff its MW is 0 (w >= 1)
//   the leaves     one Newton step over all rows of the leaf, unweighted: Qg = sum q, R = sum r (R <= 2^59), G = ldexp((double)Qg, -k),
//                  H = ldexp((double)R, -48), value = learning_rate * (G / (H + lambda)); leaf_weights records the row count
// A level is the same three launches (split, choose, partition), a tree ends in update, and the host reads nothing back during a fit.  The
// split kernel's histogram holds (sum qw, sum w), both 64-bit integer LDS atomics (16 KB per work-group); the lane-against-lane form
// carries w beside qw.  Both forms add the same integers.  Every operation is rounded on its own (-ffp-contract=off).  Every index read
// from memory is kept inside its array; a wrong one, or a weight outside 1..2^22-1, sets the problem's error word, which the fit reports
// as tree_depth[t] = -1.  No output is zero-filled by the host, there are no float atomics, and no byte outside a problem's own areas
// is touched.
#include "common.h"
#include "bbbp_hip.h"
#include "tree_fit.h"

#include <math.h>

namespace {

constexpr int CATC_SMALL = 64;                // parts of at most this many rows take the lane-against-lane form
constexpr int CATC_NO_FEATURE = 0x7fffffff;
constexpr int CATC_Q_BITS = 27;               // k = CATC_Q_BITS - ilogb(max |g|): |q| <= 2^28
constexpr int CATC_W_BITS = 16;               // fraction bits of a weight
constexpr unsigned CATC_W_ONE = 1u << CATC_W_BITS, CATC_W_END = 1u << 22;

struct State { int tree, level, n_parts, out, error, k, split_f, split_c; };

__host__ __device__ inline int part_capacity(int n, int depth) { const long by_depth = 1L << depth; return (int)(n < by_depth ? n : by_depth); }
// features per work-group of the split kernel, a multiple of four (one wave takes every fourth): at most 256 feature blocks
__host__ __device__ inline int features_per_block(int d) {
    const int blocks = (d + 3) / 4 < 256 ? (d + 3) / 4 : 256;
    return ((d + blocks - 1) / blocks + 3) / 4 * 4;
}
__host__ __device__ inline int feature_blocks(int d) { const int f = features_per_block(d); return (d + f - 1) / f; }

struct Work {                                 // offsets into a problem's `work`, in bytes; all multiples of 16
    size_t rows0, rows1, q, r, qw, w, g, s, leaf_of, tab_start0, tab_start1, tab_cnt0, tab_cnt1, tab_leaf0, tab_leaf1, tab_qw0, tab_qw1, tab_mw0, tab_mw1,
        tab_num0, tab_num1, tab_den0, tab_den1, ch_start, ch_cnt, ch_leaf, ch_qw, ch_mw, cand_score, cand_fb, state, total;
};
__host__ __device__ inline Work work_layout(int n, int d, int depth) {
    Work w;
    Area a;
    const size_t P = (size_t)part_capacity(n, depth), B = (size_t)feature_blocks(d);
    w.rows0 = a.take((size_t)n * 4); w.rows1 = a.take((size_t)n * 4);
    w.q = a.take((size_t)n * 8); w.r = a.take((size_t)n * 8); w.qw = a.take((size_t)n * 8); w.w = a.take((size_t)n * 4);
    w.g = a.take((size_t)n * 8); w.s = a.take((size_t)n * 8); w.leaf_of = a.take((size_t)n * 4);
    w.tab_start0 = a.take(P * 4); w.tab_start1 = a.take(P * 4);
    w.tab_cnt0 = a.take(P * 4); w.tab_cnt1 = a.take(P * 4);
    w.tab_leaf0 = a.take(P * 4); w.tab_leaf1 = a.take(P * 4);
    w.tab_qw0 = a.take(P * 8); w.tab_qw1 = a.take(P * 8);
    w.tab_mw0 = a.take(P * 8); w.tab_mw1 = a.take(P * 8);
    w.tab_num0 = a.take(P * 8); w.tab_num1 = a.take(P * 8);
    w.tab_den0 = a.take(P * 8); w.tab_den1 = a.take(P * 8);
    w.ch_start = a.take(2 * P * 4); w.ch_cnt = a.take(2 * P * 4); w.ch_leaf = a.take(2 * P * 4); w.ch_qw = a.take(2 * P * 8); w.ch_mw = a.take(2 * P * 8);
    w.cand_score = a.take(B * 8); w.cand_fb = a.take(B * 4);
    w.state = a.take(sizeof(State));
    w.total = a.at;
    return w;
}

struct Tab { int *start, *cnt, *leaf; long long *qw, *mw; double *num, *den; };       // the parts of one level
struct View {                                 // a problem's work area, typed
    int *rows_a, *rows_b; long long *q, *r, *qw; unsigned* w; double *g, *s; int* leaf_of; Tab tab_a, tab_b;
    int *ch_start, *ch_cnt, *ch_leaf; long long *ch_qw, *ch_mw;
    double* cand_score; int* cand_fb; State* st;
};
__device__ inline View view_of(const bbbp_catc_problem& p) {
    const Work w = work_layout(p.n, p.d, p.depth);
    char* b = static_cast<char*>(p.work);
    View v;
    v.rows_a = (int*)(b + w.rows0); v.rows_b = (int*)(b + w.rows1);
    v.q = (long long*)(b + w.q); v.r = (long long*)(b + w.r); v.qw = (long long*)(b + w.qw); v.w = (unsigned*)(b + w.w);
    v.g = (double*)(b + w.g); v.s = (double*)(b + w.s); v.leaf_of = (int*)(b + w.leaf_of);
    v.tab_a = Tab{(int*)(b + w.tab_start0), (int*)(b + w.tab_cnt0), (int*)(b + w.tab_leaf0), (long long*)(b + w.tab_qw0), (long long*)(b + w.tab_mw0),
                  (double*)(b + w.tab_num0), (double*)(b + w.tab_den0)};
    v.tab_b = Tab{(int*)(b + w.tab_start1), (int*)(b + w.tab_cnt1), (int*)(b + w.tab_leaf1), (long long*)(b + w.tab_qw1), (long long*)(b + w.tab_mw1),
                  (double*)(b + w.tab_num1), (double*)(b + w.tab_den1)};
    v.ch_start = (int*)(b + w.ch_start); v.ch_cnt = (int*)(b + w.ch_cnt); v.ch_leaf = (int*)(b + w.ch_leaf);
    v.ch_qw = (long long*)(b + w.ch_qw); v.ch_mw = (long long*)(b + w.ch_mw);
    v.cand_score = (double*)(b + w.cand_score); v.cand_fb = (int*)(b + w.cand_fb);
    v.st = (State*)(b + w.state);
    return v;
}
// The two copies of a level's array lie in one work area: the second is reached by arithmetic, not by a select (which the compiler turns into
// an indexed load from a struct in scratch).  Level L reads rows_of(L) and tab_of(L); partition writes those of L + 1
template <class T> __device__ inline T* pick(T* a, T* b, int level) { return a + (long)(level & 1) * (b - a); }
__device__ inline int* rows_of(const View& v, int level) { return pick(v.rows_a, v.rows_b, level); }
__device__ inline Tab tab_of(const View& v, int level) {
    return Tab{pick(v.tab_a.start, v.tab_b.start, level), pick(v.tab_a.cnt, v.tab_b.cnt, level), pick(v.tab_a.leaf, v.tab_b.leaf, level),
               pick(v.tab_a.qw, v.tab_b.qw, level), pick(v.tab_a.mw, v.tab_b.mw, level), pick(v.tab_a.num, v.tab_b.num, level),
               pick(v.tab_a.den, v.tab_b.den, level)};
}
// nothing to do in a level's three kernels: no tree left, no level left, or the tree ran out of candidates
__device__ inline bool level_idle(const bbbp_catc_problem& p, const State* st) { return st->tree >= p.iterations || st->level >= p.depth || st->out; }

// ---- the loss: Logloss ----------------------------------------------------------------------------------------------------------------
// xgbc.hip's sigmoid32 without its last rounding to float32: exp(-|z|) by fdlibm's reduction a = k ln2 + r and the Taylor polynomial of
// degree 13 in r, IEEE operations only, so numpy gives the same bits.  The clamp at -700 keeps p a normal float64.
__device__ inline double sigmoid64(double z) {
    const double LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33, INV_LN2 = 0x1.71547652b82fep+0;
    const double a = fmax(-fabs(z), -700.0);
    const double k = rint(a * INV_LN2);
    const double r = (a - k * LN2_HI) - k * LN2_LO;
    double P = 1.0 / 6227020800.0;
    P = P * r + 1.0 / 479001600.0;
    P = P * r + 1.0 / 39916800.0;
    P = P * r + 1.0 / 3628800.0;
    P = P * r + 1.0 / 362880.0;
    P = P * r + 1.0 / 40320.0;
    P = P * r + 1.0 / 5040.0;
    P = P * r + 1.0 / 720.0;
    P = P * r + 1.0 / 120.0;
    P = P * r + 1.0 / 24.0;
    P = P * r + 1.0 / 6.0;
    P = P * r + 1.0 / 2.0;
    P = P * r + 1.0;
    P = P * r + 1.0;
    const double e = ldexp(P, (int)k);
    return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}
// what a side that holds a row adds to a candidate's num and den: one rounding per integer, then exact scalings
__device__ inline void part_terms(long long QW, long long MW, int k, double lambda, double& num, double& den) {
    const double S = ldexp((double)QW, -(k + CATC_W_BITS)), M = ldexp((double)MW, -CATC_W_BITS), alpha = S / (M + lambda);
    num = alpha * S;
    den = (alpha * alpha) * M;
}
// one Newton step over a leaf's rows
__device__ inline double leaf_step(long long Qg, long long R, int k, double lambda, double learning_rate) {
    const double G = ldexp((double)Qg, -k), H = ldexp((double)R, -BBBP_CATC_HESS_BITS);
    return learning_rate * (G / (H + lambda));
}

struct Best { double score; int feature, bin; };
__device__ inline Best no_candidate() { return Best{-1.0, CATC_NO_FEATURE, 0}; }
// the tie rule: the larger score, among equal scores the lowest feature, then the lowest cut
__device__ inline bool better(const Best& a, const Best& b) {
    return a.score > b.score || (a.score == b.score && (a.feature < b.feature || (a.feature == b.feature && a.bin < b.bin)));
}
__device__ inline Best wave_best(Best b) {
    for (int off = 32; off >= 1; off >>= 1) {
        const Best o{__shfl_xor(b.score, off), __shfl_xor(b.feature, off), __shfl_xor(b.bin, off)};
        if (better(o, b)) b = o;
    }
    return b;
}
__device__ inline long long readlane64(long long x, int lane) {         // `lane` is uniform over the wave
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned long long)x, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)((unsigned long long)x >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// between two phases of a wave's own LDS histogram: the wave's LDS operations complete in order; this keeps the compiler from moving them
__device__ inline void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- a tree's start: approximations, gradients, hessians, weights, the root (one work-group of 1024 threads per problem; every thread
// calls it).  Behind the last tree it leaves approx = s + bias and nothing else: there is no row of weights for a tree that is not fitted
__device__ inline void start_tree(const bbbp_catc_problem& p, const View& v, int tree) {
    __shared__ double red_g[1024];
    __shared__ long long red_qw[1024], red_mw[1024];
    const int tid = threadIdx.x;
    double gmax = 0.0;
    for (int i = tid; i < p.n; i += 1024) {
        const double a = v.s[i] + p.bias;                       // the order of obl_sum_kernel: the leaf sum, then the bias
        p.approx[i] = a;
        const double pr = sigmoid64(a), g = p.t[i] - pr, h = pr * (1.0 - pr);
        const long long r = llrint(ldexp(h, BBBP_CATC_HESS_BITS));
        v.g[i] = g;
        v.r[i] = r < 1 ? 1 : r;
        gmax = fmax(gmax, fabs(g));
    }
    if (tree >= p.iterations) return;                           // uniform over the work-group
    red_g[tid] = gmax;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) red_g[tid] = fmax(red_g[tid], red_g[tid + w]);
        __syncthreads();
    }
    gmax = red_g[0];
    const int k = gmax == 0.0 ? 0 : CATC_Q_BITS - ilogb(gmax);
    const uint32_t* wrow = p.weights ? p.weights + (long)tree * p.weight_stride : nullptr;
    long long sum_qw = 0, sum_w = 0;
    for (int i = tid; i < p.n; i += 1024) {
        const long long q = llrint(ldexp(v.g[i], k));           // the same thread wrote g[i]
        unsigned w = wrow ? wrow[i] : CATC_W_ONE;
        if (w < 1u || w >= CATC_W_END) { v.st->error = 1; w = CATC_W_ONE; }         // the bounds of the integer sums rest on it
        const long long qw = q * (long long)w;                  // exact: |q| <= 2^28, w < 2^22
        v.q[i] = q; v.qw[i] = qw; v.w[i] = w;
        v.rows_a[i] = i;
        v.leaf_of[i] = 0;
        sum_qw += qw; sum_w += (long long)w;
    }
    red_qw[tid] = sum_qw; red_mw[tid] = sum_w;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) { red_qw[tid] += red_qw[tid + w]; red_mw[tid] += red_mw[tid + w]; }        // integers: no order can change a bit
        __syncthreads();
    }
    if (tid == 0) {
        double num, den;
        part_terms(red_qw[0], red_mw[0], k, p.l2_leaf_reg, num, den);
        v.tab_a.start[0] = 0; v.tab_a.cnt[0] = p.n; v.tab_a.leaf[0] = 0; v.tab_a.qw[0] = red_qw[0]; v.tab_a.mw[0] = red_mw[0];
        v.tab_a.num[0] = num; v.tab_a.den[0] = den;
        v.st->level = 0; v.st->n_parts = 1; v.st->out = 0; v.st->k = k; v.st->split_f = -1; v.st->split_c = 0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void catc_init_kernel(const bbbp_catc_problem* problems) {
    const bbbp_catc_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    for (int i = threadIdx.x; i < p.n; i += 1024) v.s[i] = 0.0;                     // the same thread reads it back in start_tree
    if (threadIdx.x == 0) { v.st->tree = 0; v.st->error = 0; }
    start_tree(p, v, 0);
}

// ---- split: the best candidate per (problem, feature block) ---------------------------------------------------------------------------
// One feature, all parts in order: every lane's running (num, den) for its CPL cuts, CPL * lane + t.  `hq` / `hw` are the wave's own.
template <int CPL>
__device__ inline Best walk_feature(const bbbp_catc_problem& p, const View& v, const Tab& tab, const int* src, int n_parts, int k, int f, int n_cuts,
                                    int level, unsigned long long* hq, unsigned long long* hw) {
    const int lane = threadIdx.x & 63, n = p.n;
    const double lambda = p.l2_leaf_reg;
    const uint8_t* col = p.bins + (long)f * n;
    double num[CPL], den[CPL];
    for (int t = 0; t < CPL; ++t) { num[t] = 0.0; den[t] = 0.0; }
    for (int s = 0; s < n_parts; ++s) {
        const int start = tab.start[s];
        int m = tab.cnt[s];
        if (start < 0 || m < 0 || start > n - m) { v.st->error = 1; m = 0; }
        if (m == 0) continue;                                   // cannot happen: the table holds parts with rows
        const long long QW = tab.qw[s], MW = tab.mw[s];
        const double whole_num = tab.num[s], whole_den = tab.den[s];
        long long ql[CPL], wl[CPL];                             // the left side's (sum qw, sum w) of every cut of this lane
        if (m <= CATC_SMALL) {                                  // one row per lane, counted lane against lane
            int b = 256, w_own = 0;
            long long qw_own = 0;
            if (lane < m) { const int row = row_of(src, start + lane, n, v.st); qw_own = v.qw[row]; w_own = (int)v.w[row]; b = col[row]; }
            for (int t = 0; t < CPL; ++t) { ql[t] = 0; wl[t] = 0; }
            for (int r = 0; r < m; ++r) {
                const int b_r = __builtin_amdgcn_readlane(b, r), w_r = __builtin_amdgcn_readlane(w_own, r);     // w < 2^22: one word
                const long long q_r = readlane64(qw_own, r);
                for (int t = 0; t < CPL; ++t)
                    if (b_r <= CPL * lane + t) { ql[t] += q_r; wl[t] += w_r; }
            }
        } else {                                                // the 256-bin histogram of (sum qw, sum w)
            for (int t = 0; t < 4; ++t) { hq[4 * lane + t] = 0ull; hw[4 * lane + t] = 0ull; }
            wave_lds_fence();
            for (int pos = lane; pos < m; pos += 64) {
                const int row = row_of(src, start + pos, n, v.st);
                const int b = col[row];
                atomicAdd(&hq[b], (unsigned long long)v.qw[row]);
                atomicAdd(&hw[b], (unsigned long long)v.w[row]);
            }
            wave_lds_fence();
            long long q_run = 0, w_run = 0;
            for (int t = 0; t < CPL; ++t) {
                q_run += (long long)hq[CPL * lane + t]; w_run += (long long)hw[CPL * lane + t];
                ql[t] = q_run; wl[t] = w_run;
            }
            long long q_incl = q_run, w_incl = w_run;
            for (int off = 1; off < 64; off <<= 1) {
                const long long pq = __shfl_up(q_incl, off), pw = __shfl_up(w_incl, off);
                if (lane >= off) { q_incl += pq; w_incl += pw; }
            }
            for (int t = 0; t < CPL; ++t) { ql[t] += q_incl - q_run; wl[t] += w_incl - w_run; }
            wave_lds_fence();                                   // the next part zeroes the histogram behind these reads
        }
        // a side without a row has the weight sum 0 (w >= 1), the other side then the whole part's
        bool mixed = false;
        for (int t = 0; t < CPL; ++t) mixed = mixed || (wl[t] > 0 && wl[t] < MW);
        if (!__any(mixed)) {                                    // no cut of this wave parts the rows: one side holds the whole part
            for (int t = 0; t < CPL; ++t) { num[t] += whole_num; den[t] += whole_den; }
            continue;
        }
        for (int t = 0; t < CPL; ++t) {
            if (wl[t] <= 0 || wl[t] >= MW) { num[t] += whole_num; den[t] += whole_den; continue; }
            double a, b;
            part_terms(ql[t], wl[t], k, lambda, a, b);          // left, then right
            num[t] += a; den[t] += b;
            part_terms(QW - ql[t], MW - wl[t], k, lambda, a, b);
            num[t] += a; den[t] += b;
        }
    }
    Best best = no_candidate();
    const long base = (long)v.st->tree * p.depth;
    for (int t = 0; t < CPL; ++t) {
        const int c = CPL * lane + t;
        if (c >= n_cuts) continue;
        bool used = false;
        for (int l = 0; l < level; ++l) used = used || (p.split_feature[base + l] == f && p.split_bin[base + l] == c);
        if (used) continue;
        const Best cand{den[t] > 0.0 ? (num[t] * num[t]) / den[t] : 0.0, f, c};
        if (better(cand, best)) best = cand;
    }
    return best;
}

__global__ __launch_bounds__(256) void catc_split_kernel(const bbbp_catc_problem* problems) {
    const bbbp_catc_problem p = problems[blockIdx.y];
    const View v = view_of(p);
    if (level_idle(p, v.st)) return;
    const int fpb = features_per_block(p.d), f0 = blockIdx.x * fpb;
    if (f0 >= p.d) return;                                      // the grid is sized for the widest problem of the batch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int level = v.st->level, k = v.st->k, P = part_capacity(p.n, p.depth);
    int n_parts = v.st->n_parts;
    if (n_parts < 0 || n_parts > P) { v.st->error = 1; n_parts = 0; }
    const Tab tab = tab_of(v, level);
    const int* src = rows_of(v, level);
    __shared__ unsigned long long hist_q[4][256], hist_w[4][256];       // a wave's own histogram: only its lanes touch it
    __shared__ double wb_score[4];
    __shared__ int wb_feature[4], wb_bin[4];
    Best best = no_candidate();
    for (int f = f0 + wave; f < f0 + fpb && f < p.d; f += 4) {
        int nc = p.n_cuts[f];
        if (nc < 1 || nc > 255) { v.st->error = 1; nc = 0; }
        const Best b = nc <= 64 ? walk_feature<1>(p, v, tab, src, n_parts, k, f, nc, level, hist_q[wave], hist_w[wave])
                                : walk_feature<4>(p, v, tab, src, n_parts, k, f, nc, level, hist_q[wave], hist_w[wave]);
        if (better(b, best)) best = b;
    }
    best = wave_best(best);
    if (lane == 0) { wb_score[wave] = best.score; wb_feature[wave] = best.feature; wb_bin[wave] = best.bin; }
    __syncthreads();
    if (tid == 0) {
        Best all = no_candidate();
        for (int w = 0; w < 4; ++w) {
            const Best c{wb_score[w], wb_feature[w], wb_bin[w]};
            if (better(c, all)) all = c;
        }
        v.cand_score[blockIdx.x] = all.score;
        v.cand_fb[blockIdx.x] = all.feature == CATC_NO_FEATURE ? -1 : all.feature * 256 + all.bin;
    }
}

// ---- choose: the best candidate over the feature blocks; the split is recorded, which makes the pair a used one -------------------------
__global__ __launch_bounds__(256) void catc_choose_kernel(const bbbp_catc_problem* problems) {
    const bbbp_catc_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    if (level_idle(p, v.st)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blocks = feature_blocks(p.d);
    __shared__ double wb_score[4];
    __shared__ int wb_feature[4], wb_bin[4];
    Best best = no_candidate();
    for (int b = tid; b < blocks; b += 256) {
        const int fb = v.cand_fb[b];
        if (fb < 0) continue;
        const Best c{v.cand_score[b], fb >> 8, fb & 255};
        if (better(c, best)) best = c;
    }
    best = wave_best(best);
    if (lane == 0) { wb_score[wave] = best.score; wb_feature[wave] = best.feature; wb_bin[wave] = best.bin; }
    __syncthreads();
    if (tid == 0) {
        Best all = no_candidate();
        for (int w = 0; w < 4; ++w) {
            const Best c{wb_score[w], wb_feature[w], wb_bin[w]};
            if (better(c, all)) all = c;
        }
        const int level = v.st->level;
        if (all.feature == CATC_NO_FEATURE) {
            v.st->out = 1;                                      // no unused candidate is left: the tree keeps its `level` levels
        } else if (all.feature < 0 || all.feature >= p.d || all.bin >= p.n_cuts[all.feature] || level < 0 || level >= p.depth) {
            v.st->error = 1; v.st->out = 1;
        } else {
            const long at = (long)v.st->tree * p.depth + level;
            p.split_feature[at] = all.feature; p.split_bin[at] = all.bin;
            v.st->split_f = all.feature; v.st->split_c = all.bin;
        }
    }
}

// ---- partition: every part's rows, stably, by bin <= cut; the next level's parts, those that hold a row --------------------------------
__global__ __launch_bounds__(256) void catc_partition_kernel(const bbbp_catc_problem* problems) {
    const bbbp_catc_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    if (level_idle(p, v.st)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = p.n;
    const int level = v.st->level, k = v.st->k, f = v.st->split_f, c = v.st->split_c, P = part_capacity(n, p.depth);
    int n_parts = v.st->n_parts;
    if (n_parts < 0 || n_parts > P || f < 0 || f >= p.d) { v.st->error = 1; n_parts = 0; }
    const Tab tab = tab_of(v, level), next = tab_of(v, level + 1);
    const int* src = rows_of(v, level);
    int* dst = rows_of(v, level + 1);
    const uint8_t* col = p.bins + (long)(f < 0 || f >= p.d ? 0 : f) * n;
    for (int s = wave; s < n_parts; s += 4) {
        const int start = tab.start[s], leaf = tab.leaf[s];
        int m = tab.cnt[s];
        if (start < 0 || m < 0 || start > n - m) { v.st->error = 1; m = 0; }
        int m_l = 0;
        long long qw_l = 0, mw_l = 0;
        for (int pos = lane; pos < m; pos += 64) {              // the left side's count and integer sums
            const int row = row_of(src, start + pos, n, v.st);
            if (col[row] <= c) { ++m_l; qw_l += v.qw[row]; mw_l += (long long)v.w[row]; }
        }
        for (int off = 32; off >= 1; off >>= 1) { m_l += __shfl_xor(m_l, off); qw_l += __shfl_xor(qw_l, off); mw_l += __shfl_xor(mw_l, off); }
        int lefts = 0;                                          // rows going left in front of this pass
        for (int pos0 = 0; pos0 < m; pos0 += 64) {
            const int pos = pos0 + lane;
            const bool in = pos < m;
            const int row = in ? row_of(src, start + pos, n, v.st) : 0;
            const bool left = in && col[row] <= c;
            const unsigned long long ballot = __ballot(left);
            const int before = lefts + __popcll(ballot & ((1ull << lane) - 1ull));
            if (in) {
                const int to = left ? before : m_l + (pos - before);
                if (to >= 0 && to < m) dst[start + to] = row;
                else v.st->error = 1;
                if (!left) v.leaf_of[row] = leaf | (1 << level);
            }
            lefts += __popcll(ballot);
        }
        if (lefts != m_l) v.st->error = 1;                      // the count and the partition disagree: cannot happen
        if (lane == 0) {
            v.ch_start[2 * s] = start; v.ch_cnt[2 * s] = m_l; v.ch_leaf[2 * s] = leaf; v.ch_qw[2 * s] = qw_l; v.ch_mw[2 * s] = mw_l;
            v.ch_start[2 * s + 1] = start + m_l; v.ch_cnt[2 * s + 1] = m - m_l; v.ch_leaf[2 * s + 1] = leaf | (1 << level);
            v.ch_qw[2 * s + 1] = tab.qw[s] - qw_l; v.ch_mw[2 * s + 1] = tab.mw[s] - mw_l;
        }
    }
    __threadfence_block();
    __syncthreads();
    __shared__ int wave_cnt[2][4];
    int total = 0;
    for (int c0 = 0, it = 0; c0 < 2 * n_parts; c0 += 256, ++it) {
        const int ch = c0 + tid;
        const bool in = ch < 2 * n_parts;
        const int m = in ? v.ch_cnt[ch] : 0;
        const bool keep = in && m > 0;
        const int at = block_rank_before(keep, wave_cnt[it & 1], total);
        if (!keep) continue;
        if (at >= P) { v.st->error = 1; continue; }             // cannot happen: at most n parts hold a row, and at most 2^depth exist
        const long long QW = v.ch_qw[ch], MW = v.ch_mw[ch];
        double num, den;
        part_terms(QW, MW, k, p.l2_leaf_reg, num, den);
        next.start[at] = v.ch_start[ch]; next.cnt[at] = m; next.leaf[at] = v.ch_leaf[ch]; next.qw[at] = QW; next.mw[at] = MW;
        next.num[at] = num; next.den[at] = den;
    }
    __syncthreads();
    if (tid == 0) { v.st->level = level + 1; v.st->n_parts = total > P ? P : total; }
}

// ---- update: a finished tree's leaves (a Newton step each) and the rows' sums, then the next tree's gradients ---------------------------
__global__ __launch_bounds__(1024) void catc_update_kernel(const bbbp_catc_problem* problems) {
    const bbbp_catc_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    if (v.st->tree >= p.iterations) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tree = v.st->tree, k = v.st->k, n = p.n, P = part_capacity(n, p.depth);
    int levels = v.st->level, n_parts = v.st->n_parts;
    if (levels < 0 || levels > p.depth || n_parts < 0 || n_parts > P) { v.st->error = 1; levels = 0; n_parts = 0; }
    const Tab tab = tab_of(v, levels);
    const int* src = rows_of(v, levels);                        // behind the last partition a part is a segment of this list
    const int n_leaves = 1 << levels;
    double* values = p.leaf_values + ((long)tree << p.depth);
    int* weights = p.leaf_weights + ((long)tree << p.depth);
    __syncthreads();                                            // every thread has read the state before thread 0 moves it on
    for (int j = tid; j < n_leaves; j += 1024) { values[j] = 0.0; weights[j] = 0; }        // an empty leaf
    __threadfence_block();
    __syncthreads();
    for (int s = wave; s < n_parts; s += 16) {                  // a wave per part: Qg = sum q and R = sum r over its rows, integers
        const int start = tab.start[s], leaf = tab.leaf[s];
        int m = tab.cnt[s];
        if (start < 0 || m < 1 || start > n - m || leaf < 0 || leaf >= n_leaves) { v.st->error = 1; continue; }
        long long Qg = 0, R = 0;
        for (int pos = lane; pos < m; pos += 64) {
            const int row = row_of(src, start + pos, n, v.st);
            Qg += v.q[row]; R += v.r[row];
        }
        for (int off = 32; off >= 1; off >>= 1) { Qg += __shfl_xor(Qg, off); R += __shfl_xor(R, off); }
        if (lane == 0) {
            values[leaf] = leaf_step(Qg, R, k, p.l2_leaf_reg, p.learning_rate);
            weights[leaf] = m;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        int leaf = v.leaf_of[i];
        if (leaf < 0 || leaf >= n_leaves) { v.st->error = 1; leaf = 0; }
        v.s[i] = v.s[i] + values[leaf];                         // float64, in tree order; the same thread reads it back in start_tree
    }
    __syncthreads();
    if (tid == 0) {
        p.tree_depth[tree] = v.st->error ? -1 : levels;         // the error word stays set: every later tree reports it too
        v.st->tree = tree + 1;
    }
    start_tree(p, v, tree + 1);                                 // behind the last tree this leaves approx = s + bias
}

// ---- proba: (1 - p1, p1) with p1 = sigmoid64(raw), the subtraction in float64 ------------------------------------------------------------
__global__ __launch_bounds__(256) void catc_proba_kernel(const double* raw, long m, double* proba) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double p1 = sigmoid64(raw[i]);
    proba[2 * i] = 1.0 - p1;
    proba[2 * i + 1] = p1;
}

int check_problem(const bbbp_catc_problem& p, int q) {
    BBBP_CHECK_ARG(p.n >= 2 && p.n <= BBBP_CAT_FIT_MAX_N, "catc_fit: problem %d: n %d outside 2..%d", q, p.n, BBBP_CAT_FIT_MAX_N);
    BBBP_CHECK_ARG(p.d >= 1 && p.d <= BBBP_CAT_FIT_MAX_D, "catc_fit: problem %d: d %d outside 1..%d", q, p.d, BBBP_CAT_FIT_MAX_D);
    BBBP_CHECK_ARG(p.iterations >= 1 && p.iterations <= BBBP_CAT_FIT_MAX_TREES, "catc_fit: problem %d: iterations %d outside 1..%d", q, p.iterations,
                   BBBP_CAT_FIT_MAX_TREES);
    BBBP_CHECK_ARG(p.depth >= 1 && p.depth <= BBBP_CAT_FIT_MAX_DEPTH, "catc_fit: problem %d: depth %d outside 1..%d", q, p.depth, BBBP_CAT_FIT_MAX_DEPTH);
    BBBP_CHECK_ARG(p.l2_leaf_reg >= 0.0 && p.l2_leaf_reg < INFINITY, "catc_fit: problem %d: l2_leaf_reg must be finite and >= 0", q);
    BBBP_CHECK_ARG(p.learning_rate > 0.0 && p.learning_rate < INFINITY, "catc_fit: problem %d: learning_rate must be positive and finite", q);
    BBBP_CHECK_ARG(p.bias == p.bias && fabs(p.bias) < INFINITY, "catc_fit: problem %d: bias must be finite", q);
    BBBP_CHECK_ARG(((long)p.iterations << p.depth) < (1L << 31), "catc_fit: problem %d: %d trees of %d leaves exceed 32-bit leaf indices", q, p.iterations,
                   1 << p.depth);
    BBBP_CHECK_ARG(!p.weights || p.weight_stride >= p.n, "catc_fit: problem %d: weight_stride %ld is below n %d", q, p.weight_stride, p.n);
    BBBP_CHECK_ARG(p.bins && p.n_cuts && p.t && p.work && p.split_feature && p.split_bin && p.leaf_values && p.leaf_weights && p.tree_depth && p.approx,
                   "catc_fit: problem %d: null pointer", q);
    return BBBP_OK;
}

// tools/bench_catc.py: with the profile on, every split launch of a fit sits between two events and the fit adds up their times
thread_local int g_profile = 0;
thread_local double g_split_ms = 0.0;
thread_local long g_launches = 0;

}  // namespace

extern "C" int bbbp_catc_fit_profile(int enable) { const int prev = g_profile; g_profile = enable != 0; return prev; }

extern "C" int bbbp_catc_fit_last(double* split_ms, long* launches) {
    BBBP_CHECK_ARG(split_ms && launches, "catc_fit_last: null pointer");
    *split_ms = g_split_ms; *launches = g_launches;
    return BBBP_OK;
}

extern "C" size_t bbbp_catc_fit_work_bytes(int n, int d, int depth) {
    if (n < 2 || n > BBBP_CAT_FIT_MAX_N || d < 1 || d > BBBP_CAT_FIT_MAX_D || depth < 1 || depth > BBBP_CAT_FIT_MAX_DEPTH) {
        bbbp_set_error("catc_fit_work_bytes: n %d outside 2..%d, d %d outside 1..%d or depth %d outside 1..%d", n, BBBP_CAT_FIT_MAX_N, d, BBBP_CAT_FIT_MAX_D,
                       depth, BBBP_CAT_FIT_MAX_DEPTH);
        return 0;
    }
    return work_layout(n, d, depth).total;
}

extern "C" int bbbp_catc_fit(void* stream, const bbbp_catc_problem* problems, const bbbp_catc_problem* problems_device, int n_problems) {
    BBBP_CHECK_ARG(problems && problems_device, "catc_fit: null pointer");
    BBBP_CHECK_ARG(n_problems >= 1 && n_problems <= 65535, "catc_fit: n_problems %d outside 1..65535", n_problems);
    int trees = 0, depth = 0, blocks_x = 1;
    for (int q = 0; q < n_problems; ++q) {
        const bbbp_catc_problem& p = problems[q];
        if (int rc = check_problem(p, q)) return rc;
        trees = p.iterations > trees ? p.iterations : trees;
        depth = p.depth > depth ? p.depth : depth;
        blocks_x = feature_blocks(p.d) > blocks_x ? feature_blocks(p.d) : blocks_x;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned P = (unsigned)n_problems;
    const dim3 feats((unsigned)blocks_x, P), one(P);
    hipLaunchKernelGGL(catc_init_kernel, one, dim3(1024), 0, st, problems_device);
    BBBP_CHECK_LAUNCH();
    hipEvent_t ev[2 * BBBP_CAT_FIT_MAX_DEPTH];
    const bool profile = g_profile != 0;
    if (profile)
        for (hipEvent_t& e : ev) BBBP_CHECK_HIP(hipEventCreate(&e));
    g_split_ms = 0.0; g_launches = 1;
    for (int t = 0; t < trees; ++t) {
        for (int l = 0; l < depth; ++l) {
            if (profile) BBBP_CHECK_HIP(hipEventRecord(ev[2 * l], st));
            hipLaunchKernelGGL(catc_split_kernel, feats, dim3(256), 0, st, problems_device);
            if (profile) BBBP_CHECK_HIP(hipEventRecord(ev[2 * l + 1], st));
            hipLaunchKernelGGL(catc_choose_kernel, one, dim3(256), 0, st, problems_device);
            hipLaunchKernelGGL(catc_partition_kernel, one, dim3(256), 0, st, problems_device);
        }
        hipLaunchKernelGGL(catc_update_kernel, one, dim3(1024), 0, st, problems_device);
        BBBP_CHECK_LAUNCH();
        g_launches += 3L * depth + 1;
        if (profile) {
            BBBP_CHECK_HIP(hipStreamSynchronize(st));
            for (int l = 0; l < depth; ++l) {
                float ms = 0.f;
                BBBP_CHECK_HIP(hipEventElapsedTime(&ms, ev[2 * l], ev[2 * l + 1]));
                g_split_ms += ms;
            }
        }
    }
    if (profile)
        for (hipEvent_t& e : ev) BBBP_CHECK_HIP(hipEventDestroy(e));
    BBBP_CHECK_HIP(hipStreamSynchronize(st));
    return BBBP_OK;
}

extern "C" int bbbp_catc_proba(void* stream, const double* raw, long m, double* proba) {
    BBBP_CHECK_ARG(m >= 0 && m <= (1L << 31) * 255L, "catc_proba: m %ld outside 0..%ld", m, (1L << 31) * 255L);
    if (m == 0) return BBBP_OK;
    BBBP_CHECK_ARG(raw && proba, "catc_proba: null pointer");
    hipLaunchKernelGGL(catc_proba_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), raw, m, proba);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
