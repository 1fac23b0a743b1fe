// Histogram-boosted classification trees, fitted on the GPU: the XGBClassifier of the classification stack (XGBClassifier(learning_rate=0.02,
// n_estimators=500, max_depth=7, colsample_bytree=0.8, subsample=0.8, reg_lambda=3, tree_method="hist"), Models/model_opt_20250130.py:445-456).
// XGBoost 2.0's hist updater for binary:logistic, restated so that no sum has an order (bbbp_amd/xgb.py states the algorithm,
// tests/xgbc_numpy.py restates it in numpy; the fit equals it bit for bit).  The rounds, the batching and the node tables are xgb.hip's; what
// differs from the regressor:
//   hessians   p = sigmoid32(margin) (IEEE operations only: the same bits as numpy), g = p - t, h = p (1 - p) in float32.  Beside q = llrint(g 2^k)
//              a row carries r = max(1, llrint(h 2^48)): a node's R = sum r is a second exact 64-bit integer (h <= 1/4, n <= 8192: R <= 2^59),
//              H = ldexp((double)R, -48).  R travels wherever Q does: r[n], the slot tables, the candidates, Best.r_left; the histogram form has
//              a third per-wave LDS array (8 KB + 8 KB + 4 KB per work-group), the lane-against-lane form carries r beside q
//   sampling   a row the tree's draw left out has q = r = 0, stays in the row list and takes its leaf's value; the draw is a counter-based hash
//              of (seed, tree, the row's position in the problem) made in the tree-start code.  The tree's eligible columns come as a bit
//              mask from the host; the split kernel skips the others (a wave-uniform decision)
//   candidates a boundary needs a row and R >= 1 on either side and H >= min_child_weight on either side (float64 comparisons); a child
//              takes a slot iff the tree may go deeper and the child has two rows; a node of R = 0 is a leaf of weight -0.0
// The file shares no code with xgb.hip on purpose: the regressor's bits are pinned and may not move.  Every index read from memory is
// kept inside its array (row_of, and the checks beside each store); a wrong one sets the problem's error word, which the fit reports as
// tree_nodes[t] = -1.
#include "common.h"
#include "bbbp_hip.h"
#include "tree_fit.h"

#include <math.h>

namespace {

constexpr int XGB_BLOCK_ROUNDS = 16;          // rounds enqueued between two reads of the `alive` word
constexpr int XGB_SMALL = 64;                 // nodes of at most this many rows take the lane-against-lane form
constexpr double XGB_RT_EPS = 1e-6;           // XGBoost's kRtEps: the smallest gain that splits
constexpr int XGB_NO_FEATURE = 0x7fffffff;
constexpr int XGB_H_BITS = 48;                // r = max(1, llrint(h 2^48))

struct State { int tree, level, n_slots, n_next, n_nodes, final, error, k; };

__host__ __device__ inline int slot_capacity(int n) { return n / 2 < 1 ? 1 : n / 2; }
// features per work-group of the split kernel, a multiple of four (one wave takes every fourth): at most 256 feature blocks
__host__ __device__ inline int features_per_block(int d) {
    const int blocks = (d + 3) / 4 < 256 ? (d + 3) / 4 : 256;
    return ((d + blocks - 1) / blocks + 3) / 4 * 4;
}
__host__ __device__ inline int feature_blocks(int d) { const int f = features_per_block(d); return (d + f - 1) / f; }
__host__ __device__ inline int tree_capacity(int n, int max_depth) {
    const long by_rows = 2L * n - 1, by_depth = max_depth >= 30 ? (1L << 31) - 1 : (2L << max_depth) - 1;
    return (int)(by_rows < by_depth ? by_rows : by_depth);
}

struct Work {                                 // offsets into a problem's `work`, in bytes; all multiples of 16
    size_t rows[2], q, r, leaf_value, tab_start[2], tab_cnt[2], tab_node[2], tab_q[2], tab_r[2], s_feature, s_bin, s_mleft, s_flags, s_lval, s_rval,
        cand_gain, cand_q, cand_r, cand_fb, cand_m, state, total;
};
__host__ __device__ inline Work work_layout(int n, int d) {
    Work w;
    Area a;
    const size_t S = (size_t)slot_capacity(n), C = S * (size_t)feature_blocks(d);
    w.rows[0] = a.take((size_t)n * 4); w.rows[1] = a.take((size_t)n * 4);
    w.q = a.take((size_t)n * 8); w.r = a.take((size_t)n * 8);
    w.leaf_value = a.take((size_t)n * 4);
    w.tab_start[0] = a.take(S * 4); w.tab_start[1] = a.take(S * 4);
    w.tab_cnt[0] = a.take(S * 4); w.tab_cnt[1] = a.take(S * 4);
    w.tab_node[0] = a.take(S * 4); w.tab_node[1] = a.take(S * 4);
    w.tab_q[0] = a.take(S * 8); w.tab_q[1] = a.take(S * 8);
    w.tab_r[0] = a.take(S * 8); w.tab_r[1] = a.take(S * 8);
    w.s_feature = a.take(S * 4); w.s_bin = a.take(S * 4); w.s_mleft = a.take(S * 4); w.s_flags = a.take(S * 4);
    w.s_lval = a.take(S * 4); w.s_rval = a.take(S * 4);
    w.cand_gain = a.take(C * 8); w.cand_q = a.take(C * 8); w.cand_r = a.take(C * 8); w.cand_fb = a.take(C * 4); w.cand_m = a.take(C * 4);
    w.state = a.take(sizeof(State));
    w.total = a.at;
    return w;
}

struct Tab { int *start, *cnt, *node; long long *q, *r; };   // the slots of one level
struct View {                                 // a problem's work area, typed
    int *rows_a, *rows_b; long long *q, *r; float* leaf_value; Tab tab_a, tab_b;
    int *s_feature, *s_bin, *s_mleft, *s_flags; float *s_lval, *s_rval;
    double* cand_gain; long long *cand_q, *cand_r; int *cand_fb, *cand_m; State* st;
};
__device__ inline View view_of(const bbbp_xgbc_problem& p) {
    const Work w = work_layout(p.n, p.d);
    char* b = static_cast<char*>(p.work);
    View v;
    v.rows_a = (int*)(b + w.rows[0]); v.rows_b = (int*)(b + w.rows[1]);
    v.q = (long long*)(b + w.q); v.r = (long long*)(b + w.r); v.leaf_value = (float*)(b + w.leaf_value);
    v.tab_a = Tab{(int*)(b + w.tab_start[0]), (int*)(b + w.tab_cnt[0]), (int*)(b + w.tab_node[0]), (long long*)(b + w.tab_q[0]), (long long*)(b + w.tab_r[0])};
    v.tab_b = Tab{(int*)(b + w.tab_start[1]), (int*)(b + w.tab_cnt[1]), (int*)(b + w.tab_node[1]), (long long*)(b + w.tab_q[1]), (long long*)(b + w.tab_r[1])};
    v.s_feature = (int*)(b + w.s_feature); v.s_bin = (int*)(b + w.s_bin); v.s_mleft = (int*)(b + w.s_mleft); v.s_flags = (int*)(b + w.s_flags);
    v.s_lval = (float*)(b + w.s_lval); v.s_rval = (float*)(b + w.s_rval);
    v.cand_gain = (double*)(b + w.cand_gain); v.cand_q = (long long*)(b + w.cand_q); v.cand_r = (long long*)(b + w.cand_r);
    v.cand_fb = (int*)(b + w.cand_fb); v.cand_m = (int*)(b + w.cand_m);
    v.st = (State*)(b + w.state);
    return v;
}
// selects, not indexed arrays: no scratch.  Level L reads rows_of(L) and tab_of(L); partition and choose write those of L + 1
__device__ inline int* rows_of(const View& v, int level) { return (level & 1) ? v.rows_b : v.rows_a; }
__device__ inline Tab tab_of(const View& v, int level) {
    const bool b = level & 1;
    return Tab{b ? v.tab_b.start : v.tab_a.start, b ? v.tab_b.cnt : v.tab_a.cnt, b ? v.tab_b.node : v.tab_a.node, b ? v.tab_b.q : v.tab_a.q,
               b ? v.tab_b.r : v.tab_a.r};
}
__device__ inline bool problem_idle(const bbbp_xgbc_problem& p, const State* st) { return st->tree >= p.n_estimators; }

// ---- the sigmoid: IEEE operations only (the file is compiled with -ffp-contract=off), so numpy gives the same bits -----------------------
// exp(-|x|) by fdlibm's reduction a = k ln2 + r and the Taylor polynomial of degree 13 in r (|r| <= ln2 / 2: its remainder is below 2^-64),
// in float64; one rounding to float32 at the end.  The clamp at -87 keeps p a normal float32.
__device__ inline float sigmoid32(float x) {
    const double LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33, INV_LN2 = 0x1.71547652b82fep+0;
    const double z = (double)x;
    const double a = fmax(-fabs(z), -87.0);
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
    const double s = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    return (float)s;
}

// ---- the draws: u(stream, tree, i) = mix(mix(mix(seed + golden (stream + 1)) + tree) + i), rf_mix being the splitmix64 finaliser ------------
__device__ inline unsigned long long tree_key(unsigned long long seed, unsigned long long stream, unsigned long long tree) {
    return rf_mix(rf_mix(seed + 0x9e3779b97f4a7c15ull * (stream + 1ull)) + tree);
}
__device__ inline bool row_sampled(unsigned long long key, int i, unsigned threshold) {
    return threshold == 0u || (unsigned)(rf_mix(key + (unsigned long long)i) >> 32) < threshold;
}

// ---- the score ----------------------------------------------------------------------------------------------------------------------
__device__ inline double to_G(long long Q, int k) { return ldexp((double)Q, -k); }          // one rounding, then an exact scaling
__device__ inline double to_H(long long R) { return ldexp((double)R, -XGB_H_BITS); }
__device__ inline double score_term(double G, double H, double lambda) { return G * G / (H + lambda); }
__device__ inline double node_weight(double G, double H, double lambda) { return -G / (H + lambda); }
__device__ inline float leaf_value_of(double w, float learning_rate) { return (float)((double)learning_rate * w); }

struct Best { double gain; long long q_left, r_left; int feature, bin, m_left; };
__device__ inline Best no_candidate() { return Best{-INFINITY, 0, 0, XGB_NO_FEATURE, 0, 0}; }
// the tie rule: the larger gain, among equal gains the lowest feature, then the lowest bin
__device__ inline bool better(const Best& a, const Best& b) {
    return a.gain > b.gain || (a.gain == b.gain && (a.feature < b.feature || (a.feature == b.feature && a.bin < b.bin)));
}
struct Node { long long Q, R; int m, k; double lambda, min_child_weight, parent_term; };
// a boundary is a candidate iff either side has a row, R >= 1 and H >= min_child_weight
__device__ inline void offer(Best& best, long long q_left, long long r_left, int m_left, const Node& nd, int feature, int bin) {
    const long long r_right = nd.R - r_left;
    if (m_left < 1 || nd.m - m_left < 1 || r_left < 1 || r_right < 1) return;
    const double H_l = to_H(r_left), H_r = to_H(r_right);
    if (!(H_l >= nd.min_child_weight) || !(H_r >= nd.min_child_weight)) return;
    const double gain = (score_term(to_G(q_left, nd.k), H_l, nd.lambda) + score_term(to_G(nd.Q - q_left, nd.k), H_r, nd.lambda)) - nd.parent_term;
    const Best c{gain, q_left, r_left, feature, bin, m_left};
    if (better(c, best)) best = c;
}
__device__ inline Best wave_best(Best b) {
    for (int off = 32; off >= 1; off >>= 1) {
        const Best o{__shfl_xor(b.gain, off), __shfl_xor(b.q_left, off), __shfl_xor(b.r_left, off), __shfl_xor(b.feature, off), __shfl_xor(b.bin, off),
                     __shfl_xor(b.m_left, off)};
        if (better(o, b)) b = o;
    }
    return b;
}
__device__ inline long long readlane64(long long x, int lane) {         // `lane` is uniform over the wave
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned long long)x, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)((unsigned long long)x >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// ---- grad: a tree's gradients, hessians, row draw and its root (one work-group of 1024 threads per problem; every thread calls it) -------
__device__ inline void start_tree(const bbbp_xgbc_problem& p, const View& v, int tree) {
    __shared__ float red_f[1024];
    __shared__ long long red_q[1024];
    const int tid = threadIdx.x;
    const unsigned long long key = tree_key(p.seed, 0ull, (unsigned long long)tree);
    float gmax = 0.f;                                           // over the sampled rows only
    for (int i = tid; i < p.n; i += 1024)
        if (row_sampled(key, i, p.subsample_threshold)) gmax = fmaxf(gmax, fabsf(sigmoid32(p.margin[i]) - p.y[i]));
    red_f[tid] = gmax;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) red_f[tid] = fmaxf(red_f[tid], red_f[tid + w]);
        __syncthreads();
    }
    gmax = red_f[0];
    const int k = gmax == 0.f ? 0 : 47 - ilogb((double)gmax);
    long long sum_q = 0, sum_r = 0;
    for (int i = tid; i < p.n; i += 1024) {
        long long q = 0, r = 0;
        if (row_sampled(key, i, p.subsample_threshold)) {
            const float pr = sigmoid32(p.margin[i]);
            const float g = pr - p.y[i];
            const float h = pr * (1.f - pr);                    // the subtraction and the product each rounded to float32
            q = llrint(ldexp((double)g, k));                    // the product is exact: g has 24 bits below 2^(ilogb + 1)
            r = llrint(ldexp((double)h, XGB_H_BITS));
            r = r < 1 ? 1 : r;
        }
        v.q[i] = q; v.r[i] = r;
        v.rows_a[i] = i;
        sum_q += q; sum_r += r;
    }
    red_q[tid] = sum_q;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) red_q[tid] += red_q[tid + w];              // integers: the order of the additions cannot change a bit
        __syncthreads();
    }
    const long long Q = red_q[0];
    __syncthreads();
    red_q[tid] = sum_r;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) red_q[tid] += red_q[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        v.tab_a.start[0] = 0; v.tab_a.cnt[0] = p.n; v.tab_a.node[0] = 0; v.tab_a.q[0] = Q; v.tab_a.r[0] = red_q[0];
        v.st->level = 0; v.st->n_slots = 1; v.st->n_next = 0; v.st->n_nodes = 1; v.st->final = 0; v.st->k = k;
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void xgbc_init_kernel(const bbbp_xgbc_problem* problems) {
    const bbbp_xgbc_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    for (int i = threadIdx.x; i < p.n; i += 1024) p.margin[i] = p.base_margin;     // the same thread reads it back in start_tree
    if (threadIdx.x == 0) { v.st->tree = 0; v.st->error = 0; }
    start_tree(p, v, 0);
}

// ---- split: the best boundary per (slot, feature block) -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xgbc_split_kernel(const bbbp_xgbc_problem* problems) {
    const bbbp_xgbc_problem p = problems[blockIdx.y];
    const View v = view_of(p);
    if (problem_idle(p, v.st)) return;
    const int fpb = features_per_block(p.d), f0 = blockIdx.x * fpb;
    if (f0 >= p.d) return;                                      // the grid is sized for the widest problem of the batch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = p.n;
    const int level = v.st->level, n_slots = v.st->n_slots, k = v.st->k;
    int tree = v.st->tree;
    tree = tree < 0 ? 0 : tree;                                 // below n_estimators: the problem is not idle
    const unsigned* mask = p.col_mask ? p.col_mask + (long)tree * p.col_mask_stride : nullptr;      // [col_mask_stride] words of this tree
    const Tab tab = tab_of(v, level);
    const int* src = rows_of(v, level);
    const long S = slot_capacity(n);
    __shared__ unsigned long long hist_q[4][256];               // a wave's own histograms: only its lanes touch them
    __shared__ unsigned long long hist_r[4][256];
    __shared__ int hist_c[4][256];
    __shared__ double wb_gain[2][4];
    __shared__ long long wb_q[2][4], wb_r[2][4];
    __shared__ int wb_feature[2][4], wb_bin[2][4], wb_m[2][4];
    for (int s = 0; s < n_slots && s < S; ++s) {
        const int start = tab.start[s];
        int m = tab.cnt[s];
        if (start < 0 || m < 0 || start > n - m) { v.st->error = 1; m = 0; }
        Node nd;
        nd.Q = tab.q[s]; nd.R = tab.r[s]; nd.m = m; nd.k = k; nd.lambda = p.reg_lambda; nd.min_child_weight = p.min_child_weight;
        nd.parent_term = score_term(to_G(nd.Q, k), to_H(nd.R), nd.lambda);      // NaN for R = 0 and lambda = 0: such a node has no candidate
        Best best = no_candidate();
        if (m <= XGB_SMALL) {                                   // one row per lane, counted lane against lane
            int row = 0;
            long long q_own = 0, r_own = 0;
            if (lane < m) { row = row_of(src, start + lane, n, v.st); q_own = v.q[row]; r_own = v.r[row]; }
            for (int f = f0 + wave; f < f0 + fpb && f < p.d; f += 4) {
                if (mask && !((mask[f >> 5] >> (f & 31)) & 1u)) continue;       // f is the wave's: all lanes skip together
                const int b = lane < m ? p.bins[(long)f * n + row] : 256;
                long long q_left = 0, r_left = 0;
                int m_left = 0;
                for (int j = 0; j < m; ++j) {
                    const int b_j = __builtin_amdgcn_readlane(b, j);
                    const long long q_j = readlane64(q_own, j), r_j = readlane64(r_own, j);
                    if (b_j <= b) { q_left += q_j; r_left += r_j; ++m_left; }
                }
                if (lane < m) offer(best, q_left, r_left, m_left, nd, f, b);
            }
        } else {                                                // the 256-bin histograms of (sum q, sum r, count), four bins per lane
            for (int j = 0; j < fpb; j += 4) {                  // the same trip count in every wave: the barriers are the group's
                const int f = f0 + j + wave;
                const bool live = f < p.d && (!mask || ((mask[f >> 5] >> (f & 31)) & 1u));
                for (int t = 0; t < 4; ++t) { hist_q[wave][4 * lane + t] = 0ull; hist_r[wave][4 * lane + t] = 0ull; hist_c[wave][4 * lane + t] = 0; }
                __syncthreads();
                if (live)
                    for (int pos = lane; pos < m; pos += 64) {
                        const int row = row_of(src, start + pos, n, v.st);
                        const int b = p.bins[(long)f * n + row];
                        atomicAdd(&hist_q[wave][b], (unsigned long long)v.q[row]);
                        atomicAdd(&hist_r[wave][b], (unsigned long long)v.r[row]);
                        atomicAdd(&hist_c[wave][b], 1);
                    }
                __syncthreads();
                if (live) {
                    long long q4[4], r4[4];
                    int c4[4];
                    long long q_run = 0, r_run = 0;
                    int c_run = 0;
                    for (int t = 0; t < 4; ++t) {
                        q_run += (long long)hist_q[wave][4 * lane + t]; r_run += (long long)hist_r[wave][4 * lane + t]; c_run += hist_c[wave][4 * lane + t];
                        q4[t] = q_run; r4[t] = r_run; c4[t] = c_run;
                    }
                    long long q_incl = q_run, r_incl = r_run;
                    int c_incl = c_run;
                    for (int off = 1; off < 64; off <<= 1) {
                        const long long pq = __shfl_up(q_incl, off), pr = __shfl_up(r_incl, off);
                        const int pc = __shfl_up(c_incl, off);
                        if (lane >= off) { q_incl += pq; r_incl += pr; c_incl += pc; }
                    }
                    const long long q_before = q_incl - q_run, r_before = r_incl - r_run;
                    const int c_before = c_incl - c_run;
                    for (int t = 0; t < 4; ++t) offer(best, q_before + q4[t], r_before + r4[t], c_before + c4[t], nd, f, 4 * lane + t);
                }
            }
        }
        best = wave_best(best);
        const int par = s & 1;                                  // two rows: a wave writes the next slot's while thread 0 still reads this one's
        if (lane == 0) {
            wb_gain[par][wave] = best.gain; wb_q[par][wave] = best.q_left; wb_r[par][wave] = best.r_left; wb_feature[par][wave] = best.feature;
            wb_bin[par][wave] = best.bin; wb_m[par][wave] = best.m_left;
        }
        __syncthreads();
        if (tid == 0) {
            Best all = no_candidate();
            for (int w = 0; w < 4; ++w) {
                const Best c{wb_gain[par][w], wb_q[par][w], wb_r[par][w], wb_feature[par][w], wb_bin[par][w], wb_m[par][w]};
                if (better(c, all)) all = c;
            }
            const long at = (long)blockIdx.x * S + s;
            v.cand_gain[at] = all.gain; v.cand_q[at] = all.q_left; v.cand_r[at] = all.r_left; v.cand_m[at] = all.m_left;
            v.cand_fb[at] = all.feature == XGB_NO_FEATURE ? -1 : all.feature * 256 + all.bin;
        }
    }
}

// ---- choose: the best candidate per slot, the stop rule, the node's arrays, the children ----------------------------------------------
__device__ inline void store_leaf(const bbbp_xgbc_problem& p, long node, float value, double H) {
    p.left[node] = -1; p.right[node] = -1; p.feature[node] = 0; p.cond[node] = value;
    p.base_weight[node] = value; p.loss_change[node] = 0.f; p.sum_hessian[node] = (float)H;
}

__global__ __launch_bounds__(256) void xgbc_choose_kernel(const bbbp_xgbc_problem* problems) {
    const bbbp_xgbc_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    if (problem_idle(p, v.st)) return;
    const int tid = threadIdx.x, n = p.n;
    const int level = v.st->level, n_slots = v.st->n_slots, n_nodes = v.st->n_nodes, k = v.st->k;
    const Tab tab = tab_of(v, level), next = tab_of(v, level + 1);
    const int S = slot_capacity(n), blocks = feature_blocks(p.d), cap = tree_capacity(n, p.max_depth);
    const long base = (long)v.st->tree * cap;
    const double lambda = p.reg_lambda;
    const bool deeper = level + 1 < p.max_depth;
    __shared__ int wave_cnt[3][2][4];
    int splits = 0, next_left = 0, next_right = 0;              // running totals over the passes
    for (int s0 = 0, it = 0; s0 < n_slots && s0 < S; s0 += 256, ++it) {
        const int s = s0 + tid;
        const bool in = s < n_slots && s < S;
        Best best = no_candidate();
        if (in)
            for (int b = 0; b < blocks; ++b) {
                const long at = (long)b * S + s;
                const int fb = v.cand_fb[at];
                if (fb < 0) continue;
                const Best c{v.cand_gain[at], v.cand_q[at], v.cand_r[at], fb >> 8, fb & 255, v.cand_m[at]};
                if (better(c, best)) best = c;
            }
        const int start = in ? tab.start[s] : 0, m = in ? tab.cnt[s] : 0, node = in ? tab.node[s] : 0;
        const long long Q = in ? tab.q[s] : 0, R = in ? tab.r[s] : 0;
        bool split = in && best.feature != XGB_NO_FEATURE && best.gain > XGB_RT_EPS && best.gain >= p.gamma;
        if (split && (best.feature >= p.d || best.bin >= p.cut_stride || best.m_left < 1 || best.m_left >= m || best.r_left < 1 || best.r_left >= R)) {
            v.st->error = 1; split = false;
        }
        const int m_l = best.m_left, m_r = m - best.m_left;
        const bool slot_l = split && deeper && m_l >= 2, slot_r = split && deeper && m_r >= 2;
        const int rank = block_rank_before(split, wave_cnt[0][it & 1], splits);
        const int lefts_before = block_rank_before(slot_l, wave_cnt[1][it & 1], next_left);
        const int at_l = lefts_before + block_rank_before(slot_r, wave_cnt[2][it & 1], next_right);      // slots in ascending node id
        if (!in) continue;
        if ((unsigned)node >= (unsigned)cap) { v.st->error = 1; continue; }
        const double H = to_H(R);
        const double w = R == 0 ? -0.0 : node_weight(to_G(Q, k), H, lambda);       // every row unsampled: a leaf of weight 0, stored as -0.0
        if (!split) {                                           // a leaf: its rows get the value in `partition`
            const float value = leaf_value_of(w, p.learning_rate);
            store_leaf(p, base + node, value, H);
            v.s_feature[s] = -1; v.s_lval[s] = value;
            continue;
        }
        const int lc = n_nodes + 2 * rank, rc = lc + 1;
        if (rc >= cap || at_l + (slot_l ? 1 : 0) + (slot_r ? 1 : 0) > S) {      // cannot happen: 2 n - 1 nodes and n / 2 slots are enough
            v.st->error = 1;
            store_leaf(p, base + node, 0.f, H);
            v.s_feature[s] = -1; v.s_lval[s] = 0.f;
            continue;
        }
        p.left[base + node] = lc; p.right[base + node] = rc; p.feature[base + node] = best.feature;
        p.cond[base + node] = p.cuts[(long)best.feature * p.cut_stride + best.bin];
        p.base_weight[base + node] = (float)w; p.loss_change[base + node] = (float)best.gain; p.sum_hessian[base + node] = (float)H;
        const double H_l = to_H(best.r_left), H_r = to_H(R - best.r_left);
        const float v_l = leaf_value_of(node_weight(to_G(best.q_left, k), H_l, lambda), p.learning_rate);
        const float v_r = leaf_value_of(node_weight(to_G(Q - best.q_left, k), H_r, lambda), p.learning_rate);
        v.s_feature[s] = best.feature; v.s_bin[s] = best.bin; v.s_mleft[s] = m_l;
        v.s_flags[s] = (slot_l ? 0 : 1) | (slot_r ? 0 : 2); v.s_lval[s] = v_l; v.s_rval[s] = v_r;
        if (slot_l) { next.start[at_l] = start; next.cnt[at_l] = m_l; next.node[at_l] = lc; next.q[at_l] = best.q_left; next.r[at_l] = best.r_left; }
        else store_leaf(p, base + lc, v_l, H_l);
        const int at_r = at_l + (slot_l ? 1 : 0);
        if (slot_r) { next.start[at_r] = start + m_l; next.cnt[at_r] = m_r; next.node[at_r] = rc; next.q[at_r] = Q - best.q_left; next.r[at_r] = R - best.r_left; }
        else store_leaf(p, base + rc, v_r, H_r);
    }
    __syncthreads();
    if (tid == 0) {
        v.st->n_nodes = n_nodes + 2 * splits;
        v.st->n_next = next_left + next_right;
        v.st->final = next_left + next_right == 0;
    }
}

// ---- partition: a slot's rows, stably, by bin <= split bin; the rows of new leaves take their leaf's value ------------------------------
__global__ __launch_bounds__(256) void xgbc_partition_kernel(const bbbp_xgbc_problem* problems) {
    const bbbp_xgbc_problem p = problems[blockIdx.y];
    const View v = view_of(p);
    if (problem_idle(p, v.st)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = p.n;
    const int level = v.st->level, n_slots = v.st->n_slots, S = slot_capacity(n);
    const Tab tab = tab_of(v, level);
    const int* src = rows_of(v, level);
    int* dst = rows_of(v, level + 1);
    for (int s = blockIdx.x * 4 + wave; s < n_slots && s < S; s += gridDim.x * 4) {
        const int start = tab.start[s], m = tab.cnt[s], f = v.s_feature[s];
        if (start < 0 || m < 0 || start > n - m || f >= p.d) { v.st->error = 1; continue; }
        if (f < 0) {                                            // the slot became a leaf: its rows stay put
            const float value = v.s_lval[s];
            for (int pos = lane; pos < m; pos += 64) v.leaf_value[row_of(src, start + pos, n, v.st)] = value;
            continue;
        }
        const int bin = v.s_bin[s], m_l = v.s_mleft[s], flags = v.s_flags[s];
        const float v_l = v.s_lval[s], v_r = v.s_rval[s];
        int lefts = 0;                                          // rows going left in front of this pass
        for (int pos0 = 0; pos0 < m; pos0 += 64) {
            const int pos = pos0 + lane;
            const bool in = pos < m;
            const int row = in ? row_of(src, start + pos, n, v.st) : 0;
            const bool left = in && p.bins[(long)f * n + row] <= bin;
            const unsigned long long ballot = __ballot(left);
            const int before = lefts + __popcll(ballot & ((1ull << lane) - 1ull));
            if (in) {
                const int to = left ? before : m_l + (pos - before);
                if (to >= 0 && to < m) dst[start + to] = row;
                else v.st->error = 1;
                if (left && (flags & 1)) v.leaf_value[row] = v_l;
                if (!left && (flags & 2)) v.leaf_value[row] = v_r;
            }
            lefts += __popcll(ballot);
        }
        if (lefts != m_l) v.st->error = 1;                      // the histogram and the partition disagree: cannot happen
    }
}

// ---- update: a level more, or a finished tree's margins and the next tree's gradients --------------------------------------------------
__global__ __launch_bounds__(1024) void xgbc_update_kernel(const bbbp_xgbc_problem* problems, int* alive, int tell) {
    const bbbp_xgbc_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    if (problem_idle(p, v.st)) return;
    const int tid = threadIdx.x, tree = v.st->tree;
    const bool final = v.st->final;
    __syncthreads();
    if (!final) {
        if (tid == 0) { v.st->level = v.st->level + 1; v.st->n_slots = v.st->n_next; }
        if (tid == 0 && tell) *alive = 1;
        return;
    }
    for (int i = tid; i < p.n; i += 1024) p.margin[i] = p.margin[i] + v.leaf_value[i];       // float32; the same thread reads it back in start_tree
    if (tid == 0) {
        p.tree_nodes[tree] = v.st->error ? -1 : v.st->n_nodes;  // the error word stays set: every later tree reports it too
        v.st->tree = tree + 1;
    }
    if (tree + 1 >= p.n_estimators) return;
    start_tree(p, v, tree + 1);
    if (tid == 0 && tell) *alive = 1;
}

// ---- proba: (1 - p1, p1) with p1 = sigmoid32(margin), the subtraction in float32 ---------------------------------------------------------
__global__ __launch_bounds__(256) void xgbc_proba_kernel(const float* margin, long m, float* proba) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float p1 = sigmoid32(margin[i]);
    proba[2 * i] = 1.f - p1;
    proba[2 * i + 1] = p1;
}

int check_problem(const bbbp_xgbc_problem& p, int q) {
    BBBP_CHECK_ARG(p.n >= 2 && p.n <= BBBP_XGB_FIT_MAX_N, "xgbc_fit: problem %d: n %d outside 2..%d", q, p.n, BBBP_XGB_FIT_MAX_N);
    BBBP_CHECK_ARG(p.d >= 1 && p.d <= BBBP_XGB_FIT_MAX_D, "xgbc_fit: problem %d: d %d outside 1..%d", q, p.d, BBBP_XGB_FIT_MAX_D);
    BBBP_CHECK_ARG(p.cut_stride >= 1 && p.cut_stride <= 255, "xgbc_fit: problem %d: cut_stride %d outside 1..255", q, p.cut_stride);
    BBBP_CHECK_ARG(p.n_estimators >= 1 && p.n_estimators <= BBBP_XGB_FIT_MAX_TREES, "xgbc_fit: problem %d: n_estimators %d outside 1..%d", q, p.n_estimators,
                   BBBP_XGB_FIT_MAX_TREES);
    BBBP_CHECK_ARG(p.max_depth >= 1 && p.max_depth <= BBBP_XGB_FIT_MAX_DEPTH, "xgbc_fit: problem %d: max_depth %d outside 1..%d", q, p.max_depth,
                   BBBP_XGB_FIT_MAX_DEPTH);
    BBBP_CHECK_ARG(p.reg_lambda >= 0.0 && p.reg_lambda < INFINITY, "xgbc_fit: problem %d: reg_lambda must be finite and >= 0", q);
    BBBP_CHECK_ARG(p.gamma >= 0.0 && p.gamma < INFINITY, "xgbc_fit: problem %d: gamma must be finite and >= 0", q);
    BBBP_CHECK_ARG(p.min_child_weight >= 0.0 && p.min_child_weight < INFINITY, "xgbc_fit: problem %d: min_child_weight must be finite and >= 0", q);
    BBBP_CHECK_ARG(p.learning_rate > 0.f && p.learning_rate < INFINITY, "xgbc_fit: problem %d: learning_rate must be positive and finite", q);
    BBBP_CHECK_ARG(p.base_margin == p.base_margin && fabsf(p.base_margin) < INFINITY, "xgbc_fit: problem %d: base_margin must be finite", q);
    BBBP_CHECK_ARG((long)p.n_estimators * tree_capacity(p.n, p.max_depth) < (1L << 31), "xgbc_fit: problem %d: %d trees of %d nodes exceed 32-bit node indices", q,
                   p.n_estimators, tree_capacity(p.n, p.max_depth));
    BBBP_CHECK_ARG(!p.col_mask || p.col_mask_stride >= (p.d + 31) / 32, "xgbc_fit: problem %d: col_mask_stride %d is less than ceil(d / 32) = %d", q,
                   p.col_mask_stride, (p.d + 31) / 32);
    BBBP_CHECK_ARG(p.bins && p.cuts && p.y && p.work && p.left && p.right && p.feature && p.cond && p.base_weight && p.loss_change && p.sum_hessian &&
                       p.tree_nodes && p.margin, "xgbc_fit: problem %d: null pointer", q);
    return BBBP_OK;
}

}  // namespace

extern "C" int bbbp_xgbc_fit_tree_capacity(int n, int max_depth) {
    if (n < 2 || n > BBBP_XGB_FIT_MAX_N || max_depth < 1 || max_depth > BBBP_XGB_FIT_MAX_DEPTH) {
        bbbp_set_error("xgbc_fit_tree_capacity: n %d outside 2..%d or max_depth %d outside 1..%d", n, BBBP_XGB_FIT_MAX_N, max_depth, BBBP_XGB_FIT_MAX_DEPTH);
        return 0;
    }
    return tree_capacity(n, max_depth);
}

extern "C" size_t bbbp_xgbc_fit_work_bytes(int n, int d) {
    if (n < 2 || n > BBBP_XGB_FIT_MAX_N || d < 1 || d > BBBP_XGB_FIT_MAX_D) {
        bbbp_set_error("xgbc_fit_work_bytes: n %d outside 2..%d or d %d outside 1..%d", n, BBBP_XGB_FIT_MAX_N, d, BBBP_XGB_FIT_MAX_D);
        return 0;
    }
    return work_layout(n, d).total;
}

extern "C" int bbbp_xgbc_proba(void* stream, const float* margin, long m, float* proba) {
    BBBP_CHECK_ARG(m >= 0 && m < (1L << 38), "xgbc_proba: m %ld outside 0..2^38", m);
    if (m == 0) return BBBP_OK;
    BBBP_CHECK_ARG(margin && proba, "xgbc_proba: null pointer");
    hipLaunchKernelGGL(xgbc_proba_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), margin, m, proba);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_xgbc_fit(void* stream, const bbbp_xgbc_problem* problems, const bbbp_xgbc_problem* problems_device, int n_problems, int* alive_device) {
    BBBP_CHECK_ARG(problems && problems_device && alive_device, "xgbc_fit: null pointer");
    BBBP_CHECK_ARG(n_problems >= 1 && n_problems <= 65535, "xgbc_fit: n_problems %d outside 1..65535", n_problems);
    int max_n = 0;
    long rounds = 0;
    for (int q = 0; q < n_problems; ++q) {
        const bbbp_xgbc_problem& p = problems[q];
        if (int rc = check_problem(p, q)) return rc;
        max_n = p.n > max_n ? p.n : max_n;
        // a tree searches the levels above max_depth, and no more levels than it has rows to part; the root's level always
        const int levels = p.max_depth < p.n - 1 ? p.max_depth : p.n - 1;
        const long r = (long)p.n_estimators * (levels < 1 ? 1 : levels);
        rounds = r > rounds ? r : rounds;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned P = (unsigned)n_problems;
    int blocks_x = 1;
    for (int q = 0; q < n_problems; ++q) blocks_x = feature_blocks(problems[q].d) > blocks_x ? feature_blocks(problems[q].d) : blocks_x;
    const dim3 feats((unsigned)blocks_x, P), slots((unsigned)clampi(cdiv(slot_capacity(max_n), 4), 1, 64), P), one(P);
    hipLaunchKernelGGL(xgbc_init_kernel, one, dim3(1024), 0, st, problems_device);
    BBBP_CHECK_LAUNCH();
    const long max_blocks = rounds / XGB_BLOCK_ROUNDS + 2;
    for (long b = 0; b < max_blocks; ++b) {
        BBBP_CHECK_HIP(hipMemsetAsync(alive_device, 0, sizeof(int), st));
        for (int r = 0; r < XGB_BLOCK_ROUNDS; ++r) {
            hipLaunchKernelGGL(xgbc_split_kernel, feats, dim3(256), 0, st, problems_device);
            hipLaunchKernelGGL(xgbc_choose_kernel, one, dim3(256), 0, st, problems_device);
            hipLaunchKernelGGL(xgbc_partition_kernel, slots, dim3(256), 0, st, problems_device);
            hipLaunchKernelGGL(xgbc_update_kernel, one, dim3(1024), 0, st, problems_device, alive_device, r == XGB_BLOCK_ROUNDS - 1 ? 1 : 0);
            BBBP_CHECK_LAUNCH();
        }
        int alive = 0;                                          // the only host read before the result
        BBBP_CHECK_HIP(hipMemcpyAsync(&alive, alive_device, sizeof(int), hipMemcpyDeviceToHost, st));
        BBBP_CHECK_HIP(hipStreamSynchronize(st));
        if (!alive) return BBBP_OK;
    }
    bbbp_set_error("xgbc_fit: a problem still grows after %ld rounds", max_blocks * XGB_BLOCK_ROUNDS);
    return BBBP_ERR_HIP;
}
