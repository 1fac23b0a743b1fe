// Histogram-boosted regression trees, fitted on the GPU: the xgb base learner of the logBB stack (XGBRegressor(n_estimators=300,
// learning_rate=0.01, max_depth=30, tree_method="hist") over hstack([fingerprint, image]) = 49 319 columns on about 1 058 rows,
// Models/multi_input_data_regression_opt_transformer_cnn_20250108.py:186-189).  XGBoost 2.0's hist updater for reg:squarederror, restated so
// that no sum has an order (bbbp_amd/xgb.py states the algorithm, tests/xgb_numpy.py restates it in numpy; the fit equals it bit for bit):
// features are bytes, bin(x) = the number of the feature's cuts <= x; g = margin - y in float32, h = 1; per tree k = 47 - ilogb(max |g|)
// and q = llrint(g 2^k), so a node's Q = sum q is an exact 64-bit integer, G = ldexp((double)Q, -k), H = its row count; a boundary between
// two bins scores (G_L^2 / (H_L + lambda) + G_R^2 / (H_R + lambda)) - G^2 / (H + lambda) in float64, every operation rounded on its own
// (the file is compiled with -ffp-contract=off); the best boundary wins, the lowest feature and then the lowest bin among equal gains.
//
// A *problem* is one model being fitted; problems run side by side in one batch (five folds and the refit).  Few rows, tens of thousands
// of low-cardinality columns, trees that grow until rows are alone: the state of a problem is its feature-major byte matrix
// bins[d][n], ONE row list partitioned into the level's nodes (no sorted order per feature: gbt.hip and rf.hip keep d of them) and node
// tables by slot in global memory.  A *slot* is a node of the current level that may still split (at least two rows, above max_depth);
// a child that cannot split is made a leaf by its parent and never takes a slot, so a level has at most n / 2 slots.
// One *round* advances every problem by one level with four launches:
//   split      a grid of (feature block x problem); a work-group walks the level's slots, each wave takes every fourth feature of the
//              block.  A node of more than 64 rows builds the 256-bin histogram of (sum q, count) per (node, feature) in the wave's own LDS
//              with integer atomic adds (64-bit for sum q: one ds_add_u64, checked in the compiled code -- not a compare-and-swap loop),
//              then every lane scans four bins behind a wave prefix sum and scores their boundaries.  A node of at most 64 rows holds one
//              row per lane and counts lane against lane: what lies in bins <= its own, in m steps instead of a pass over 256 bins (deep
//              levels are hundreds of nodes of 2-5 rows).  Both forms add the same integers, so they give the same bits.  One candidate
//              (gain, feature, bin, Q_L, m_L) per (slot, feature block) is written; nothing is zero-filled, no float atomics
//   choose     one work-group per problem: the best candidate per slot over the feature blocks, the stop rule (gain > 1e-6, gain >= gamma),
//              the node's arrays, the children's ids (the next two ids per split, slots in ascending id), their slots or their leaves
//   partition  a wave per slot: the row list of the slot's segment, stably, by bin <= split bin; the rows of new leaves get their leaf's value
//   update     one work-group per problem: a level more; or, behind a finished tree, margin += value[leaf] in float32, then the next
//              tree's gradients: g, max |g| (a maximum has no order), k, q and the root's Q (an integer sum)
// The depth a tree reaches is not known in advance: every problem keeps its own (tree, level) on the device and a kernel leaves at once for
// a problem that has nothing to do in it.  Rounds are enqueued in blocks of XGB_BLOCK_ROUNDS, then one word is read that says whether any
// problem still grows (as rf.hip does); nothing else is read by the host before the result.
// Every index read from memory is kept inside its array (row_of, and the checks beside each store); a wrong one sets the problem's error
// word, which the fit reports as tree_nodes[t] = -1.
#include "common.h"
#include "bbbp_hip.h"
#include "tree_fit.h"

#include <math.h>

namespace {

constexpr int XGB_BLOCK_ROUNDS = 16;          // rounds enqueued between two reads of the `alive` word
constexpr int XGB_SMALL = 64;                 // nodes of at most this many rows take the lane-against-lane form
constexpr double XGB_RT_EPS = 1e-6;           // XGBoost's kRtEps: the smallest gain that splits
constexpr int XGB_NO_FEATURE = 0x7fffffff;

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
    size_t rows[2], q, leaf_value, tab_start[2], tab_cnt[2], tab_node[2], tab_q[2], s_feature, s_bin, s_mleft, s_flags, s_lval, s_rval, cand_gain, cand_q,
        cand_fb, cand_m, state, total;
};
__host__ __device__ inline Work work_layout(int n, int d) {
    Work w;
    Area a;
    const size_t S = (size_t)slot_capacity(n), C = S * (size_t)feature_blocks(d);
    w.rows[0] = a.take((size_t)n * 4); w.rows[1] = a.take((size_t)n * 4);
    w.q = a.take((size_t)n * 8);
    w.leaf_value = a.take((size_t)n * 4);
    w.tab_start[0] = a.take(S * 4); w.tab_start[1] = a.take(S * 4);
    w.tab_cnt[0] = a.take(S * 4); w.tab_cnt[1] = a.take(S * 4);
    w.tab_node[0] = a.take(S * 4); w.tab_node[1] = a.take(S * 4);
    w.tab_q[0] = a.take(S * 8); w.tab_q[1] = a.take(S * 8);
    w.s_feature = a.take(S * 4); w.s_bin = a.take(S * 4); w.s_mleft = a.take(S * 4); w.s_flags = a.take(S * 4);
    w.s_lval = a.take(S * 4); w.s_rval = a.take(S * 4);
    w.cand_gain = a.take(C * 8); w.cand_q = a.take(C * 8); w.cand_fb = a.take(C * 4); w.cand_m = a.take(C * 4);
    w.state = a.take(sizeof(State));
    w.total = a.at;
    return w;
}

struct Tab { int *start, *cnt, *node; long long* q; };       // the slots of one level
struct View {                                 // a problem's work area, typed
    int *rows_a, *rows_b; long long* q; float* leaf_value; Tab tab_a, tab_b;
    int *s_feature, *s_bin, *s_mleft, *s_flags; float *s_lval, *s_rval;
    double* cand_gain; long long* cand_q; int *cand_fb, *cand_m; State* st;
};
__device__ inline View view_of(const bbbp_xgb_problem& p) {
    const Work w = work_layout(p.n, p.d);
    char* b = static_cast<char*>(p.work);
    View v;
    v.rows_a = (int*)(b + w.rows[0]); v.rows_b = (int*)(b + w.rows[1]);
    v.q = (long long*)(b + w.q); v.leaf_value = (float*)(b + w.leaf_value);
    v.tab_a = Tab{(int*)(b + w.tab_start[0]), (int*)(b + w.tab_cnt[0]), (int*)(b + w.tab_node[0]), (long long*)(b + w.tab_q[0])};
    v.tab_b = Tab{(int*)(b + w.tab_start[1]), (int*)(b + w.tab_cnt[1]), (int*)(b + w.tab_node[1]), (long long*)(b + w.tab_q[1])};
    v.s_feature = (int*)(b + w.s_feature); v.s_bin = (int*)(b + w.s_bin); v.s_mleft = (int*)(b + w.s_mleft); v.s_flags = (int*)(b + w.s_flags);
    v.s_lval = (float*)(b + w.s_lval); v.s_rval = (float*)(b + w.s_rval);
    v.cand_gain = (double*)(b + w.cand_gain); v.cand_q = (long long*)(b + w.cand_q); v.cand_fb = (int*)(b + w.cand_fb); v.cand_m = (int*)(b + w.cand_m);
    v.st = (State*)(b + w.state);
    return v;
}
// selects, not indexed arrays: no scratch.  Level L reads rows_of(L) and tab_of(L); partition and choose write those of L + 1
__device__ inline int* rows_of(const View& v, int level) { return (level & 1) ? v.rows_b : v.rows_a; }
__device__ inline Tab tab_of(const View& v, int level) {
    const bool b = level & 1;
    return Tab{b ? v.tab_b.start : v.tab_a.start, b ? v.tab_b.cnt : v.tab_a.cnt, b ? v.tab_b.node : v.tab_a.node, b ? v.tab_b.q : v.tab_a.q};
}
__device__ inline bool problem_idle(const bbbp_xgb_problem& p, const State* st) { return st->tree >= p.n_estimators; }

// ---- the score ----------------------------------------------------------------------------------------------------------------------
__device__ inline double to_G(long long Q, int k) { return ldexp((double)Q, -k); }          // one rounding, then an exact scaling
__device__ inline double score_term(double G, double H, double lambda) { return G * G / (H + lambda); }
__device__ inline double node_weight(double G, double H, double lambda) { return -G / (H + lambda); }
__device__ inline float leaf_value_of(double w, float learning_rate) { return (float)((double)learning_rate * w); }

struct Best { double gain; long long q_left; int feature, bin, m_left; };
__device__ inline Best no_candidate() { return Best{-INFINITY, 0, XGB_NO_FEATURE, 0, 0}; }
// the tie rule: the larger gain, among equal gains the lowest feature, then the lowest bin
__device__ inline bool better(const Best& a, const Best& b) {
    return a.gain > b.gain || (a.gain == b.gain && (a.feature < b.feature || (a.feature == b.feature && a.bin < b.bin)));
}
__device__ inline void offer(Best& best, long long q_left, int m_left, long long Q, int m, int k, double lambda, double parent_term, int feature, int bin) {
    const double gain = (score_term(to_G(q_left, k), (double)m_left, lambda) + score_term(to_G(Q - q_left, k), (double)(m - m_left), lambda)) - parent_term;
    const Best c{gain, q_left, feature, bin, m_left};
    if (better(c, best)) best = c;
}
__device__ inline Best wave_best(Best b) {
    for (int off = 32; off >= 1; off >>= 1) {
        const Best o{__shfl_xor(b.gain, off), __shfl_xor(b.q_left, off), __shfl_xor(b.feature, off), __shfl_xor(b.bin, off), __shfl_xor(b.m_left, off)};
        if (better(o, b)) b = o;
    }
    return b;
}
__device__ inline long long readlane64(long long x, int lane) {         // `lane` is uniform over the wave
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned long long)x, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)((unsigned long long)x >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// ---- bin: bin(x) = the number of the feature's cuts <= x ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xgb_bin_kernel(const float* XT, int n, int d, const float* cuts, int cut_stride, uint8_t* bins) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * d) return;
    const float x = XT[i];
    const float* c = cuts + (i / n) * cut_stride;
    int lo = 0, hi = cut_stride;                                // the row is padded with +infinity behind the feature's cuts
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= x) lo = mid + 1; else hi = mid;
    }
    bins[i] = (uint8_t)lo;
}

// ---- grad: a tree's gradients and its root (one work-group of 1024 threads per problem; every thread calls it) -------------------------
__device__ inline void start_tree(const bbbp_xgb_problem& p, const View& v) {
    __shared__ float red_f[1024];
    __shared__ long long red_q[1024];
    const int tid = threadIdx.x;
    float gmax = 0.f;
    for (int i = tid; i < p.n; i += 1024) gmax = fmaxf(gmax, fabsf(p.margin[i] - p.y[i]));
    red_f[tid] = gmax;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) red_f[tid] = fmaxf(red_f[tid], red_f[tid + w]);
        __syncthreads();
    }
    gmax = red_f[0];
    const int k = gmax == 0.f ? 0 : 47 - ilogb((double)gmax);
    long long sum = 0;
    for (int i = tid; i < p.n; i += 1024) {
        const float g = p.margin[i] - p.y[i];
        const long long q = llrint(ldexp((double)g, k));        // the product is exact: g has 24 bits below 2^(ilogb + 1)
        v.q[i] = q;
        v.rows_a[i] = i;
        sum += q;
    }
    red_q[tid] = sum;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) red_q[tid] += red_q[tid + w];              // integers: the order of the additions cannot change a bit
        __syncthreads();
    }
    if (tid == 0) {
        v.tab_a.start[0] = 0; v.tab_a.cnt[0] = p.n; v.tab_a.node[0] = 0; v.tab_a.q[0] = red_q[0];
        v.st->level = 0; v.st->n_slots = 1; v.st->n_next = 0; v.st->n_nodes = 1; v.st->final = 0; v.st->k = k;
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void xgb_init_kernel(const bbbp_xgb_problem* problems) {
    const bbbp_xgb_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    for (int i = threadIdx.x; i < p.n; i += 1024) p.margin[i] = p.base_score;      // the same thread reads it back in start_tree
    if (threadIdx.x == 0) { v.st->tree = 0; v.st->error = 0; }
    start_tree(p, v);
}

// ---- split: the best boundary per (slot, feature block) -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xgb_split_kernel(const bbbp_xgb_problem* problems) {
    const bbbp_xgb_problem p = problems[blockIdx.y];
    const View v = view_of(p);
    if (problem_idle(p, v.st)) return;
    const int fpb = features_per_block(p.d), f0 = blockIdx.x * fpb;
    if (f0 >= p.d) return;                                      // the grid is sized for the widest problem of the batch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = p.n;
    const int level = v.st->level, n_slots = v.st->n_slots, k = v.st->k, mc = p.min_child_rows;
    const Tab tab = tab_of(v, level);
    const int* src = rows_of(v, level);
    const double lambda = p.reg_lambda;
    const long S = slot_capacity(n);
    __shared__ unsigned long long hist_q[4][256];               // a wave's own histogram: only its lanes touch it
    __shared__ int hist_c[4][256];
    __shared__ double wb_gain[2][4];
    __shared__ long long wb_q[2][4];
    __shared__ int wb_feature[2][4], wb_bin[2][4], wb_m[2][4];
    for (int s = 0; s < n_slots && s < S; ++s) {
        const int start = tab.start[s];
        int m = tab.cnt[s];
        if (start < 0 || m < 0 || start > n - m) { v.st->error = 1; m = 0; }
        const long long Q = tab.q[s];
        const double parent_term = score_term(to_G(Q, k), (double)m, lambda);
        Best best = no_candidate();
        if (m <= XGB_SMALL) {                                   // one row per lane, counted lane against lane
            int row = 0;
            long long q_own = 0;
            if (lane < m) { row = row_of(src, start + lane, n, v.st); q_own = v.q[row]; }
            for (int f = f0 + wave; f < f0 + fpb && f < p.d; f += 4) {
                const int b = lane < m ? p.bins[(long)f * n + row] : 256;
                long long q_left = 0;
                int m_left = 0;
                for (int r = 0; r < m; ++r) {
                    const int b_r = __builtin_amdgcn_readlane(b, r);
                    const long long q_r = readlane64(q_own, r);
                    if (b_r <= b) { q_left += q_r; ++m_left; }
                }
                if (lane < m && m_left >= mc && m - m_left >= mc) offer(best, q_left, m_left, Q, m, k, lambda, parent_term, f, b);
            }
        } else {                                                // the 256-bin histogram of (sum q, count), four bins per lane
            for (int j = 0; j < fpb; j += 4) {                  // the same trip count in every wave: the barriers are the group's
                const int f = f0 + j + wave;
                const bool live = f < p.d;
                for (int t = 0; t < 4; ++t) { hist_q[wave][4 * lane + t] = 0ull; hist_c[wave][4 * lane + t] = 0; }
                __syncthreads();
                if (live)
                    for (int pos = lane; pos < m; pos += 64) {
                        const int row = row_of(src, start + pos, n, v.st);
                        const int b = p.bins[(long)f * n + row];
                        atomicAdd(&hist_q[wave][b], (unsigned long long)v.q[row]);
                        atomicAdd(&hist_c[wave][b], 1);
                    }
                __syncthreads();
                if (live) {
                    long long q4[4];
                    int c4[4];
                    long long q_run = 0;
                    int c_run = 0;
                    for (int t = 0; t < 4; ++t) {
                        q_run += (long long)hist_q[wave][4 * lane + t]; c_run += hist_c[wave][4 * lane + t];
                        q4[t] = q_run; c4[t] = c_run;
                    }
                    long long q_incl = q_run;
                    int c_incl = c_run;
                    for (int off = 1; off < 64; off <<= 1) {
                        const long long pq = __shfl_up(q_incl, off);
                        const int pc = __shfl_up(c_incl, off);
                        if (lane >= off) { q_incl += pq; c_incl += pc; }
                    }
                    const long long q_before = q_incl - q_run;
                    const int c_before = c_incl - c_run;
                    for (int t = 0; t < 4; ++t) {
                        const int m_left = c_before + c4[t];
                        if (m_left >= mc && m - m_left >= mc) offer(best, q_before + q4[t], m_left, Q, m, k, lambda, parent_term, f, 4 * lane + t);
                    }
                }
            }
        }
        best = wave_best(best);
        const int par = s & 1;                                  // two rows: a wave writes the next slot's while thread 0 still reads this one's
        if (lane == 0) { wb_gain[par][wave] = best.gain; wb_q[par][wave] = best.q_left; wb_feature[par][wave] = best.feature; wb_bin[par][wave] = best.bin; wb_m[par][wave] = best.m_left; }
        __syncthreads();
        if (tid == 0) {
            Best all = no_candidate();
            for (int w = 0; w < 4; ++w) {
                const Best c{wb_gain[par][w], wb_q[par][w], wb_feature[par][w], wb_bin[par][w], wb_m[par][w]};
                if (better(c, all)) all = c;
            }
            const long at = (long)blockIdx.x * S + s;
            v.cand_gain[at] = all.gain; v.cand_q[at] = all.q_left; v.cand_m[at] = all.m_left;
            v.cand_fb[at] = all.feature == XGB_NO_FEATURE ? -1 : all.feature * 256 + all.bin;
        }
    }
}

// ---- choose: the best candidate per slot, the stop rule, the node's arrays, the children ----------------------------------------------
__device__ inline void store_leaf(const bbbp_xgb_problem& p, long node, float value, int m) {
    p.left[node] = -1; p.right[node] = -1; p.feature[node] = 0; p.cond[node] = value;
    p.base_weight[node] = value; p.loss_change[node] = 0.f; p.sum_hessian[node] = (float)m;
}

__global__ __launch_bounds__(256) void xgb_choose_kernel(const bbbp_xgb_problem* problems) {
    const bbbp_xgb_problem p = problems[blockIdx.x];
    const View v = view_of(p);
    if (problem_idle(p, v.st)) return;
    const int tid = threadIdx.x, n = p.n;
    const int level = v.st->level, n_slots = v.st->n_slots, n_nodes = v.st->n_nodes, k = v.st->k, mc = p.min_child_rows;
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
                const Best c{v.cand_gain[at], v.cand_q[at], fb >> 8, fb & 255, v.cand_m[at]};
                if (better(c, best)) best = c;
            }
        const int start = in ? tab.start[s] : 0, m = in ? tab.cnt[s] : 0, node = in ? tab.node[s] : 0;
        const long long Q = in ? tab.q[s] : 0;
        bool split = in && best.feature != XGB_NO_FEATURE && best.gain > XGB_RT_EPS && best.gain >= p.gamma;
        if (split && (best.feature >= p.d || best.bin >= p.cut_stride || best.m_left < 1 || best.m_left >= m)) { v.st->error = 1; split = false; }
        const int m_l = best.m_left, m_r = m - best.m_left;
        const bool slot_l = split && deeper && m_l >= 2 * mc, slot_r = split && deeper && m_r >= 2 * mc;
        const int rank = block_rank_before(split, wave_cnt[0][it & 1], splits);
        const int lefts_before = block_rank_before(slot_l, wave_cnt[1][it & 1], next_left);
        const int at_l = lefts_before + block_rank_before(slot_r, wave_cnt[2][it & 1], next_right);      // slots in ascending node id
        if (!in) continue;
        if ((unsigned)node >= (unsigned)cap) { v.st->error = 1; continue; }
        const double w = node_weight(to_G(Q, k), (double)m, lambda);
        if (!split) {                                           // a leaf: its rows get the value in `partition`
            const float value = leaf_value_of(w, p.learning_rate);
            store_leaf(p, base + node, value, m);
            v.s_feature[s] = -1; v.s_lval[s] = value;
            continue;
        }
        const int lc = n_nodes + 2 * rank, rc = lc + 1;
        if (rc >= cap || at_l + (slot_l ? 1 : 0) + (slot_r ? 1 : 0) > S) {      // cannot happen: 2 n - 1 nodes and n / 2 slots are enough
            v.st->error = 1;
            store_leaf(p, base + node, 0.f, m);
            v.s_feature[s] = -1; v.s_lval[s] = 0.f;
            continue;
        }
        p.left[base + node] = lc; p.right[base + node] = rc; p.feature[base + node] = best.feature;
        p.cond[base + node] = p.cuts[(long)best.feature * p.cut_stride + best.bin];
        p.base_weight[base + node] = (float)w; p.loss_change[base + node] = (float)best.gain; p.sum_hessian[base + node] = (float)m;
        const float v_l = leaf_value_of(node_weight(to_G(best.q_left, k), (double)m_l, lambda), p.learning_rate);
        const float v_r = leaf_value_of(node_weight(to_G(Q - best.q_left, k), (double)m_r, lambda), p.learning_rate);
        v.s_feature[s] = best.feature; v.s_bin[s] = best.bin; v.s_mleft[s] = m_l;
        v.s_flags[s] = (slot_l ? 0 : 1) | (slot_r ? 0 : 2); v.s_lval[s] = v_l; v.s_rval[s] = v_r;
        if (slot_l) { next.start[at_l] = start; next.cnt[at_l] = m_l; next.node[at_l] = lc; next.q[at_l] = best.q_left; }
        else store_leaf(p, base + lc, v_l, m_l);
        const int at_r = at_l + (slot_l ? 1 : 0);
        if (slot_r) { next.start[at_r] = start + m_l; next.cnt[at_r] = m_r; next.node[at_r] = rc; next.q[at_r] = Q - best.q_left; }
        else store_leaf(p, base + rc, v_r, m_r);
    }
    __syncthreads();
    if (tid == 0) {
        v.st->n_nodes = n_nodes + 2 * splits;
        v.st->n_next = next_left + next_right;
        v.st->final = next_left + next_right == 0;
    }
}

// ---- partition: a slot's rows, stably, by bin <= split bin; the rows of new leaves take their leaf's value ------------------------------
__global__ __launch_bounds__(256) void xgb_partition_kernel(const bbbp_xgb_problem* problems) {
    const bbbp_xgb_problem p = problems[blockIdx.y];
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
__global__ __launch_bounds__(1024) void xgb_update_kernel(const bbbp_xgb_problem* problems, int* alive, int tell) {
    const bbbp_xgb_problem p = problems[blockIdx.x];
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
    start_tree(p, v);
    if (tid == 0 && tell) *alive = 1;
}

int check_problem(const bbbp_xgb_problem& p, int q) {
    BBBP_CHECK_ARG(p.n >= 2 && p.n <= BBBP_XGB_FIT_MAX_N, "xgb_fit: problem %d: n %d outside 2..%d", q, p.n, BBBP_XGB_FIT_MAX_N);
    BBBP_CHECK_ARG(p.d >= 1 && p.d <= BBBP_XGB_FIT_MAX_D, "xgb_fit: problem %d: d %d outside 1..%d", q, p.d, BBBP_XGB_FIT_MAX_D);
    BBBP_CHECK_ARG(p.cut_stride >= 1 && p.cut_stride <= 255, "xgb_fit: problem %d: cut_stride %d outside 1..255", q, p.cut_stride);
    BBBP_CHECK_ARG(p.n_estimators >= 1 && p.n_estimators <= BBBP_XGB_FIT_MAX_TREES, "xgb_fit: problem %d: n_estimators %d outside 1..%d", q, p.n_estimators,
                   BBBP_XGB_FIT_MAX_TREES);
    BBBP_CHECK_ARG(p.max_depth >= 1 && p.max_depth <= BBBP_XGB_FIT_MAX_DEPTH, "xgb_fit: problem %d: max_depth %d outside 1..%d", q, p.max_depth,
                   BBBP_XGB_FIT_MAX_DEPTH);
    BBBP_CHECK_ARG(p.min_child_rows >= 1, "xgb_fit: problem %d: min_child_rows %d must be >= 1", q, p.min_child_rows);
    BBBP_CHECK_ARG(p.reg_lambda >= 0.0 && p.reg_lambda < INFINITY, "xgb_fit: problem %d: reg_lambda must be finite and >= 0", q);
    BBBP_CHECK_ARG(p.gamma >= 0.0 && p.gamma < INFINITY, "xgb_fit: problem %d: gamma must be finite and >= 0", q);
    BBBP_CHECK_ARG(p.learning_rate > 0.f && p.learning_rate < INFINITY, "xgb_fit: problem %d: learning_rate must be positive and finite", q);
    BBBP_CHECK_ARG(p.base_score == p.base_score && fabsf(p.base_score) < INFINITY, "xgb_fit: problem %d: base_score must be finite", q);
    BBBP_CHECK_ARG((long)p.n_estimators * tree_capacity(p.n, p.max_depth) < (1L << 31), "xgb_fit: problem %d: %d trees of %d nodes exceed 32-bit node indices", q,
                   p.n_estimators, tree_capacity(p.n, p.max_depth));
    BBBP_CHECK_ARG(p.bins && p.cuts && p.y && p.work && p.left && p.right && p.feature && p.cond && p.base_weight && p.loss_change && p.sum_hessian &&
                       p.tree_nodes && p.margin, "xgb_fit: problem %d: null pointer", q);
    return BBBP_OK;
}

// tools/bench_xgb.py: with the profile on, every split launch of a fit sits between two events and the fit adds up their times
thread_local int g_profile = 0;
thread_local double g_split_ms = 0.0;
thread_local long g_launches = 0;

}  // namespace

extern "C" int bbbp_xgb_fit_profile(int enable) { const int prev = g_profile; g_profile = enable != 0; return prev; }

extern "C" int bbbp_xgb_fit_last(double* split_ms, long* launches) {
    BBBP_CHECK_ARG(split_ms && launches, "xgb_fit_last: null pointer");
    *split_ms = g_split_ms; *launches = g_launches;
    return BBBP_OK;
}

extern "C" int bbbp_xgb_fit_tree_capacity(int n, int max_depth) {
    if (n < 2 || n > BBBP_XGB_FIT_MAX_N || max_depth < 1 || max_depth > BBBP_XGB_FIT_MAX_DEPTH) {
        bbbp_set_error("xgb_fit_tree_capacity: n %d outside 2..%d or max_depth %d outside 1..%d", n, BBBP_XGB_FIT_MAX_N, max_depth, BBBP_XGB_FIT_MAX_DEPTH);
        return 0;
    }
    return tree_capacity(n, max_depth);
}

extern "C" size_t bbbp_xgb_fit_work_bytes(int n, int d) {
    if (n < 2 || n > BBBP_XGB_FIT_MAX_N || d < 1 || d > BBBP_XGB_FIT_MAX_D) {
        bbbp_set_error("xgb_fit_work_bytes: n %d outside 2..%d or d %d outside 1..%d", n, BBBP_XGB_FIT_MAX_N, d, BBBP_XGB_FIT_MAX_D);
        return 0;
    }
    return work_layout(n, d).total;
}

extern "C" int bbbp_xgb_bin(void* stream, const float* XT, int n, int d, const float* cuts, int cut_stride, uint8_t* bins) {
    BBBP_CHECK_ARG(n >= 1 && d >= 1 && (long)n * d < (1L << 40), "xgb_bin: n and d must be positive, got n %d d %d", n, d);
    BBBP_CHECK_ARG(cut_stride >= 1 && cut_stride <= 255, "xgb_bin: cut_stride %d outside 1..255 (bins are one byte)", cut_stride);
    BBBP_CHECK_ARG(XT && cuts && bins, "xgb_bin: null pointer");
    const long blocks = ((long)n * d + 255) / 256;
    BBBP_CHECK_ARG(blocks <= 0x7fffffffL, "xgb_bin: too many values");
    hipLaunchKernelGGL(xgb_bin_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), XT, n, d, cuts, cut_stride, bins);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_xgb_fit(void* stream, const bbbp_xgb_problem* problems, const bbbp_xgb_problem* problems_device, int n_problems, int* alive_device) {
    BBBP_CHECK_ARG(problems && problems_device && alive_device, "xgb_fit: null pointer");
    BBBP_CHECK_ARG(n_problems >= 1 && n_problems <= 65535, "xgb_fit: n_problems %d outside 1..65535", n_problems);
    int max_n = 0, max_d = 0;
    long rounds = 0;
    for (int q = 0; q < n_problems; ++q) {
        const bbbp_xgb_problem& p = problems[q];
        if (int rc = check_problem(p, q)) return rc;
        max_n = p.n > max_n ? p.n : max_n;
        max_d = p.d > max_d ? p.d : max_d;
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
    hipLaunchKernelGGL(xgb_init_kernel, one, dim3(1024), 0, st, problems_device);
    BBBP_CHECK_LAUNCH();
    hipEvent_t ev[2 * XGB_BLOCK_ROUNDS];
    const bool profile = g_profile != 0;
    if (profile)
        for (hipEvent_t& e : ev) BBBP_CHECK_HIP(hipEventCreate(&e));
    g_split_ms = 0.0; g_launches = 1;
    const long max_blocks = rounds / XGB_BLOCK_ROUNDS + 2;
    for (long b = 0; b < max_blocks; ++b) {
        BBBP_CHECK_HIP(hipMemsetAsync(alive_device, 0, sizeof(int), st));
        for (int r = 0; r < XGB_BLOCK_ROUNDS; ++r) {
            if (profile) BBBP_CHECK_HIP(hipEventRecord(ev[2 * r], st));
            hipLaunchKernelGGL(xgb_split_kernel, feats, dim3(256), 0, st, problems_device);
            if (profile) BBBP_CHECK_HIP(hipEventRecord(ev[2 * r + 1], st));
            hipLaunchKernelGGL(xgb_choose_kernel, one, dim3(256), 0, st, problems_device);
            hipLaunchKernelGGL(xgb_partition_kernel, slots, dim3(256), 0, st, problems_device);
            hipLaunchKernelGGL(xgb_update_kernel, one, dim3(1024), 0, st, problems_device, alive_device, r == XGB_BLOCK_ROUNDS - 1 ? 1 : 0);
            BBBP_CHECK_LAUNCH();
        }
        int alive = 0;                                          // the only host read before the result
        BBBP_CHECK_HIP(hipMemcpyAsync(&alive, alive_device, sizeof(int), hipMemcpyDeviceToHost, st));
        BBBP_CHECK_HIP(hipStreamSynchronize(st));
        g_launches += 4 * XGB_BLOCK_ROUNDS;
        if (profile)
            for (int r = 0; r < XGB_BLOCK_ROUNDS; ++r) {
                float ms = 0.f;
                BBBP_CHECK_HIP(hipEventElapsedTime(&ms, ev[2 * r], ev[2 * r + 1]));
                g_split_ms += ms;
            }
        if (!alive || b + 1 == max_blocks) {
            if (profile)
                for (hipEvent_t& e : ev) BBBP_CHECK_HIP(hipEventDestroy(e));
            if (!alive) return BBBP_OK;
        }
    }
    bbbp_set_error("xgb_fit: a problem still grows after %ld rounds", max_blocks * XGB_BLOCK_ROUNDS);
    return BBBP_ERR_HIP;
}
