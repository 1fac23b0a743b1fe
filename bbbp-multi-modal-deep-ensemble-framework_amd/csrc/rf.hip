// Random-forest classification trees, fitted on the GPU: RandomForestClassifier and DecisionTreeClassifier of the classification stack
// (Models/model_opt_maccs.py:124-200; two classes, Gini, bootstrap rows as integer weights, a feature subset per node), searched over
// n_estimators x max_depth x min_samples_split x min_samples_leaf.  scikit-learn's rules (ensemble/_forest.py, tree/_splitter.pyx,
// _criterion.pyx), restated: features are float32; a node of m distinct rows is a leaf at max_depth, below min_samples_split or
// 2 min_samples_leaf rows, when it is pure or when no drawn feature has a valid position; a position is valid between two values more than
// 1e-7f apart with min_samples_leaf rows on either side; the best position maximises (W_R L_1 - W_L R_1)^2 / (W_L W_R) over the node's drawn
// features, W the weight totals and L_1, R_1 the class-1 weights of the sides.  With n <= 8192 numerator and denominator are exact integers
// (below 2^53 and 2^26) and the score is one correctly rounded float64 division: no sum has an order, a tree is the same alone, in any
// batch and run to run, and a numpy restatement (tests/rf_numpy.py) reproduces it bit for bit.  Among equal scores the lowest feature
// wins, then the lowest position.
//
// Random numbers are one counter-based hash (rf_hash): a tree's key is hash(seed, tree), a child's key hash(parent's key, side); bootstrap
// draw j is hash(hash(key(root), RF_BOOT), j) mapped to [0, n) by multiply-high; a node's candidate features are the max_features features
// with the lowest hash(key, 2 + f) among those not constant in the node.  A subtree therefore depends on its rows, min_samples_leaf,
// max_features and its path alone: a tree grown under a larger min_samples_split or a smaller max_depth is the pruning of the unlimited one.
//
// A *tree* is one descriptor; many trees grow side by side, trees over one matrix share its column-major float32 copy and its presorted
// row order per feature.  Every feature's order is kept partitioned into the level's nodes, each segment sorted by that feature; a row
// carries the 16-bit slot of its node within the level (RF_DEAD once it sits in a leaf).  A level can hold thousands of nodes, so the node
// tables live in global memory.  `init` (three launches) draws the weights and compacts each order to the rows of positive weight.  One
// *round* grows one level of every tree with six launches:
//   stats      one wave per node: weight totals over the node's segment of feature 0's order, n_node_samples, value, the stop rules
//   draw       one wave per active node: which features are constant, their hash ranks, the drawn list and each (node, feature)'s place in it
//   split      one work-group per (feature, tree): a segmented integer scan of (weight, weight x class) packed in 32 bits over the
//              feature's order, the score at the valid positions of nodes that drew the feature, a segmented arg-max (lowest position among
//              equals), merged per (node, drawn feature) by the one thread at the segment's last position of the pass: no atomics
//   choose     one work-group per tree: arg-max over a node's drawn features, threshold, children numbered level by level, the next table
//   side       one thread per row: the slot at the next level
//   partition  one work-group per (feature, tree): every segment stably by side; rows of leaves stay where they are
// Depth is not known in advance: rounds are enqueued in blocks of RF_BLOCK_ROUNDS, then one word is read that says whether any tree still grows.
//
// Regression trees (RandomForestRegressor / DecisionTreeRegressor of the logBB stack, Models/multi_input_data_regression_opt_transformer_cnn_opt.py:
// 163-165; squared error) grow through the same rounds under a second criterion, chosen per launch by the kernels' template parameter.  The
// targets arrive as integers q (|q| <= 2^49, the host rounds y to a dyadic grid) held in float64.  A row carries its weight w and w q (int64);
// a node's S = sum w q (|S| <= 2^62) and W = sum w are exact integers, its value is (double)S / (double)W, its weight W goes to `value0`, and
// it is a leaf when min q == max q.  The score of a position is scikit-learn's proxy on those sums,
// (double)S_L (double)S_L / (double)W_L + (double)S_R (double)S_R / (double)W_R: two conversions, two products, two divisions and one add, each
// rounded to nearest and none contracted, so a regression fit has no summation order either (tests/rfr_numpy.py).  `init`, `stats` and `split`
// have a regression form; draw, choose, side and partition do not depend on the criterion.
#include "common.h"
#include "bbbp_hip.h"
#include "tree_fit.h"

#include <limits.h>
#include <math.h>
#include <type_traits>

namespace {

constexpr int RF_SCAN = 256;                  // positions per pass of the compact, split and partition kernels = their threads
constexpr int RF_BLOCK_ROUNDS = 8;            // levels enqueued between two reads of the `alive` word
constexpr unsigned RF_DEAD = 0xffffu;         // slot of a row that is in no node of the level
constexpr int NODE_LEAF = 0, NODE_ACTIVE = 1;
constexpr float RF_FEATURE_THRESHOLD = 1e-7f;
constexpr double RF_MAX_TARGET = 0x1p49;         // |q| of a regression target
constexpr unsigned long long RF_BOOT = 0xB007ull;          // the stream of a tree's bootstrap draws; features use 2 + f <= 1025, sides 0 and 1

// rf_hash: tree_fit.h (iforest.hip draws from the same hash)

struct TreeState { int level, nk, nk_prev, n_nodes, n_eff, done, active, error; };
struct Table { int *start, *cnt, *node; unsigned long long* key; };       // the nodes of one level, by slot
__host__ __device__ inline int tree_capacity(int n) { return 2 * n - 1; }

struct Work {                                 // offsets into a tree's `work`, in bytes; all multiples of 16
    size_t order[2], hist, wy, slot, tab_start[2], tab_cnt[2], tab_node[2], tab_key[2], flag, wtot, ndrawn, left_base, sp_rank, sp_feature, sp_thr,
        code, feat, cand_enc, cand_pos, state, total;
    size_t wq, w16, stot, total_regression;     // a regression tree's rows (w q, w) and node sums S follow the classifier's area: `total` stays
};
__host__ __device__ inline Work work_layout(int n, int d, int mf) {
    Work w;
    Area a;
    const size_t N = (size_t)n;
    w.order[0] = a.take((size_t)d * N * 2); w.order[1] = a.take((size_t)d * N * 2);
    w.hist = a.take(N * 4); w.wy = a.take(N * 4); w.slot = a.take(N * 2);
    w.tab_start[0] = a.take(N * 4); w.tab_cnt[0] = a.take(N * 4); w.tab_node[0] = a.take(N * 4); w.tab_key[0] = a.take(N * 8);      // no loop: an indexed
    w.tab_start[1] = a.take(N * 4); w.tab_cnt[1] = a.take(N * 4); w.tab_node[1] = a.take(N * 4); w.tab_key[1] = a.take(N * 8);      // member goes to scratch
    w.flag = a.take(N * 4); w.wtot = a.take(N * 4); w.ndrawn = a.take(N * 4); w.left_base = a.take(N * 4);
    w.sp_rank = a.take(N * 4); w.sp_feature = a.take(N * 4); w.sp_thr = a.take(N * 8);
    w.code = a.take(N * (size_t)d * 2); w.feat = a.take(N * (size_t)mf * 2);
    w.cand_enc = a.take(N * (size_t)mf * 8); w.cand_pos = a.take(N * (size_t)mf * 4);
    w.state = a.take(sizeof(TreeState));
    w.total = a.at;
    w.wq = a.take(N * 8); w.w16 = a.take(N * 2); w.stot = a.take(N * 8);
    w.total_regression = a.at;
    return w;
}

struct View {                                 // a tree's work area, typed
    uint16_t *order_a, *order_b; unsigned* hist; unsigned* wy; uint16_t* slot; Table tab_a, tab_b;
    int* flag; unsigned* wtot; int *ndrawn, *left_base, *sp_rank, *sp_feature; double* sp_thr;
    uint16_t *code, *feat; unsigned long long* cand_enc; int* cand_pos; TreeState* st;
    long long* wq; uint16_t* w16; long long* stot;          // inside `work` for a regression tree only; the Gini kernels never touch them
};
__device__ inline View view_of(const bbbp_rf_tree& c) {
    const Work w = work_layout(c.n, c.d, c.max_features);
    char* b = static_cast<char*>(c.work);
    View v;
    v.order_a = (uint16_t*)(b + w.order[0]); v.order_b = (uint16_t*)(b + w.order[1]);
    v.hist = (unsigned*)(b + w.hist); v.wy = (unsigned*)(b + w.wy); v.slot = (uint16_t*)(b + w.slot);
    v.tab_a = Table{(int*)(b + w.tab_start[0]), (int*)(b + w.tab_cnt[0]), (int*)(b + w.tab_node[0]), (unsigned long long*)(b + w.tab_key[0])};
    v.tab_b = Table{(int*)(b + w.tab_start[1]), (int*)(b + w.tab_cnt[1]), (int*)(b + w.tab_node[1]), (unsigned long long*)(b + w.tab_key[1])};
    v.flag = (int*)(b + w.flag); v.wtot = (unsigned*)(b + w.wtot); v.ndrawn = (int*)(b + w.ndrawn); v.left_base = (int*)(b + w.left_base);
    v.sp_rank = (int*)(b + w.sp_rank); v.sp_feature = (int*)(b + w.sp_feature); v.sp_thr = (double*)(b + w.sp_thr);
    v.code = (uint16_t*)(b + w.code); v.feat = (uint16_t*)(b + w.feat);
    v.cand_enc = (unsigned long long*)(b + w.cand_enc); v.cand_pos = (int*)(b + w.cand_pos);
    v.st = (TreeState*)(b + w.state);
    v.wq = (long long*)(b + w.wq); v.w16 = (uint16_t*)(b + w.w16); v.stot = (long long*)(b + w.stot);
    return v;
}
// Level L reads order buffer L & 1 and table L & 1; `partition` and `choose` write the other one
// (`c ? v.a : v.b` on members is a select between their addresses and would keep the whole view in scratch: select between copies)
template <class T> __device__ inline T pick(bool second, T a, T b) { return second ? b : a; }
__device__ inline uint16_t* order_of(const View& v, int level) { return pick(level & 1, v.order_a, v.order_b); }
__device__ inline Table table_of(const View& v, int level) {
    const bool b = level & 1;
    return Table{pick(b, v.tab_a.start, v.tab_b.start), pick(b, v.tab_a.cnt, v.tab_b.cnt), pick(b, v.tab_a.node, v.tab_b.node), pick(b, v.tab_a.key, v.tab_b.key)};
}
// row_of (tree_fit.h) sets the tree's error word, which `choose` reports as n_nodes = -1
// A node's segment, kept inside [0, n_eff): s >= 0, m >= 1, s + m <= n_eff, or the empty segment and the error word
__device__ inline void segment_of(const Table& tab, int k, int n_eff, TreeState* st, int& s, int& m) {
    s = tab.start[k]; m = tab.cnt[k];
    if (s < 0 || m < 1 || s > n_eff - m) { st->error = 1; s = 0; m = 0; }
}

// ---- the two criteria's sums: Gini's (weight, weight x class) packed in 32 bits, squared error's (sum of w q in 64 bits, weight) --------------
struct Sum64 { long long s; unsigned w; };
template <bool REG> using SumOf = std::conditional_t<REG, Sum64, unsigned>;
__device__ inline unsigned sum_add(unsigned a, unsigned b) { return a + b; }
__device__ inline Sum64 sum_add(Sum64 a, Sum64 b) { return Sum64{a.s + b.s, a.w + b.w}; }
__device__ inline unsigned sum_sub(unsigned a, unsigned b) { return a - b; }
__device__ inline Sum64 sum_sub(Sum64 a, Sum64 b) { return Sum64{a.s - b.s, a.w - b.w}; }
__device__ inline Sum64 lane_up(Sum64 v, int off) { return Sum64{__shfl_up(v.s, off), (unsigned)__shfl_up((int)v.w, off)}; }
// Gini: (W_R L_1 - W_L R_1)^2 / (W_L W_R); false when a side has no weight (cannot happen at a valid position)
__device__ inline bool score_of(unsigned tot, unsigned left, double& score) {
    const long long W = tot >> 16, W1 = tot & 0xffffu, WL = left >> 16, L1 = left & 0xffffu, WR = W - WL, R1 = W1 - L1;
    if (WL <= 0 || WR <= 0) return false;
    const long long diff = WR * L1 - WL * R1;                                          // |diff| <= 2^26: the square is exact in 64 bits and in a double
    score = (double)(diff * diff) / (double)(WL * WR);
    return true;
}
// squared error: S_L^2 / W_L + S_R^2 / W_R in float64, seven roundings and no contraction into fused multiply-adds
__device__ inline bool score_of(Sum64 tot, Sum64 left, double& score) {
#pragma clang fp contract(off)
    if (left.w == 0u || left.w >= tot.w) return false;
    const double SL = (double)left.s, SR = (double)(tot.s - left.s);
    const double l = SL * SL / (double)left.w, r = SR * SR / (double)(tot.w - left.w);
    score = l + r;
    return true;
}

// ---- init: weights, the compacted orders, the root --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rf_init_rows_kernel(const bbbp_rf_tree* trees) {
    const bbbp_rf_tree c = trees[blockIdx.y];
    const View v = view_of(c);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *v.st = TreeState{0, 0, 0, 0, 0, 0, 0, 0};
    if (i < c.n) v.hist[i] = c.bootstrap ? 0u : 1u;
}
__global__ __launch_bounds__(256) void rf_init_boot_kernel(const bbbp_rf_tree* trees) {
    const bbbp_rf_tree c = trees[blockIdx.y];
    if (!c.bootstrap) return;
    const View v = view_of(c);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= c.n) return;
    const unsigned long long stream = rf_hash(rf_hash(c.seed, (unsigned long long)c.tree_index), RF_BOOT);
    const unsigned i = (unsigned)__umul64hi(rf_hash(stream, (unsigned long long)j), (unsigned long long)c.n);      // < n
    atomicAdd(&v.hist[i < (unsigned)c.n ? i : 0u], 1u);     // integer counts: the histogram does not depend on the order of the adds
}
template <bool REG> __global__ __launch_bounds__(RF_SCAN) void rf_init_compact_kernel(const bbbp_rf_tree* trees) {
    const bbbp_rf_tree c = trees[blockIdx.y];
    const View v = view_of(c);
    const int f = blockIdx.x, tid = threadIdx.x, n = c.n;
    if (f >= c.d) return;                                   // the grid is sized for the widest tree of the batch
    __shared__ int wave_cnt[2][4];
    const int* src = c.order0 + (long)f * n;
    uint16_t* dst = v.order_a + (long)f * n;
    int before = 0;
    for (int base = 0, it = 0; base < n; base += RF_SCAN, ++it) {
        const int p = base + tid;
        int i = p < n ? src[p] : 0;
        if ((unsigned)i >= (unsigned)n) { v.st->error = 1; i = 0; }
        const bool keep = p < n && v.hist[i] > 0u;
        const int to = block_rank_before(keep, wave_cnt[it & 1], before);
        if (keep) dst[to] = (uint16_t)i;                    // to < n: it counts kept rows in front of p
    }
    if (f != 0) return;
    for (int i = tid; i < n; i += RF_SCAN) {
        const unsigned w = v.hist[i];
        if constexpr (REG) {
            double q = c.y[i];
            if (!(fabs(q) <= RF_MAX_TARGET)) { v.st->error = 1; q = 0.0; }           // NaN included: no conversion of a value outside int64
            v.wq[i] = (long long)w * (long long)q;          // w <= n <= 8192 = 2^13: |w q| <= 2^62, and so is every sum over a tree's rows
            v.w16[i] = (uint16_t)w;
        } else {
            const unsigned y1 = c.y[i] > 0.5 ? 1u : 0u;
            v.wy[i] = (w << 16) | (w * y1);                 // w <= n <= 8192: both halves stay below 2^16 in every partial sum
        }
        v.slot[i] = w ? (uint16_t)0 : (uint16_t)RF_DEAD;
    }
    if (tid == 0) {
        v.st->n_eff = before; v.st->nk = 1; v.st->n_nodes = 1;
        v.tab_a.start[0] = 0; v.tab_a.cnt[0] = before; v.tab_a.node[0] = 0;
        v.tab_a.key[0] = rf_hash(c.seed, (unsigned long long)c.tree_index);
    }
}

// ---- stats: the level's nodes: totals, n_node_samples, value, the stop rules ------------------------------------------------------------
template <bool REG> __global__ __launch_bounds__(256) void rf_stats_kernel(const bbbp_rf_tree* trees) {
    const bbbp_rf_tree c = trees[blockIdx.y];
    const View v = view_of(c);
    if (v.st->done) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int level = v.st->level, nk = min(v.st->nk, c.n), n_eff = min(v.st->n_eff, c.n), cap = tree_capacity(c.n);
    const Table tab = table_of(v, level);
    const uint16_t* src = order_of(v, level);               // feature 0's order: the nodes' segments are contiguous in it
    for (int k = blockIdx.x * 4 + wave; k < nk; k += gridDim.x * 4) {
        int s, m;
        segment_of(tab, k, n_eff, v.st, s, m);
        bool bad, pure;
        double value, value0;
        if constexpr (REG) {                                // S = sum w q, W = sum w, min q and max q over the node's rows; value = S / W, value0 = W
            long long S = 0, lo = LLONG_MAX, hi = LLONG_MIN;
            unsigned W = 0u;
            for (int p = lane; p < m; p += 64) {
                const int i = row_of(src, s + p, c.n, v.st);
                const unsigned w = v.w16[i];
                const long long wq = v.wq[i], q = w ? wq / (long long)w : 0;               // exact: wq is w times an integer
                S += wq; W += w;
                lo = q < lo ? q : lo; hi = q > hi ? q : hi;
            }
            for (int off = 32; off >= 1; off >>= 1) {
                S += __shfl_xor(S, off); W += (unsigned)__shfl_xor((int)W, off);
                const long long ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
                lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
            }
            if (lane != 0) continue;
            // scikit-learn's rule is impurity <= EPSILON; here a node is pure when all its targets are one integer (DESIGN.md compares the two)
            bad = W == 0u; pure = lo == hi;
            value = W ? (double)S / (double)W : 0.0; value0 = (double)W;
            v.wtot[k] = W; v.stot[k] = S;
        } else {
            unsigned acc = 0u;
            for (int p = lane; p < m; p += 64) acc += v.wy[row_of(src, s + p, c.n, v.st)];
            for (int off = 32; off >= 1; off >>= 1) acc += (unsigned)__shfl_xor((int)acc, off);
            if (lane != 0) continue;
            const unsigned W = acc >> 16, W1 = acc & 0xffffu;
            // scikit-learn's impurity <= EPSILON: with integer weights W <= 8192 the Gini impurity is 0 for a pure node and at least
            // (2 W - 2) / W^2 > 2.4e-4 otherwise
            bad = W == 0u || W1 > W; pure = W1 == 0u || W1 == W;
            value = W ? (double)W1 / (double)W : 0.0; value0 = W ? (double)(W - W1) / (double)W : 0.0;
            v.wtot[k] = acc;
        }
        int node = tab.node[k];
        if ((unsigned)node >= (unsigned)cap || bad) { v.st->error = 1; node = 0; }
        const bool leaf = level >= c.max_depth || m < c.min_samples_split || m < 2 * c.min_samples_leaf || pure;
        c.n_node_samples[node] = m;
        c.value[node] = value;
        c.value0[node] = value0;
        if (leaf) {
            v.flag[k] = NODE_LEAF;
            make_leaf(c, node);
        } else {
            v.flag[k] = NODE_ACTIVE;
            v.st->active = 1;                               // every writer stores the same 1; `choose` clears it for the next level
        }
    }
}

// ---- draw: an active node's candidate features ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rf_draw_kernel(const bbbp_rf_tree* trees) {
    const bbbp_rf_tree c = trees[blockIdx.y];
    const View v = view_of(c);
    if (v.st->done || !v.st->active) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = c.n, d = c.d, mf = c.max_features;
    const int level = v.st->level, nk = min(v.st->nk, n), n_eff = min(v.st->n_eff, n);
    const Table tab = table_of(v, level);
    const uint16_t* src = order_of(v, level);
    __shared__ unsigned long long sh[4][BBBP_RF_FIT_MAX_D];
    __shared__ uint8_t snc[4][BBBP_RF_FIT_MAX_D];
    unsigned long long* h = sh[wave];
    uint8_t* nc = snc[wave];
    for (int k0 = blockIdx.x * 4; k0 < nk; k0 += gridDim.x * 4) {          // the same trip count for the four waves: barriers inside
        const int k = k0 + wave;
        const bool on = k < nk && v.flag[k] == NODE_ACTIVE;
        int s = 0, m = 0;
        if (on) segment_of(tab, k, n_eff, v.st, s, m);
        const unsigned long long key = on ? tab.key[k] : 0ull;
        if (on && m > 0)
            for (int f = lane; f < d; f += 64) {
                const float* col = c.XT + (long)f * n;
                const uint16_t* of = src + (long)f * n;
                const float a = col[row_of(of, s, n, v.st)], b = col[row_of(of, s + m - 1, n, v.st)];
                nc[f] = b > a + RF_FEATURE_THRESHOLD ? 1 : 0;
                h[f] = rf_hash(key, 2ull + (unsigned long long)f);
            }
        __syncthreads();
        int drawn_before = 0;
        if (on && m > 0) {
            for (int f0 = 0; f0 < d; f0 += 64) {
                const int f = f0 + lane;
                bool drawn = false;
                if (f < d && nc[f]) {
                    const unsigned long long hf = h[f];
                    int rank = 0;
                    for (int g = 0; g < d; ++g) rank += (nc[g] && (h[g] < hf || (h[g] == hf && g < f))) ? 1 : 0;
                    drawn = rank < mf;
                }
                const unsigned long long ballot = __ballot(drawn);
                const int j = drawn_before + __popcll(ballot & ((1ull << lane) - 1ull));          // < mf: ranks are distinct
                if (f < d) v.code[(long)k * d + f] = (drawn && j < mf) ? (uint16_t)(j + 1) : (uint16_t)0;
                if (drawn && j < mf) {
                    v.feat[(long)k * mf + j] = (uint16_t)f;
                    v.cand_enc[(long)k * mf + j] = 0ull;
                    v.cand_pos[(long)k * mf + j] = 0;
                }
                drawn_before += __popcll(ballot);
            }
            if (lane == 0) v.ndrawn[k] = min(drawn_before, mf);
        }
        __syncthreads();
    }
}

// ---- split: the best (score, position) per (node, drawn feature) for one feature ----------------------------------------------------------
template <bool REG> __global__ __launch_bounds__(RF_SCAN) void rf_split_kernel(const bbbp_rf_tree* trees) {
    using Sum = SumOf<REG>;
    const bbbp_rf_tree c = trees[blockIdx.y];
    const View v = view_of(c);
    if (v.st->done || !v.st->active) return;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = c.n, d = c.d, mf = c.max_features;
    if (f >= d) return;                                     // the grid is sized for the widest tree of the batch
    const int level = v.st->level, nk = min(v.st->nk, n), n_eff = min(v.st->n_eff, n);
    const Table tab = table_of(v, level);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // staged rows.  Gini: [n] (weight, weight x class) in 32 bits, [n] slots.  Squared error: [n] w q in 64 bits, [n] w, [n] slots
    unsigned* swy = reinterpret_cast<unsigned*>(smem);
    long long* swq = reinterpret_cast<long long*>(smem);
    uint16_t* sw = reinterpret_cast<uint16_t*>(swq + n);
    uint16_t* sslot = REG ? sw + n : reinterpret_cast<uint16_t*>(swy + n);
    __shared__ Sum wave_val[4], carry_s;
    __shared__ int wave_flag[4], wave_pos[4];
    __shared__ unsigned long long wave_enc[4];
    for (int i = tid; i < n; i += RF_SCAN) {
        if constexpr (REG) { swq[i] = v.wq[i]; sw[i] = v.w16[i]; } else swy[i] = v.wy[i];
        sslot[i] = v.slot[i];
    }
    if (tid == 0) carry_s = Sum{};
    __syncthreads();
    const uint16_t* src = order_of(v, level) + (long)f * n;
    const float* col = c.XT + (long)f * n;
    const int msl = c.min_samples_leaf;
    for (int base = 0; base < n_eff; base += RF_SCAN) {
        const int p = base + tid;
        const bool in = p < n_eff;
        const int i = in ? row_of(src, p, n, v.st) : 0;
        const unsigned k = in ? sslot[i] : RF_DEAD;
        bool act = false;
        int s = 0, m = 0, j = 0;
        Sum wt{};
        if (k != RF_DEAD) {
            if (k >= (unsigned)nk) v.st->error = 1;
            else if (v.flag[k] == NODE_ACTIVE) {
                j = v.code[(long)k * d + f];
                if (j > mf) { v.st->error = 1; j = 0; }
                if (j > 0) { segment_of(tab, (int)k, n_eff, v.st, s, m); act = m > 0 && p >= s && p < s + m;
                             if constexpr (REG) wt = Sum64{v.stot[k], v.wtot[k]}; else wt = v.wtot[k]; }
            }
        }
        Sum x{};
        if (act) { if constexpr (REG) x = Sum64{swq[i], sw[i]}; else x = swy[i]; }
        const Sum carry = carry_s;                          // the inclusive sum at position base - 1, inside its segment
        // segmented inclusive scan inside the wave: a segment starts at its node's first position and at every position that is not scored
        const auto add = [](Sum a, Sum b) { return sum_add(a, b); };
        Sum val = x;
        int flg = (!act || p == s) ? 1 : 0;
        const int own = flg;
        wave_segmented_scan(val, flg, add);
        if (lane == 63) { wave_val[wave] = val; wave_flag[wave] = flg; }
        __syncthreads();
        if (!flg) val = sum_add(val, block_segment_prefix(carry, wave_val, wave_flag, add));
        if (tid == RF_SCAN - 1) carry_s = val;
        // the candidate between positions p - 1 and p
        unsigned long long enc = 0ull;
        if (act && p > s) {
            const int n_l = p - s, n_r = m - n_l;
            const float fv = col[i], fv_prev = col[row_of(src, p - 1, n, v.st)];
            if (fv > fv_prev + RF_FEATURE_THRESHOLD && n_l >= msl && n_r >= msl) {
                double score = 0.0;
                if (!score_of(wt, sum_sub(val, x), score)) v.st->error = 1;        // the exclusive sum: everything in front of p in the segment
                else enc = encode_score(score);
            }
        }
        // segmented arg-max with the same segments: the lowest position among equal scores
        int pos = p;
        flg = own;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long pe = (unsigned long long)__shfl_up((long long)enc, off);
            const int pp = __shfl_up(pos, off);
            const int pf = __shfl_up(flg, off);
            if (lane >= off) {
                if (!flg && pe != 0ull && pe >= enc) { enc = pe; pos = pp; }
                flg |= pf;
            }
        }
        if (lane == 63) { wave_enc[wave] = enc; wave_pos[wave] = pos; }
        __syncthreads();
        if (!flg) {
            unsigned long long be = 0ull;
            int bp = 0;
            for (int w = 0; w < wave; ++w) {
                if (wave_flag[w] || (wave_enc[w] != 0ull && wave_enc[w] > be)) { be = wave_enc[w]; bp = wave_pos[w]; }
            }
            if (be != 0ull && be >= enc) { enc = be; pos = bp; }
        }
        // the segment's last position of this pass merges into the (node, drawn feature) slot: one thread per slot and pass, passes in order
        if (act && enc != 0ull && (p + 1 == s + m || tid == RF_SCAN - 1)) {
            const long at = (long)k * mf + (j - 1);
            if (enc > v.cand_enc[at]) { v.cand_enc[at] = enc; v.cand_pos[at] = pos; }
        }
        __syncthreads();                                    // the next pass may merge into the same slot from another wave
    }
}
size_t split_lds_bytes(int n, bool regression) { return (size_t)n * (regression ? 12 : 6); }

// ---- choose: the best drawn feature per node, its threshold and children, the next level's table ---------------------------------------
__device__ inline void block_scan2(int& a, int& b, int* tmp, int tid) {       // inclusive sums over the 256 threads; tmp: [2][4] ints
    const int lane = tid & 63, wave = tid >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const int pa = __shfl_up(a, off), pb = __shfl_up(b, off);
        if (lane >= off) { a += pa; b += pb; }
    }
    __syncthreads();                                        // tmp may still be read from the previous call
    if (lane == 63) { tmp[wave] = a; tmp[4 + wave] = b; }
    __syncthreads();
    for (int w = 0; w < wave; ++w) { a += tmp[w]; b += tmp[4 + w]; }
}
__global__ __launch_bounds__(256) void rf_choose_kernel(const bbbp_rf_tree* trees, int* alive, int last_round) {
    const bbbp_rf_tree c = trees[blockIdx.x];
    const View v = view_of(c);
    const TreeState st = *v.st;
    if (st.done) return;
    const int tid = threadIdx.x, n = c.n, mf = c.max_features, cap = tree_capacity(n);
    __shared__ int tmp[8];
    __syncthreads();                                        // every thread holds the state before thread 0 rewrites it
    if (!st.active) {
        if (tid == 0) { v.st->done = 1; *c.n_nodes = st.error ? -1 : st.n_nodes; }
        return;
    }
    const int level = st.level, nk = min(st.nk, n), n_eff = min(st.n_eff, n);
    const Table tab = table_of(v, level), next = table_of(v, level + 1);
    int splits_before = 0, lefts_before = 0;
    for (int base = 0; base < nk; base += 256) {
        const int k = base + tid;
        const bool on = k < nk && v.flag[k] == NODE_ACTIVE;
        int s = 0, m = 0, bf = 0, bp = 0, node = 0;
        unsigned long long best = 0ull;
        if (on) {
            segment_of(tab, k, n_eff, v.st, s, m);
            node = tab.node[k];
            if ((unsigned)node >= (unsigned)cap) { v.st->error = 1; node = 0; }
            const int nd = min(v.ndrawn[k], mf);
            for (int j = 0; j < nd; ++j) {                  // features ascend with j: the lowest feature wins among equal scores
                const unsigned long long e = v.cand_enc[(long)k * mf + j];
                if (e > best) { best = e; bf = v.feat[(long)k * mf + j]; bp = v.cand_pos[(long)k * mf + j]; }
            }
            if (bf >= c.d) { v.st->error = 1; bf = 0; best = 0ull; }
        }
        const bool split = on && best != 0ull && bp > s && bp < s + m;
        const int n_left = split ? bp - s : 0;
        int rank = split ? 1 : 0, lefts = n_left;
        block_scan2(rank, lefts, tmp, tid);
        const int r = splits_before + rank - (split ? 1 : 0);
        if (split) {
            const uint16_t* src = order_of(v, level) + (long)bf * n;
            const float a = c.XT[(long)bf * n + row_of(src, bp - 1, n, v.st)], b = c.XT[(long)bf * n + row_of(src, bp, n, v.st)];
            const double thr = split_threshold(a, b);
            const int lc = st.n_nodes + 2 * r, rc = lc + 1;
            if (rc >= cap || 2 * r + 1 >= n) { v.st->error = 1; v.sp_rank[k] = -1; }      // cannot happen: a level's nodes are non-empty and disjoint
            else {
                c.left[node] = lc; c.right[node] = rc; c.feature[node] = bf; c.threshold[node] = thr;
                v.sp_rank[k] = r; v.sp_feature[k] = bf; v.sp_thr[k] = thr;
                v.left_base[r] = lefts_before + lefts - n_left;          // rows that go left in the segments in front of this one
                const unsigned long long key = tab.key[k];
                next.start[2 * r] = s; next.cnt[2 * r] = n_left; next.node[2 * r] = lc; next.key[2 * r] = rf_hash(key, 0ull);
                next.start[2 * r + 1] = s + n_left; next.cnt[2 * r + 1] = m - n_left; next.node[2 * r + 1] = rc; next.key[2 * r + 1] = rf_hash(key, 1ull);
            }
        } else if (k < nk) {
            v.sp_rank[k] = -1;
            if (on) make_leaf(c, node);                     // no valid split: a leaf after all
        }
        // the running totals: the last thread's inclusive sums
        __syncthreads();
        if (tid == 255) { tmp[0] = rank; tmp[4] = lefts; }
        __syncthreads();
        splits_before += tmp[0]; lefts_before += tmp[4];
    }
    __syncthreads();
    if (tid == 0) {
        const int error = v.st->error;
        if (splits_before == 0 || error) {
            v.st->done = 1;
            *c.n_nodes = error ? -1 : st.n_nodes;
        } else {
            v.st->level = level + 1; v.st->nk_prev = nk; v.st->nk = 2 * splits_before; v.st->n_nodes = st.n_nodes + 2 * splits_before; v.st->active = 0;
            if (last_round) *alive = 1;
        }
    }
}

// ---- side: every row's slot at the next level ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rf_side_kernel(const bbbp_rf_tree* trees) {
    const bbbp_rf_tree c = trees[blockIdx.y];
    const View v = view_of(c);
    if (v.st->done) return;                                 // `choose` has moved the state on to the next level
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const unsigned k = v.slot[i];
    if (k == RF_DEAD) return;
    if (k >= (unsigned)min(v.st->nk_prev, c.n)) { v.st->error = 1; v.slot[i] = (uint16_t)RF_DEAD; return; }
    const int r = v.sp_rank[k];
    if (r < 0) { v.slot[i] = (uint16_t)RF_DEAD; return; }
    int bf = v.sp_feature[k];
    if ((unsigned)bf >= (unsigned)c.d) { v.st->error = 1; bf = 0; }
    const int side = ((double)c.XT[(long)bf * c.n + i] <= v.sp_thr[k]) ? 0 : 1;
    v.slot[i] = (uint16_t)(2 * r + side);
}

// ---- partition: every feature's order, stably, by side inside each split segment -----------------------------------------------------------
__global__ __launch_bounds__(RF_SCAN) void rf_partition_kernel(const bbbp_rf_tree* trees) {
    const bbbp_rf_tree c = trees[blockIdx.y];
    const View v = view_of(c);
    if (v.st->done) return;
    const int f = blockIdx.x, tid = threadIdx.x, n = c.n;
    if (f >= c.d) return;                                   // the grid is sized for the widest tree of the batch
    const int level = v.st->level - 1, nk_new = min(v.st->nk, n), n_eff = min(v.st->n_eff, n);
    if (level < 0) return;
    const Table next = table_of(v, level + 1);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t* sslot = reinterpret_cast<uint16_t*>(smem);              // [n] new slots
    __shared__ int wave_cnt[2][4];
    for (int i = tid; i < n; i += RF_SCAN) sslot[i] = v.slot[i];
    __syncthreads();
    const uint16_t* src = order_of(v, level) + (long)f * n;
    uint16_t* dst = order_of(v, level + 1) + (long)f * n;
    int before = 0;                                                   // rows going left in front of this pass
    for (int base = 0, it = 0; base < n_eff; base += RF_SCAN, ++it) {
        const int p = base + tid;
        const bool in = p < n_eff;
        const int i = in ? row_of(src, p, n, v.st) : 0;
        unsigned cs = in ? sslot[i] : RF_DEAD;
        if (cs != RF_DEAD && cs >= (unsigned)nk_new) { v.st->error = 1; cs = RF_DEAD; }
        const bool moving = cs != RF_DEAD, left = moving && !(cs & 1u);
        const int lefts = block_rank_before(left, wave_cnt[it & 1], before);
        if (in) {
            int to = p;                                               // a row of a leaf stays where it is
            if (moving) {
                const int r = (int)(cs >> 1), s = next.start[2 * r], nl = next.cnt[2 * r];
                const int in_seg = lefts - v.left_base[r];            // rows of this segment going left in front of p
                to = left ? s + in_seg : s + nl + (p - s - in_seg);
            }
            if ((unsigned)to < (unsigned)n_eff) dst[to] = (uint16_t)i;
            else v.st->error = 1;
        }
    }
}
size_t partition_lds_bytes(int n) { return (size_t)n * 2; }

// ---- predict: class probabilities of query rows from a forest, optionally pruned by limits ------------------------------------------------
struct PredictArgs {
    const float* X; long ld; int m, d;
    const int *left, *right, *feature; const double *threshold, *p0, *p1; const int *n_node_samples, *root;
    int n_trees, max_depth, min_samples_split; double* out;
};
template <bool MEAN> __global__ __launch_bounds__(256) void rf_predict_kernel(PredictArgs a) {         // MEAN: one value per node (p1), out [m]
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const float* x = a.X + (long)i * a.ld;
    double s0 = 0.0, s1 = 0.0;
    for (int t = 0; t < a.n_trees; ++t) {
        int node = a.root[t], depth = 0;
        int l = a.left[node];
        // bounded: arrays handed to the C ABI directly cannot spin a wave for ever
        while (l >= 0 && depth < a.max_depth && a.n_node_samples[node] >= a.min_samples_split && depth < BBBP_RF_MAX_WALK) {
            node = (double)x[a.feature[node]] <= a.threshold[node] ? l : a.right[node];
            l = a.left[node];
            ++depth;
        }
        const bool lost = l >= 0 && depth >= BBBP_RF_MAX_WALK && depth < a.max_depth;
        if constexpr (!MEAN) s0 = lost ? __builtin_nan("") : s0 + a.p0[node];          // scikit-learn's forest: the trees' outputs summed in tree order
        s1 = lost ? __builtin_nan("") : s1 + a.p1[node];
    }
    if constexpr (MEAN) a.out[i] = s1 / (double)a.n_trees;
    else {
        a.out[2 * (long)i] = s0 / (double)a.n_trees;
        a.out[2 * (long)i + 1] = s1 / (double)a.n_trees;
    }
}

int check_tree(const bbbp_rf_tree& c, int q) {
    BBBP_CHECK_ARG(c.n >= 2 && c.d >= 1, "rf_fit: tree %d: n >= 2 and d >= 1 must hold, got n %d d %d", q, c.n, c.d);
    BBBP_CHECK_ARG(c.n <= BBBP_RF_FIT_MAX_N, "rf_fit: tree %d: n %d exceeds BBBP_RF_FIT_MAX_N %d", q, c.n, BBBP_RF_FIT_MAX_N);
    BBBP_CHECK_ARG(c.d <= BBBP_RF_FIT_MAX_D, "rf_fit: tree %d: d %d exceeds BBBP_RF_FIT_MAX_D %d", q, c.d, BBBP_RF_FIT_MAX_D);
    BBBP_CHECK_ARG(c.max_depth >= 1, "rf_fit: tree %d: max_depth %d must be >= 1", q, c.max_depth);
    BBBP_CHECK_ARG(c.min_samples_split >= 2, "rf_fit: tree %d: min_samples_split %d must be >= 2", q, c.min_samples_split);
    BBBP_CHECK_ARG(c.min_samples_leaf >= 1, "rf_fit: tree %d: min_samples_leaf %d must be >= 1", q, c.min_samples_leaf);
    BBBP_CHECK_ARG(c.max_features >= 1 && c.max_features <= c.d, "rf_fit: tree %d: max_features %d outside 1..d = %d", q, c.max_features, c.d);
    BBBP_CHECK_ARG(c.tree_index >= 0, "rf_fit: tree %d: tree_index %d must be >= 0", q, c.tree_index);
    BBBP_CHECK_ARG(c.XT && c.order0 && c.y && c.work && c.left && c.right && c.feature && c.n_node_samples && c.threshold && c.value && c.value0 &&
                       c.n_nodes, "rf_fit: tree %d: null pointer", q);
    return BBBP_OK;
}

}  // namespace

extern "C" int bbbp_rf_fit_tree_capacity(int n) {
    if (n < 2 || n > BBBP_RF_FIT_MAX_N) {
        bbbp_set_error("rf_fit_tree_capacity: n %d outside 2..%d", n, BBBP_RF_FIT_MAX_N);
        return 0;
    }
    return tree_capacity(n);
}

namespace {
bool check_work_shape(const char* who, int n, int d, int max_features) {
    if (n < 2 || d < 1) { bbbp_set_error("%s: n >= 2 and d >= 1 must hold, got n %d d %d", who, n, d); return false; }
    if (n > BBBP_RF_FIT_MAX_N) { bbbp_set_error("%s: n %d exceeds BBBP_RF_FIT_MAX_N %d", who, n, BBBP_RF_FIT_MAX_N); return false; }
    if (d > BBBP_RF_FIT_MAX_D) { bbbp_set_error("%s: d %d exceeds BBBP_RF_FIT_MAX_D %d", who, d, BBBP_RF_FIT_MAX_D); return false; }
    if (max_features < 1 || max_features > d) { bbbp_set_error("%s: max_features %d outside 1..d = %d", who, max_features, d); return false; }
    return true;
}
}  // namespace

extern "C" size_t bbbp_rf_fit_work_bytes(int n, int d, int max_features) {
    return check_work_shape("rf_fit_work_bytes", n, d, max_features) ? work_layout(n, d, max_features).total : 0;
}

extern "C" size_t bbbp_rf_fit_regression_work_bytes(int n, int d, int max_features) {
    return check_work_shape("rf_fit_regression_work_bytes", n, d, max_features) ? work_layout(n, d, max_features).total_regression : 0;
}

extern "C" unsigned long long bbbp_rf_hash(unsigned long long a, unsigned long long b) { return rf_hash(a, b); }

namespace {
template <bool REG> int fit_trees(void* stream, const bbbp_rf_tree* trees, const bbbp_rf_tree* trees_device, int n_trees, int* alive_device) {
    BBBP_CHECK_ARG(trees && trees_device && alive_device, "rf_fit: null pointer");
    BBBP_CHECK_ARG(n_trees >= 1 && n_trees <= 65535, "rf_fit: n_trees %d outside 1..65535", n_trees);
    int max_n = 0, max_d = 0;
    for (int q = 0; q < n_trees; ++q) {
        if (int rc = check_tree(trees[q], q)) return rc;
        max_n = trees[q].n > max_n ? trees[q].n : max_n;
        max_d = trees[q].d > max_d ? trees[q].d : max_d;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t split_lds = split_lds_bytes(max_n, REG), part_lds = partition_lds_bytes(max_n);      // 12 n reaches 96 KB of the CU's 160 KB at n = 8192
    if (int rc = bbbp_ensure_dyn_lds(reinterpret_cast<const void*>(rf_split_kernel<REG>), split_lds)) return rc;
    if (int rc = bbbp_ensure_dyn_lds(reinterpret_cast<const void*>(rf_partition_kernel), part_lds)) return rc;
    const unsigned T = (unsigned)n_trees;
    const dim3 rows((unsigned)cdiv(max_n, 256), T), feats((unsigned)max_d, T), nodes((unsigned)clampi(cdiv(max_n, 64), 1, 32), T), one(T);
    hipLaunchKernelGGL(rf_init_rows_kernel, rows, dim3(256), 0, st, trees_device);
    hipLaunchKernelGGL(rf_init_boot_kernel, rows, dim3(256), 0, st, trees_device);
    hipLaunchKernelGGL(rf_init_compact_kernel<REG>, feats, dim3(RF_SCAN), 0, st, trees_device);
    BBBP_CHECK_LAUNCH();
    // a tree of n rows has at most n - 1 levels that split, and one more round to find that nothing is left
    const int max_blocks = max_n / RF_BLOCK_ROUNDS + 2;
    for (int b = 0; b < max_blocks; ++b) {
        BBBP_CHECK_HIP(hipMemsetAsync(alive_device, 0, sizeof(int), st));
        for (int r = 0; r < RF_BLOCK_ROUNDS; ++r) {
            hipLaunchKernelGGL(rf_stats_kernel<REG>, nodes, dim3(256), 0, st, trees_device);
            hipLaunchKernelGGL(rf_draw_kernel, nodes, dim3(256), 0, st, trees_device);
            hipLaunchKernelGGL(rf_split_kernel<REG>, feats, dim3(RF_SCAN), split_lds, st, trees_device);
            hipLaunchKernelGGL(rf_choose_kernel, one, dim3(256), 0, st, trees_device, alive_device, r == RF_BLOCK_ROUNDS - 1 ? 1 : 0);
            hipLaunchKernelGGL(rf_side_kernel, rows, dim3(256), 0, st, trees_device);
            hipLaunchKernelGGL(rf_partition_kernel, feats, dim3(RF_SCAN), part_lds, st, trees_device);
            BBBP_CHECK_LAUNCH();
        }
        int alive = 0;                                      // the only host read before the result
        BBBP_CHECK_HIP(hipMemcpyAsync(&alive, alive_device, sizeof(int), hipMemcpyDeviceToHost, st));
        BBBP_CHECK_HIP(hipStreamSynchronize(st));
        if (!alive) return BBBP_OK;
    }
    bbbp_set_error("rf_fit: a tree still grows after %d levels", max_blocks * RF_BLOCK_ROUNDS);
    return BBBP_ERR_HIP;
}
}  // namespace

extern "C" int bbbp_rf_fit(void* stream, const bbbp_rf_tree* trees, const bbbp_rf_tree* trees_device, int n_trees, int* alive_device) {
    return fit_trees<false>(stream, trees, trees_device, n_trees, alive_device);
}

extern "C" int bbbp_rf_fit_regression(void* stream, const bbbp_rf_tree* trees, const bbbp_rf_tree* trees_device, int n_trees, int* alive_device) {
    return fit_trees<true>(stream, trees, trees_device, n_trees, alive_device);
}

extern "C" int bbbp_rf_predict_proba(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                                     const double* threshold, const double* p0, const double* p1, const int* n_node_samples, const int* root,
                                     int n_trees, int max_depth, int min_samples_split, double* out) {
    BBBP_CHECK_ARG(m >= 1 && d >= 1, "rf_predict_proba: m and d must be positive, got m %d d %d", m, d);
    BBBP_CHECK_ARG(ld >= d, "rf_predict_proba: leading dimension %ld below d %d", ld, d);
    BBBP_CHECK_ARG(n_trees >= 1 && max_depth >= 0 && min_samples_split >= 0, "rf_predict_proba: n_trees %d, max_depth %d, min_samples_split %d", n_trees,
                   max_depth, min_samples_split);
    BBBP_CHECK_ARG(X && left && right && feature && threshold && p0 && p1 && n_node_samples && root && out, "rf_predict_proba: null pointer");
    PredictArgs a{X, ld, m, d, left, right, feature, threshold, p0, p1, n_node_samples, root, n_trees, max_depth, min_samples_split, out};
    hipLaunchKernelGGL(rf_predict_kernel<false>, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_rf_predict_mean(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                                    const double* threshold, const double* value, const int* n_node_samples, const int* root, int n_trees,
                                    int max_depth, int min_samples_split, double* out) {
    BBBP_CHECK_ARG(m >= 1 && d >= 1, "rf_predict_mean: m and d must be positive, got m %d d %d", m, d);
    BBBP_CHECK_ARG(ld >= d, "rf_predict_mean: leading dimension %ld below d %d", ld, d);
    BBBP_CHECK_ARG(n_trees >= 1 && max_depth >= 0 && min_samples_split >= 0, "rf_predict_mean: n_trees %d, max_depth %d, min_samples_split %d", n_trees,
                   max_depth, min_samples_split);
    BBBP_CHECK_ARG(X && left && right && feature && threshold && value && n_node_samples && root && out, "rf_predict_mean: null pointer");
    PredictArgs a{X, ld, m, d, left, right, feature, threshold, nullptr, value, n_node_samples, root, n_trees, max_depth, min_samples_split, out};
    hipLaunchKernelGGL(rf_predict_kernel<true>, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
