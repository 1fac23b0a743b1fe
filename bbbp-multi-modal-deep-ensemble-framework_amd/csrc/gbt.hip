// Gradient-boosted classification trees, fitted on the GPU: GradientBoostingClassifier of the classification stack
// (Models/model_opt_maccs.py:124-200; two classes, log-loss, friedman_mse, no subsampling, the prior as init), searched over
// n_estimators x learning_rate x max_depth x min_samples_split.  scikit-learn's algorithm (ensemble/_gb.py, tree/_splitter.pyx,
// _criterion.pyx), restated: features are float32; a stage fits one regression tree to g = y - expit(raw) by exact split search over the
// sorted columns, a leaf's value is mean(g) / mean(p (1 - p)) with p = y - g, and raw += learning_rate * value[leaf].
//
// A *chain* is one boosted model being fitted.  Many chains run side by side (the grid's chains of all folds); chains over the same
// training matrix share its float32 column-major copy and its presorted row order per feature.  Trees grow level by level.  The rows of
// a chain carry a *key*: the path from the root, one bit per level (a leaf's rows keep going "left"), so at level L the keys are
// < 2^L and every feature's row order is partitioned into the same contiguous key segments, each sorted by that feature's value.
// One *round* advances every chain by one level with six launches:
//   stats      one work-group per chain: sum g, sum g^2, sum p (1 - p) of every new node (one wave per node, lane-strided then a
//              butterfly: the order is fixed by the node's rows in feature 0's order); decides the leaves the stop rules give
//   split      one work-group per (feature, chain): residuals and keys in LDS, a segmented float64 prefix sum over the feature's order
//              in passes of GBT_SCAN positions with a carry, the score of every valid position, the best (score, position) per node
//   choose     one wave per chain: arg-max over features (the lowest feature wins among equal scores, then the lowest position),
//              the threshold, the children; a node without a valid split becomes a leaf
//   side       one thread per row: the new key
//   partition  one work-group per (feature, chain): a stable partition of every segment by the new key's last bit
//   update     one work-group per chain: on a finished tree raw += lr * value[leaf], the stage's score under the loss, the next residuals
// Chains of different depth take different numbers of rounds per tree; each keeps its own (tree, level) on the device and a kernel
// leaves at once for a chain that has nothing to do in it.  Nothing is read back by the host before the last round.
// Every sum's order depends on the chain's own data alone: a chain's trees are bit-identical alone, in any batch, and run to run.
//
// The loss is a template parameter of the kernels that know about it -- init, stats, update, and choose for the leaf it makes of a node
// without a valid split -- so no row takes a runtime branch on it; split, side and partition are shared.  HalfBinomial is the classifier
// above (bbbp_gbt_fit).  SquaredError (bbbp_gbr_fit) is GradientBoostingRegressor of the logBB stack's bake-off
// (Models/multi_input_data_regression_opt_transformer_cnn_opt_more.py:118-125): g = y - raw, stats sums g and g^2 alone, every node's
// value is sum g / m (scikit-learn skips the leaf update for this loss), the stage score is the mean of (y - raw)^2.
#include "common.h"
#include "bbbp_hip.h"
#include "tree_fit.h"

#include <math.h>

namespace {

constexpr int GBT_SCAN = 256;                 // positions per pass of the split and partition kernels = their threads
constexpr int GBT_KEYS = 1 << BBBP_GBT_FIT_MAX_DEPTH;          // keys at the deepest level
constexpr int GBT_SPLIT_KEYS = GBT_KEYS / 2;  // keys at the deepest level that is searched
constexpr int KEY_EMPTY = 0, KEY_ACTIVE = 1, KEY_LEAF = 2;
constexpr double GBT_EPSILON = 2.220446049250313e-16;      // scikit-learn's impurity floor (the float64 machine epsilon)
constexpr float GBT_FEATURE_THRESHOLD = 1e-7f;

struct KeyTab {                               // the nodes of one level, by key
    int start[GBT_KEYS], cnt[GBT_KEYS], node[GBT_KEYS], flag[GBT_KEYS];
    double sum_g[GBT_KEYS], sum_pq[GBT_KEYS];
};
struct SplitTab {                             // what `choose` leaves for `side` and `partition`
    int split[GBT_SPLIT_KEYS], feature[GBT_SPLIT_KEYS], n_left[GBT_SPLIT_KEYS], left_base[GBT_SPLIT_KEYS];
    double threshold[GBT_SPLIT_KEYS];
};
struct ChainState { int tree, level, final, n_nodes, error; };      // error: an index left its array (see row_of); reported through tree_nodes
__host__ __device__ inline int tree_capacity(int max_depth) { return (2 << max_depth) - 1; }

struct Work {                                 // offsets into a chain's `work`, in bytes; all multiples of 16
    size_t order[2], key, g, tab[2], split, cand_enc, cand_pos, state, total;
};
__host__ __device__ inline Work work_layout(int n, int d) {
    Work w;
    Area a;
    w.order[0] = a.take((size_t)d * n * 4);
    w.order[1] = a.take((size_t)d * n * 4);
    w.key = a.take((size_t)n);
    w.g = a.take((size_t)n * 8);
    w.tab[0] = a.take(sizeof(KeyTab));
    w.tab[1] = a.take(sizeof(KeyTab));
    w.split = a.take(sizeof(SplitTab));
    w.cand_enc = a.take((size_t)d * GBT_SPLIT_KEYS * 8);
    w.cand_pos = a.take((size_t)d * GBT_SPLIT_KEYS * 4);
    w.state = a.take(sizeof(ChainState));
    w.total = a.at;
    return w;
}

struct View {                                 // a chain's work area, typed
    int *order_a, *order_b; uint8_t* key; double* g; KeyTab *tab_a, *tab_b; SplitTab* split; unsigned long long* cand_enc; int* cand_pos; ChainState* st;
};
__device__ inline View view_of(const bbbp_gbt_chain& c) {
    const Work w = work_layout(c.n, c.d);
    char* b = static_cast<char*>(c.work);
    View v;
    v.order_a = (int*)(b + w.order[0]); v.order_b = (int*)(b + w.order[1]);
    v.key = (uint8_t*)(b + w.key); v.g = (double*)(b + w.g);
    v.tab_a = (KeyTab*)(b + w.tab[0]); v.tab_b = (KeyTab*)(b + w.tab[1]);
    v.split = (SplitTab*)(b + w.split);
    v.cand_enc = (unsigned long long*)(b + w.cand_enc); v.cand_pos = (int*)(b + w.cand_pos);
    v.st = (ChainState*)(b + w.state);
    return v;
}
// The row order the kernels of level L read (level 0: the presorted order all chains of a matrix share) and the one `partition` writes
__device__ inline const int* order_src(const bbbp_gbt_chain& c, const View& v, int level) { return level == 0 ? c.order0 : (((level - 1) & 1) ? v.order_b : v.order_a); }
__device__ inline int* order_dst(const View& v, int level) { return (level & 1) ? v.order_b : v.order_a; }
__device__ inline KeyTab* tab_of(const View& v, int level) { return (level & 1) ? v.tab_b : v.tab_a; }       // selects, not indexed arrays: no scratch
// row_of (tree_fit.h) sets the chain's error word, which `update` reports as tree_nodes[t] = -1
__device__ inline bool chain_idle(const bbbp_gbt_chain& c, const ChainState* st) { return st->tree >= c.n_estimators; }

// ---- the loss: a compile-time parameter of the kernels that know about it (init, stats, choose's late leaf, update) ------------------
// scikit-learn's half-binomial loss and gradient (_loss/_loss.pyx.tp), restated: loss = log1pexp(raw) - y raw, residual = y - expit(raw)
__device__ inline double log1pexp(double x) {
    if (x <= -37.0) return exp(x);
    if (x <= -2.0) return log1p(exp(x));
    if (x <= 18.0) return log(1.0 + exp(x));
    if (x <= 33.3) return x + exp(-x);
    return x;
}
struct HalfBinomial {                         // GradientBoostingClassifier: y in {0, 1}
    static constexpr bool kNewton = true;     // a leaf's value is one Newton step, mean(g) / mean(p (1 - p)): stats sums p (1 - p) too
    __device__ static inline double residual(double y, double raw) {
        if (raw > -37.0) {
            const double e = exp(-raw);
            return -(((1.0 - y) - y * e) / (1.0 + e));
        }
        return -(exp(raw) - y);
    }
    __device__ static inline double row_loss(double y, double raw) {
#pragma clang fp contract(off)
        return log1pexp(raw) - y * raw;                     // product and difference rounded separately, as the sum they join
    }
    __device__ static inline double leaf_value(double sum_g, double sum_pq, int m) {
        const double num = sum_g / m, den = sum_pq / m;
        return fabs(den) < 1e-150 ? 0.0 : num / den;
    }
    __device__ static inline double stage_score(double sum, int n) { return 2.0 * (sum / n); }      // scikit-learn's train_score_: twice the mean half-binomial loss
};
// scikit-learn's half squared error: residual = y - raw; _update_terminal_regions is skipped, so the tree's own node mean sum g / m, which
// stats writes into every node, is the update and nothing is summed beside g and g^2; train_score_ is the mean of (y - raw)^2
struct SquaredError {                         // GradientBoostingRegressor: y real
    static constexpr bool kNewton = false;
    __device__ static inline double residual(double y, double raw) { return y - raw; }
    __device__ static inline double row_loss(double y, double raw) {
#pragma clang fp contract(off)
        const double r = y - raw;
        return r * r;
    }
    __device__ static inline double stage_score(double sum, int n) { return sum / n; }
};

template <class Loss>
__global__ __launch_bounds__(256) void gbt_init_kernel(const bbbp_gbt_chain* chains) {
    const bbbp_gbt_chain c = chains[blockIdx.y];
    const View v = view_of(c);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *v.st = ChainState{0, 0, 0, 0, 0};
    if (i >= c.n) return;
    c.raw[i] = c.init;
    v.g[i] = Loss::residual(c.y[i], c.init);
    v.key[i] = 0;
}

// ---- stats: the new nodes' sums and the stop rules ----------------------------------------------------------------------------------
template <class Loss>
__global__ __launch_bounds__(256) void gbt_stats_kernel(const bbbp_gbt_chain* chains) {
    const bbbp_gbt_chain c = chains[blockIdx.x];
    const View v = view_of(c);
    if (chain_idle(c, v.st)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int level = v.st->level, tree = v.st->tree, nk = 1 << level;
    KeyTab* tab = tab_of(v, level);
    if (level == 0) {
        if (tid == 0) {
            tab->start[0] = 0; tab->cnt[0] = c.n; tab->node[0] = 0; tab->flag[0] = KEY_ACTIVE;
            v.st->n_nodes = 1;
        }
        __syncthreads();
    }
    const int cap = tree_capacity(c.max_depth);
    const long base = (long)tree * cap;
    const int* src = order_src(c, v, level);       // feature 0's order: key segments are contiguous in it
    __shared__ int active[4];
    int mine = 0;
    for (int k = wave; k < nk; k += 4) {
        if (tab->flag[k] != KEY_ACTIVE) continue;
        const int s = tab->start[k], m = tab->cnt[k];
        double sg = 0.0, sq = 0.0, spq = 0.0;
        for (int p = lane; p < m && s + p < c.n; p += 64) {
            const int i = row_of(src, s + p, c.n, v.st);
            const double g = v.g[i];
            sg += g; sq += g * g;
            if constexpr (Loss::kNewton) {
                const double pr = c.y[i] - g;
                spq += pr * (1.0 - pr);
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            sg += __shfl_xor(sg, off); sq += __shfl_xor(sq, off);
            if constexpr (Loss::kNewton) spq += __shfl_xor(spq, off);
        }
        if (lane == 0) {
            const double mean = sg / m, impurity = sq / m - mean * mean;
            const bool leaf = level >= c.max_depth || m < c.min_samples_split || m < 2 * c.min_samples_leaf || impurity <= GBT_EPSILON;
            const long node = base + tab->node[k];
            tab->sum_g[k] = sg; tab->sum_pq[k] = spq;           // sum_pq: 0 without a Newton step, and nothing reads it then
            c.n_node_samples[node] = m;
            if (leaf) {
                tab->flag[k] = KEY_LEAF;
                make_leaf(c, node);
                if constexpr (Loss::kNewton) c.value[node] = Loss::leaf_value(sg, spq, m);
                else c.value[node] = mean;
            } else {
                c.value[node] = mean;
                ++mine;
            }
        }
    }
    if (lane == 0) active[wave] = mine;
    __syncthreads();
    if (tid == 0) v.st->final = (active[0] + active[1] + active[2] + active[3]) == 0;
}

// ---- split: best (score, position) per node for one feature -------------------------------------------------------------------------
__global__ __launch_bounds__(GBT_SCAN) void gbt_split_kernel(const bbbp_gbt_chain* chains) {
    const bbbp_gbt_chain c = chains[blockIdx.y];
    const View v = view_of(c);
    if (chain_idle(c, v.st) || v.st->final) return;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = c.n;
    if (f >= c.d) return;                                   // the grid is sized for the widest chain of the batch
    const int level = v.st->level, nk = 1 << level;
    const KeyTab* tab = tab_of(v, level);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sg = reinterpret_cast<double*>(smem);                                 // [n] residuals
    double* slot = sg + n;                                                        // [GBT_SCAN + 1] inclusive sums of a pass, behind the carry
    double* ksum = slot + GBT_SCAN + 1;                                           // [GBT_SPLIT_KEYS] node totals
    unsigned long long* best_enc = reinterpret_cast<unsigned long long*>(ksum + GBT_SPLIT_KEYS);      // [GBT_SPLIT_KEYS]
    unsigned long long* pass_enc = best_enc + GBT_SPLIT_KEYS;
    double* wave_val = reinterpret_cast<double*>(pass_enc + GBT_SPLIT_KEYS);      // [4]
    int* best_pos = reinterpret_cast<int*>(wave_val + 4);                         // [GBT_SPLIT_KEYS] each
    int* pass_pos = best_pos + GBT_SPLIT_KEYS;
    int* kstart = pass_pos + GBT_SPLIT_KEYS;
    int* kcnt = kstart + GBT_SPLIT_KEYS;
    int* kflag = kcnt + GBT_SPLIT_KEYS;
    int* wave_flag = kflag + GBT_SPLIT_KEYS;                                      // [4]
    uint8_t* skey = reinterpret_cast<uint8_t*>(wave_flag + 4);                    // [n]
    for (int i = tid; i < n; i += GBT_SCAN) { sg[i] = v.g[i]; skey[i] = v.key[i]; }
    if (tid < GBT_SPLIT_KEYS) {
        const bool in = tid < nk;
        kstart[tid] = in ? tab->start[tid] : 0; kcnt[tid] = in ? tab->cnt[tid] : 0; kflag[tid] = in ? tab->flag[tid] : KEY_EMPTY;
        ksum[tid] = in ? tab->sum_g[tid] : 0.0;
        best_enc[tid] = 0ull; best_pos[tid] = 0;
    }
    if (tid == 0) slot[GBT_SCAN] = 0.0;
    __syncthreads();
    const int* src = order_src(c, v, level) + (long)f * n;
    const float* col = c.XT + (long)f * n;
    const int msl = c.min_samples_leaf;
    for (int base = 0; base < n; base += GBT_SCAN) {
        const int p = base + tid;
        const bool in = p < n;
        const int i = in ? row_of(src, p, n, v.st) : 0;
        const int k = in ? (skey[i] & (GBT_SPLIT_KEYS - 1)) : 0;
        const bool act = in && kflag[k] == KEY_ACTIVE;
        const int s = kstart[k];
        const double x = act ? sg[i] : 0.0;
        const double carry = slot[GBT_SCAN];                // the inclusive sum at position base - 1
        // segmented inclusive scan inside the wave: a segment starts at its node's first position (and at every position past the end)
        const auto add = [](double a, double b) { return a + b; };
        double val = x;
        int flg = (!in || p == s) ? 1 : 0;
        wave_segmented_scan(val, flg, add);
        if (lane == 63) { wave_val[wave] = val; wave_flag[wave] = flg; }
        if (tid < GBT_SPLIT_KEYS) { pass_enc[tid] = 0ull; pass_pos[tid] = 0x7fffffff; }
        __syncthreads();
        const double pre = block_segment_prefix(carry, wave_val, wave_flag, add);
        if (!flg) val = pre + val;
        slot[1 + tid] = val;
        if (tid == 0) slot[0] = carry;
        __syncthreads();
        // the candidate between positions p - 1 and p
        unsigned long long enc = 0ull;
        if (act && p > s) {
            const int n_l = p - s, n_r = kcnt[k] - n_l;
            const float fv = col[i], fv_prev = col[row_of(src, p - 1, n, v.st)];
            if (fv > fv_prev + GBT_FEATURE_THRESHOLD && n_l >= msl && n_r >= msl) {
#pragma clang fp contract(off)
                const double s_l = slot[tid], s_r = ksum[k] - s_l;
                const double diff = (double)n_r * s_l - (double)n_l * s_r;
                const double score = diff * diff / ((double)n_l * (double)n_r);
                enc = encode_score(score);
                atomicMax(&pass_enc[k], enc);
            }
        }
        __syncthreads();
        if (enc != 0ull && pass_enc[k] == enc) atomicMin(&pass_pos[k], p);
        __syncthreads();
        if (tid < GBT_SPLIT_KEYS && pass_enc[tid] > best_enc[tid]) { best_enc[tid] = pass_enc[tid]; best_pos[tid] = pass_pos[tid]; }
        // the next pass reads slot[GBT_SCAN] and rewrites pass_* before its first barrier: only threads tid < GBT_SPLIT_KEYS touch pass_*
        // there, the same ones that read them here; slot is rewritten behind that barrier
    }
    __syncthreads();
    if (tid < nk) {
        v.cand_enc[(long)f * GBT_SPLIT_KEYS + tid] = best_enc[tid];
        v.cand_pos[(long)f * GBT_SPLIT_KEYS + tid] = best_pos[tid];
    }
}
size_t split_lds_bytes(int n) {
    return (size_t)n * 8 + (GBT_SCAN + 1 + GBT_SPLIT_KEYS) * 8 + 2 * GBT_SPLIT_KEYS * 8 + 4 * 8 + 5 * GBT_SPLIT_KEYS * 4 + 4 * 4 + (size_t)n;
}

// ---- choose: the best feature per node, its threshold and children ------------------------------------------------------------------
template <class Loss>
__global__ __launch_bounds__(64) void gbt_choose_kernel(const bbbp_gbt_chain* chains) {
    const bbbp_gbt_chain c = chains[blockIdx.x];
    const View v = view_of(c);
    if (chain_idle(c, v.st) || v.st->final) return;
    const int k = threadIdx.x, n = c.n;
    const int level = v.st->level, nk = 1 << level, n_nodes = v.st->n_nodes;
    KeyTab* tab = tab_of(v, level);
    KeyTab* next = tab_of(v, level + 1);
    const long base = (long)v.st->tree * tree_capacity(c.max_depth);
    const bool in = k < nk;
    const int flag = in ? tab->flag[k] : KEY_EMPTY;
    const int s = in ? tab->start[k] : 0, m = in ? tab->cnt[k] : 0, node = in ? tab->node[k] : 0;
    unsigned long long best = 0ull;
    int bf = 0, bp = 0;
    if (flag == KEY_ACTIVE)
        for (int f = 0; f < c.d; ++f) {
            const unsigned long long e = v.cand_enc[(long)f * GBT_SPLIT_KEYS + k];
            if (e > best) { best = e; bf = f; bp = v.cand_pos[(long)f * GBT_SPLIT_KEYS + k]; }
        }
    const bool split = best != 0ull && bp > s && bp < s + m;
    const unsigned long long ballot = __ballot(split);
    const int rank = __popcll(ballot & ((1ull << k) - 1ull));
    int n_left = (flag == KEY_EMPTY) ? 0 : m;               // a leaf's rows all keep going left
    if (split) {
        const int* src = order_src(c, v, level) + (long)bf * n;
        const float a = c.XT[(long)bf * n + row_of(src, bp - 1, n, v.st)], b = c.XT[(long)bf * n + row_of(src, bp, n, v.st)];
        const double thr = split_threshold(a, b);
        n_left = bp - s;
        const int lc = n_nodes + 2 * rank, rc = lc + 1;
        c.left[base + node] = lc; c.right[base + node] = rc; c.feature[base + node] = bf; c.threshold[base + node] = thr;
        v.split->feature[k] = bf; v.split->threshold[k] = thr;
        next->start[2 * k] = s; next->cnt[2 * k] = n_left; next->node[2 * k] = lc; next->flag[2 * k] = KEY_ACTIVE;
        next->start[2 * k + 1] = s + n_left; next->cnt[2 * k + 1] = m - n_left; next->node[2 * k + 1] = rc; next->flag[2 * k + 1] = KEY_ACTIVE;
    } else if (in) {
        if (flag == KEY_ACTIVE) {                           // no valid split: a leaf after all
            make_leaf(c, base + node);
            if constexpr (Loss::kNewton) c.value[base + node] = Loss::leaf_value(tab->sum_g[k], tab->sum_pq[k], m);      // else: stats wrote the mean
        }
        const int keep = flag == KEY_EMPTY ? KEY_EMPTY : KEY_LEAF;
        next->start[2 * k] = s; next->cnt[2 * k] = m; next->node[2 * k] = node; next->flag[2 * k] = keep;
        next->start[2 * k + 1] = s + m; next->cnt[2 * k + 1] = 0; next->node[2 * k + 1] = 0; next->flag[2 * k + 1] = KEY_EMPTY;
    }
    // rows that go left in the segments in front of this one
    int incl = n_left;
    for (int off = 1; off < 64; off <<= 1) {
        const int pv = __shfl_up(incl, off);
        if (k >= off) incl += pv;
    }
    v.split->split[k] = split ? 1 : 0;
    v.split->n_left[k] = n_left;
    v.split->left_base[k] = incl - n_left;
    __syncthreads();
    if (k == 0) v.st->n_nodes = n_nodes + 2 * __popcll(ballot);
}

// ---- side: every row's key at the next level ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gbt_side_kernel(const bbbp_gbt_chain* chains) {
    const bbbp_gbt_chain c = chains[blockIdx.y];
    const View v = view_of(c);
    if (chain_idle(c, v.st) || v.st->final) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const int k = v.key[i] & (GBT_SPLIT_KEYS - 1);
    int side = 0;
    if (v.split->split[k]) side = ((double)c.XT[(long)v.split->feature[k] * c.n + i] <= v.split->threshold[k]) ? 0 : 1;
    v.key[i] = (uint8_t)(2 * k + side);
}

// ---- partition: every feature's order, stably, by the new key's last bit inside each segment -----------------------------------------
__global__ __launch_bounds__(GBT_SCAN) void gbt_partition_kernel(const bbbp_gbt_chain* chains) {
    const bbbp_gbt_chain c = chains[blockIdx.y];
    const View v = view_of(c);
    if (chain_idle(c, v.st) || v.st->final) return;
    const int f = blockIdx.x, tid = threadIdx.x, n = c.n;
    if (f >= c.d) return;                                   // the grid is sized for the widest chain of the batch
    const int level = v.st->level, nk = 1 << level;
    const KeyTab* tab = tab_of(v, level);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* kstart = reinterpret_cast<int*>(smem);                       // [GBT_SPLIT_KEYS] each
    int* kleft = kstart + GBT_SPLIT_KEYS;
    int* kbase = kleft + GBT_SPLIT_KEYS;
    int* wave_cnt = kbase + GBT_SPLIT_KEYS;                           // [2][4]
    uint8_t* skey = reinterpret_cast<uint8_t*>(wave_cnt + 8);         // [n] new keys
    for (int i = tid; i < n; i += GBT_SCAN) skey[i] = v.key[i];
    if (tid < GBT_SPLIT_KEYS) {
        const bool in = tid < nk;
        kstart[tid] = in ? tab->start[tid] : 0; kleft[tid] = in ? v.split->n_left[tid] : 0; kbase[tid] = in ? v.split->left_base[tid] : 0;
    }
    __syncthreads();
    const int* src = order_src(c, v, level) + (long)f * n;
    int* dst = order_dst(v, level) + (long)f * n;
    int before = 0;                                                   // rows going left in front of this pass
    for (int base = 0, it = 0; base < n; base += GBT_SCAN, ++it) {
        const int p = base + tid;
        const bool in = p < n;
        const int i = in ? row_of(src, p, n, v.st) : 0;
        const int key = in ? skey[i] : 0;
        const bool left = in && !(key & 1);
        const int lefts = block_rank_before(left, wave_cnt + (it & 1) * 4, before);
        if (in) {
            const int k = (key >> 1) & (GBT_SPLIT_KEYS - 1);
            const int in_seg = lefts - kbase[k];                      // rows of this segment going left in front of p
            const int to = left ? kstart[k] + in_seg : kstart[k] + kleft[k] + (p - kstart[k] - in_seg);
            if ((unsigned)to < (unsigned)n) dst[to] = i;
            else v.st->error = 1;
        }
    }
}
size_t partition_lds_bytes(int n) { return (3 * GBT_SPLIT_KEYS + 8) * 4 + (size_t)n; }

// ---- update: a finished tree's raw scores, the stage's score under the loss and next residuals; every chain's next (tree, level) -------
template <class Loss>
__global__ __launch_bounds__(1024) void gbt_update_kernel(const bbbp_gbt_chain* chains) {
    const bbbp_gbt_chain c = chains[blockIdx.x];
    const View v = view_of(c);
    if (chain_idle(c, v.st)) return;
    const int tid = threadIdx.x;
    const int level = v.st->level, tree = v.st->tree;
    if (!v.st->final) {
        __syncthreads();
        if (tid == 0) v.st->level = level + 1;
        return;
    }
    const KeyTab* tab = tab_of(v, level);
    const int cap = tree_capacity(c.max_depth);
    const long base = (long)tree * cap;
    __shared__ double part[1024];
    double loss = 0.0;
    for (int i = tid; i < c.n; i += 1024) {
#pragma clang fp contract(off)
        const int node = tab->node[v.key[i] & (GBT_KEYS - 1)];
        if ((unsigned)node >= (unsigned)cap) v.st->error = 1;
        const double val = c.value[base + ((unsigned)node < (unsigned)cap ? node : 0)];
        const double step = c.learning_rate * val;           // two roundings, as scikit-learn's predict_stages
        const double raw = c.raw[i] + step;
        const double y = c.y[i];
        c.raw[i] = raw;
        loss += Loss::row_loss(y, raw);
        v.g[i] = Loss::residual(y, raw);
        v.key[i] = 0;
    }
    part[tid] = loss;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        c.train_score[tree] = Loss::stage_score(part[0], c.n);
        c.tree_nodes[tree] = v.st->error ? -1 : v.st->n_nodes;       // the error word stays set: every later tree reports it too
        v.st->tree = tree + 1; v.st->level = 0; v.st->final = 0; v.st->n_nodes = 0;
    }
}

// ---- decision: raw scores of query rows at the requested stage counts ---------------------------------------------------------------
struct DecisionArgs {
    const float* X; long ld; int m, d;
    const int *left, *right, *feature; const double *threshold, *value; const int* root;
    int n_trees; double init, lr; const int* stages; int n_stages; double* out;
};
__global__ __launch_bounds__(256) void gbt_decision_kernel(DecisionArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const float* x = a.X + (long)i * a.ld;
    double raw = a.init;
    int s = 0;
    for (int t = 0; t < a.n_trees && s < a.n_stages; ++t) {
#pragma clang fp contract(off)
        int node = a.root[t], steps = 0;
        int l = a.left[node];
        while (l >= 0 && steps < BBBP_GBT_FIT_MAX_WALK) {         // bounded: arrays handed to the C ABI directly cannot spin a wave for ever
            node = (double)x[a.feature[node]] <= a.threshold[node] ? l : a.right[node];
            l = a.left[node];
            ++steps;
        }
        const double step = a.lr * a.value[node];            // scikit-learn's predict_stages: scale * value, then the add
        raw = (l >= 0) ? __builtin_nan("") : raw + step;
        if (t + 1 == a.stages[s]) { a.out[(long)s * a.m + i] = raw; ++s; }
    }
}

int check_chain(const char* who, const bbbp_gbt_chain& c, int q) {
    BBBP_CHECK_ARG(c.n >= 2 && c.d >= 1, "%s: chain %d: n >= 2 and d >= 1 must hold, got n %d d %d", who, q, c.n, c.d);
    BBBP_CHECK_ARG(c.n <= BBBP_GBT_FIT_MAX_N, "%s: chain %d: n %d exceeds BBBP_GBT_FIT_MAX_N %d", who, q, c.n, BBBP_GBT_FIT_MAX_N);
    BBBP_CHECK_ARG(c.d <= BBBP_GBT_FIT_MAX_D, "%s: chain %d: d %d exceeds BBBP_GBT_FIT_MAX_D %d", who, q, c.d, BBBP_GBT_FIT_MAX_D);
    BBBP_CHECK_ARG(c.max_depth >= 1 && c.max_depth <= BBBP_GBT_FIT_MAX_DEPTH, "%s: chain %d: max_depth %d outside 1..%d", who, q, c.max_depth, BBBP_GBT_FIT_MAX_DEPTH);
    BBBP_CHECK_ARG(c.n_estimators >= 1 && c.n_estimators <= BBBP_GBT_FIT_MAX_TREES, "%s: chain %d: n_estimators %d outside 1..%d", who, q, c.n_estimators,
                   BBBP_GBT_FIT_MAX_TREES);
    BBBP_CHECK_ARG(c.min_samples_split >= 2, "%s: chain %d: min_samples_split %d must be >= 2", who, q, c.min_samples_split);
    BBBP_CHECK_ARG(c.min_samples_leaf >= 1, "%s: chain %d: min_samples_leaf %d must be >= 1", who, q, c.min_samples_leaf);
    BBBP_CHECK_ARG(c.learning_rate > 0.0 && c.learning_rate < INFINITY, "%s: chain %d: learning_rate must be positive and finite", who, q);
    BBBP_CHECK_ARG(c.init == c.init && fabs(c.init) < INFINITY, "%s: chain %d: init must be finite", who, q);
    BBBP_CHECK_ARG(c.XT && c.order0 && c.y && c.work && c.left && c.right && c.feature && c.n_node_samples && c.threshold && c.value && c.tree_nodes &&
                       c.train_score && c.raw, "%s: chain %d: null pointer", who, q);
    return BBBP_OK;
}

template <class Loss>
int fit_chains(const char* who, void* stream, const bbbp_gbt_chain* chains, const bbbp_gbt_chain* chains_device, int n_chains) {
    BBBP_CHECK_ARG(chains && chains_device, "%s: null pointer", who);
    BBBP_CHECK_ARG(n_chains >= 1 && n_chains <= 65535, "%s: n_chains %d outside 1..65535", who, n_chains);
    int max_n = 0, max_d = 0;
    long rounds = 0;
    for (int q = 0; q < n_chains; ++q) {
        if (int rc = check_chain(who, chains[q], q)) return rc;
        max_n = chains[q].n > max_n ? chains[q].n : max_n;
        max_d = chains[q].d > max_d ? chains[q].d : max_d;
        const long r = (long)chains[q].n_estimators * (chains[q].max_depth + 1);
        rounds = r > rounds ? r : rounds;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t split_lds = split_lds_bytes(max_n), part_lds = partition_lds_bytes(max_n);
    if (int rc = bbbp_ensure_dyn_lds(reinterpret_cast<const void*>(gbt_split_kernel), split_lds)) return rc;
    if (int rc = bbbp_ensure_dyn_lds(reinterpret_cast<const void*>(gbt_partition_kernel), part_lds)) return rc;
    const dim3 rows((unsigned)cdiv(max_n, 256), (unsigned)n_chains), feats((unsigned)max_d, (unsigned)n_chains), one((unsigned)n_chains);
    hipLaunchKernelGGL(gbt_init_kernel<Loss>, rows, dim3(256), 0, st, chains_device);
    BBBP_CHECK_LAUNCH();
    for (long r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(gbt_stats_kernel<Loss>, one, dim3(256), 0, st, chains_device);
        hipLaunchKernelGGL(gbt_split_kernel, feats, dim3(GBT_SCAN), split_lds, st, chains_device);
        hipLaunchKernelGGL(gbt_choose_kernel<Loss>, one, dim3(64), 0, st, chains_device);
        hipLaunchKernelGGL(gbt_side_kernel, rows, dim3(256), 0, st, chains_device);
        hipLaunchKernelGGL(gbt_partition_kernel, feats, dim3(GBT_SCAN), part_lds, st, chains_device);
        hipLaunchKernelGGL(gbt_update_kernel<Loss>, one, dim3(1024), 0, st, chains_device);
        BBBP_CHECK_LAUNCH();
    }
    return BBBP_OK;
}

}  // namespace

extern "C" int bbbp_gbt_fit_tree_capacity(int max_depth) {
    if (max_depth < 1 || max_depth > BBBP_GBT_FIT_MAX_DEPTH) {
        bbbp_set_error("gbt_fit_tree_capacity: max_depth %d outside 1..%d", max_depth, BBBP_GBT_FIT_MAX_DEPTH);
        return 0;
    }
    return tree_capacity(max_depth);
}

extern "C" size_t bbbp_gbt_fit_work_bytes(int n, int d) {
    if (n < 2 || d < 1) { bbbp_set_error("gbt_fit_work_bytes: n >= 2 and d >= 1 must hold, got n %d d %d", n, d); return 0; }
    if (n > BBBP_GBT_FIT_MAX_N) { bbbp_set_error("gbt_fit_work_bytes: n %d exceeds BBBP_GBT_FIT_MAX_N %d", n, BBBP_GBT_FIT_MAX_N); return 0; }
    if (d > BBBP_GBT_FIT_MAX_D) { bbbp_set_error("gbt_fit_work_bytes: d %d exceeds BBBP_GBT_FIT_MAX_D %d", d, BBBP_GBT_FIT_MAX_D); return 0; }
    return work_layout(n, d).total;
}

extern "C" int bbbp_gbt_fit(void* stream, const bbbp_gbt_chain* chains, const bbbp_gbt_chain* chains_device, int n_chains) {
    return fit_chains<HalfBinomial>("gbt_fit", stream, chains, chains_device, n_chains);
}

extern "C" int bbbp_gbr_fit(void* stream, const bbbp_gbt_chain* chains, const bbbp_gbt_chain* chains_device, int n_chains) {
    return fit_chains<SquaredError>("gbr_fit", stream, chains, chains_device, n_chains);
}

extern "C" int bbbp_gbt_staged_decision(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                                        const double* threshold, const double* value, const int* root, int n_trees, double init, double learning_rate,
                                        const int* stages, int n_stages, double* out) {
    BBBP_CHECK_ARG(m >= 1 && d >= 1, "gbt_staged_decision: m and d must be positive, got m %d d %d", m, d);
    BBBP_CHECK_ARG(ld >= d, "gbt_staged_decision: leading dimension %ld below d %d", ld, d);
    BBBP_CHECK_ARG(n_trees >= 1 && n_stages >= 1 && n_stages <= n_trees, "gbt_staged_decision: n_trees %d, n_stages %d: 1 <= n_stages <= n_trees must hold",
                   n_trees, n_stages);
    BBBP_CHECK_ARG(X && left && right && feature && threshold && value && root && stages && out, "gbt_staged_decision: null pointer");
    DecisionArgs a{X, ld, m, d, left, right, feature, threshold, value, root, n_trees, init, learning_rate, stages, n_stages, out};
    hipLaunchKernelGGL(gbt_decision_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
