// Isolation forest, fitted and walked on the GPU: IsolationForest(contamination=0.05, random_state=42) of the regression stack's preprocessing
// (Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest*.py), the step behind PCA.  scikit-learn's rule
// (ensemble/_iforest.py over ExtraTreeRegressor(max_features=1, splitter="random")), restated: a tree takes max_samples distinct rows; a node
// is a leaf with fewer than two rows, at depth ceil(log2(max_samples)) or when every feature is constant on its rows (float32 max <= min +
// 1e-7f); otherwise one feature is drawn uniformly among the features that are not constant and the threshold uniformly in [min, max).
// scikit-learn's further stop on the impurity of its random target has no counterpart: a tree here has no target.
//
// Random numbers are the forests' counter-based hash (rf_hash, tree_fit.h) under a tag of their own; include/bbbp_hip.h states the keys.  A
// tree's rows are the max_samples rows with the lowest hash: the hash is a bijection of the row index, so the max_samples-th lowest value is
// found by a radix select (eight passes over the n hashes, one byte each, a 256-bin histogram in LDS) and the rows below it are compacted in
// ascending order.  The uniform feature draw is a hashed order of the features, tried until one is not constant.
//
// One work-group of 256 threads grows one tree, all levels in one launch, everything in LDS: the row permutation (a node's rows are a
// contiguous segment of it), every position's slot in the level's node table (IF_DEAD once the row sits in a leaf) and the tables of this
// level and the next (start, count, node number, key).  One level:
//   open       a node with two rows or more above max_depth is open, the others are leaves
//   try        every open node takes the next feature of its hashed order; one segmented min / max scan over the positions (passes of 256, rows
//              gathered from X) tells at each segment's last position whether the feature is constant; if not the node splits at the drawn
//              threshold, else it stays open for the next try; a node that runs out of features is a leaf
//   number     the split nodes' ranks (block_rank_before over the table) number the children level by level
//   partition  every split segment stably by side (block_rank_before over the positions), rows of leaves stay where they are; the next table
// The threshold's three float64 operations are rounded one by one (the file is compiled with -ffp-contract=off), so tests/iforest_numpy.py
// reproduces a fit bit for bit.
#include "common.h"
#include "bbbp_hip.h"
#include "tree_fit.h"

#include <math.h>

namespace {

constexpr int IF_THREADS = 256;
constexpr unsigned long long IF_TAG = 0x1F0BE57ull;          // keeps these streams apart from the forests': key(root) = hash(hash(seed, IF_TAG), tree)
constexpr unsigned long long IF_SAMPLE = 0x5A3B1Eull;        // the stream of a tree's row hashes
constexpr unsigned long long IF_THRESHOLD = 0x7412E5ull;     // a node's threshold draw; features use 2 + f <= 1025, sides 0 and 1
constexpr unsigned IF_DEAD = 0xffffu;                        // slot of a row that is in no node of the level
constexpr int IF_LEAF = 0, IF_OPEN = 1, IF_SPLIT = 2;
constexpr float IF_FEATURE_THRESHOLD = 1e-7f;
static_assert(BBBP_IFOREST_MAX_SAMPLES < (int)IF_DEAD && BBBP_IFOREST_MAX_SAMPLES % IF_THREADS == 0, "slots are 16 bits, passes are whole");
static_assert(2 + BBBP_IFOREST_MAX_D < 0x10000, "feature counters stay below the tags");

__host__ __device__ inline int tree_capacity(int S) { return 2 * S - 1; }
__host__ __device__ inline int depth_limit(int S) {          // ceil(log2(max(S, 2)))
    int depth = 1;
    while ((1 << depth) < S) ++depth;
    return depth;
}

struct Lds {                                  // offsets into the work-group's dynamic LDS, in bytes; all multiples of 16
    size_t perm_a, perm_b, slot_a, slot_b, start_a, start_b, cnt_a, cnt_b, node_a, node_b, key_a, key_b;
    size_t state, feat, prevh, thr, srank, lbase, lend, rank, total;
};
__host__ __device__ inline Lds lds_layout(int S) {
    Lds w;
    Area a;
    const size_t N = (size_t)S;
    w.perm_a = a.take(N * 4); w.perm_b = a.take(N * 4); w.slot_a = a.take(N * 2); w.slot_b = a.take(N * 2);
    w.start_a = a.take(N * 4); w.start_b = a.take(N * 4); w.cnt_a = a.take(N * 4); w.cnt_b = a.take(N * 4);
    w.node_a = a.take(N * 4); w.node_b = a.take(N * 4); w.key_a = a.take(N * 8); w.key_b = a.take(N * 8);
    w.state = a.take(N * 4); w.feat = a.take(N * 4); w.prevh = a.take(N * 8); w.thr = a.take(N * 8);
    w.srank = a.take(N * 4); w.lbase = a.take(N * 4); w.lend = a.take(N * 4); w.rank = a.take(N * 4);
    w.total = a.at;
    return w;
}

struct MinMax { float lo, hi; };
__device__ inline MinMax lane_up(MinMax v, int off) { return MinMax{__shfl_up(v.lo, off), __shfl_up(v.hi, off)}; }
__device__ inline MinMax mm_add(MinMax a, MinMax b) { return MinMax{fminf(a.lo, b.lo), fmaxf(a.hi, b.hi)}; }

// thr = lo + (hi - lo) u in float64, u in [0, 1) from the hash's upper 53 bits: three roundings, none fused; a threshold that reaches hi
// (the sum can round up to it) falls back to lo, so that both sides keep a row
__device__ inline double draw_threshold(unsigned long long key, float lo, float hi) {
#pragma clang fp contract(off)
    const double u = (double)(rf_hash(key, IF_THRESHOLD) >> 11) * 0x1p-53;          // exact: 53 bits and a power of two
    const double l = (double)lo, h = (double)hi;
    const double span = h - l;
    const double step = span * u;
    double thr = l + step;
    if (thr >= h) thr = l;
    return thr;
}

struct FitArgs {
    const float* X; long ld; int n, d, S, max_depth, cap; unsigned long long seed;
    int *left, *right, *feature, *nns; double* threshold; int* samples; int* n_nodes;
};
struct NodeArrays { int *left, *right, *feature; double* threshold; };          // one tree's slots, for make_leaf
struct Shared { unsigned long long prefix; int want, open, error; };

__global__ __launch_bounds__(IF_THREADS) void iforest_fit_kernel(FitArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n, d = a.d, S = a.S;
    const long t_at = (long)blockIdx.x;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Lds w = lds_layout(S);
    int *perm = (int*)(smem + w.perm_a), *perm_next = (int*)(smem + w.perm_b);
    uint16_t *slot = (uint16_t*)(smem + w.slot_a), *slot_next = (uint16_t*)(smem + w.slot_b);
    int *start = (int*)(smem + w.start_a), *start_next = (int*)(smem + w.start_b), *cnt = (int*)(smem + w.cnt_a), *cnt_next = (int*)(smem + w.cnt_b);
    int *tnode = (int*)(smem + w.node_a), *tnode_next = (int*)(smem + w.node_b);
    unsigned long long *tkey = (unsigned long long*)(smem + w.key_a), *tkey_next = (unsigned long long*)(smem + w.key_b);
    int *state = (int*)(smem + w.state), *feat = (int*)(smem + w.feat), *srank = (int*)(smem + w.srank), *lbase = (int*)(smem + w.lbase);
    int *lend = (int*)(smem + w.lend), *rank = (int*)(smem + w.rank);
    unsigned long long* prevh = (unsigned long long*)(smem + w.prevh);
    double* thr = (double*)(smem + w.thr);
    __shared__ int hist[256], wave_cnt[2][4], wave_flag[4];
    __shared__ MinMax wave_val[4], carry_s;
    __shared__ Shared sh;

    const NodeArrays out{a.left + t_at * a.cap, a.right + t_at * a.cap, a.feature + t_at * a.cap, a.threshold + t_at * a.cap};
    int* nns = a.nns + t_at * a.cap;
    int* samples = a.samples + t_at * S;
    const unsigned long long key0 = rf_hash(rf_hash(a.seed, IF_TAG), (unsigned long long)blockIdx.x);
    const unsigned long long stream = rf_hash(key0, IF_SAMPLE);
    if (tid == 0) sh.error = 0;

    // ---- the tree's rows: the S-th lowest hash by radix select, one byte per pass from the top ----
    unsigned long long prefix = 0ull;
    int want = S;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (long i = tid; i < n; i += IF_THREADS) {
            const unsigned long long h = rf_hash(stream, (unsigned long long)i);
            if (shift == 56 || (h >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((h >> shift) & 255ull)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0, digit = 0;
            for (; digit < 255; ++digit) {
                if (acc + hist[digit] >= want) break;
                acc += hist[digit];
            }
            sh.prefix = (prefix << 8) | (unsigned long long)digit;
            sh.want = want - acc;
        }
        __syncthreads();
        prefix = sh.prefix;
        want = sh.want;
    }
    // the rows at or below it, in ascending order: exactly S of them
    int taken = 0;
    int it = 0;
    for (long base = 0; base < n; base += IF_THREADS, ++it) {
        const long i = base + tid;
        const bool in = i < n && rf_hash(stream, (unsigned long long)i) <= prefix;
        const int r = block_rank_before(in, wave_cnt[it & 1], taken);
        if (in) {
            if (r < S) { perm[r] = (int)i; slot[r] = 0; samples[r] = (int)i; }
            else sh.error = 1;
        }
    }
    if (taken != S) sh.error = 1;
    if (tid == 0) { start[0] = 0; cnt[0] = S; tnode[0] = 0; tkey[0] = key0; }
    __syncthreads();
    if (sh.error) {                                         // uniform: read behind the barrier, written in front of it
        if (tid == 0) a.n_nodes[t_at] = -1;
        return;
    }

    // ---- the levels ----
    int nk = 1, total = 1;
    for (int level = 0;; ++level) {
        for (int k = tid; k < nk; k += IF_THREADS) {
            const int m = cnt[k];
            nns[tnode[k]] = m;
            state[k] = (m >= 2 && level < a.max_depth) ? IF_OPEN : IF_LEAF;
            feat[k] = -1;
            prevh[k] = 0ull;
        }
        __syncthreads();
        for (int attempt = 0; attempt <= d; ++attempt) {
            if (tid == 0) { sh.open = 0; carry_s = MinMax{0.0f, 0.0f}; }
            __syncthreads();
            for (int k = tid; k < nk; k += IF_THREADS) {
                if (state[k] != IF_OPEN) continue;
                // the next feature of the node's hashed order: the lowest hash above the last one tried
                const unsigned long long key = tkey[k], prev = prevh[k];
                const bool first = feat[k] < 0;
                unsigned long long best = 0ull;
                int bf = -1;
                for (int f = 0; f < d; ++f) {
                    const unsigned long long h = rf_hash(key, 2ull + (unsigned long long)f);
                    if ((first || h > prev) && (bf < 0 || h < best)) { best = h; bf = f; }
                }
                if (bf < 0) state[k] = IF_LEAF;               // every feature is constant on its rows
                else { feat[k] = bf; prevh[k] = best; sh.open = 1; }
            }
            __syncthreads();
            if (!sh.open) break;                            // uniform
            // segmented min / max of every open node's feature over its rows
            for (int base = 0; base < S; base += IF_THREADS) {
                const int p = base + tid;
                const unsigned k = p < S ? slot[p] : IF_DEAD;
                bool act = false;
                int s = 0, m = 0;
                MinMax x{0.0f, 0.0f};
                if (k != IF_DEAD) {
                    if (k >= (unsigned)nk) sh.error = 1;
                    else if (state[k] == IF_OPEN) {
                        s = start[k]; m = cnt[k];
                        act = p >= s && p - s < m;
                        if (!act) sh.error = 1;
                    }
                }
                if (act) {
                    const float v = a.X[(long)row_of(perm, p, n, &sh) * a.ld + feat[k]];
                    x = MinMax{v, v};
                }
                const MinMax carry = carry_s;               // the inclusive minimum / maximum at position base - 1, inside its segment
                const auto add = [](MinMax own, MinMax earlier) { return mm_add(own, earlier); };
                MinMax val = x;
                int flg = (!act || p == s) ? 1 : 0;
                wave_segmented_scan(val, flg, add);
                if (lane == 63) { wave_val[wave] = val; wave_flag[wave] = flg; }
                __syncthreads();
                if (!flg) val = mm_add(val, block_segment_prefix(carry, wave_val, wave_flag, add));
                if (tid == IF_THREADS - 1) carry_s = val;
                if (act && p + 1 == s + m && val.hi > val.lo + IF_FEATURE_THRESHOLD) {          // the segment's last position decides
                    state[k] = IF_SPLIT;
                    thr[k] = draw_threshold(tkey[k], val.lo, val.hi);
                }
                __syncthreads();
            }
        }
        // ---- number: the children of the level's split nodes, in table order ----
        int n_split = 0;
        it = 0;
        for (int base = 0; base < nk; base += IF_THREADS, ++it) {
            const int k = base + tid;
            const bool sp = k < nk && state[k] == IF_SPLIT;
            const int r = block_rank_before(sp, wave_cnt[it & 1], n_split);
            if (k < nk) {
                const int node = tnode[k];
                if (sp) {
                    srank[k] = r;
                    out.left[node] = total + 2 * r; out.right[node] = total + 2 * r + 1; out.feature[node] = feat[k]; out.threshold[node] = thr[k];
                } else make_leaf(out, node);
            }
        }
        __syncthreads();
        if (n_split == 0) break;
        if (2 * n_split > S || total + 2 * n_split > a.cap) { if (tid == 0) sh.error = 1; break; }      // uniform; cannot happen: split nodes hold two rows each
        // ---- partition: every split segment stably by side ----
        int before = 0;
        it = 0;
        for (int base = 0; base < S; base += IF_THREADS, ++it) {
            const int p = base + tid;
            const unsigned k = p < S ? slot[p] : IF_DEAD;
            const bool moving = k < (unsigned)nk && state[k] == IF_SPLIT;
            bool left = false;
            if (moving) left = (double)a.X[(long)row_of(perm, p, n, &sh) * a.ld + feat[k]] <= thr[k];
            const int r = block_rank_before(left, wave_cnt[it & 1], before);
            if (p < S) rank[p] = 2 * r + (left ? 1 : 0);
            if (moving) {
                const int s = start[k], m = cnt[k];
                if (p == s) lbase[k] = r;
                if (p + 1 == s + m) lend[k] = r + (left ? 1 : 0);
            }
        }
        __syncthreads();
        for (int p = tid; p < S; p += IF_THREADS) {
            const unsigned k = slot[p];
            int to = p;                                     // a row of a leaf stays where it is
            unsigned ns = IF_DEAD;
            if (k < (unsigned)nk && state[k] == IF_SPLIT) {
                const int s = start[k], nl = lend[k] - lbase[k], in_seg = (rank[p] >> 1) - lbase[k];          // rows of this segment going left in front of p
                const bool left = rank[p] & 1;
                to = left ? s + in_seg : s + nl + (p - s - in_seg);
                ns = 2u * (unsigned)srank[k] + (left ? 0u : 1u);
            }
            if ((unsigned)to < (unsigned)S) { perm_next[to] = perm[p]; slot_next[to] = (uint16_t)ns; }
            else sh.error = 1;
        }
        for (int k = tid; k < nk; k += IF_THREADS) {
            if (state[k] != IF_SPLIT) continue;
            const int r = srank[k], s = start[k], m = cnt[k];
            int nl = lend[k] - lbase[k];
            if (nl < 1 || nl >= m) { sh.error = 1; nl = 1; }          // cannot happen: the minimum goes left, the maximum right
            const unsigned long long key = tkey[k];
            start_next[2 * r] = s; cnt_next[2 * r] = nl; tnode_next[2 * r] = total + 2 * r; tkey_next[2 * r] = rf_hash(key, 0ull);
            start_next[2 * r + 1] = s + nl; cnt_next[2 * r + 1] = m - nl; tnode_next[2 * r + 1] = total + 2 * r + 1; tkey_next[2 * r + 1] = rf_hash(key, 1ull);
        }
        __syncthreads();
        { int* q = perm; perm = perm_next; perm_next = q; }
        { uint16_t* q = slot; slot = slot_next; slot_next = q; }
        { int* q = start; start = start_next; start_next = q; }
        { int* q = cnt; cnt = cnt_next; cnt_next = q; }
        { int* q = tnode; tnode = tnode_next; tnode_next = q; }
        { unsigned long long* q = tkey; tkey = tkey_next; tkey_next = q; }
        total += 2 * n_split;
        nk = 2 * n_split;
        if (sh.error) break;                                // uniform: behind the barrier
    }
    __syncthreads();
    if (tid == 0) a.n_nodes[t_at] = sh.error ? -1 : total;
}

// ---- path sums: every query row walks every tree; the leaves' terms are summed in tree order ------------------------------------------------
struct PathArgs {
    const float* X; long ld; int m, d;
    const int *left, *right, *feature; const double *threshold, *term; const int* root;
    int n_trees; double* out;
};
__global__ __launch_bounds__(256) void iforest_path_sum_kernel(PathArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const float* x = a.X + (long)i * a.ld;
    double s = 0.0;
    for (int t = 0; t < a.n_trees; ++t) {
        int node = a.root[t], steps = 0;
        int l = a.left[node];
        // bounded: arrays handed to the C ABI directly cannot spin a wave for ever
        while (l >= 0 && steps < BBBP_RF_MAX_WALK) {
            node = (double)x[a.feature[node]] <= a.threshold[node] ? l : a.right[node];
            l = a.left[node];
            ++steps;
        }
        s = l >= 0 ? __builtin_nan("") : s + a.term[node];
    }
    a.out[i] = s;
}

bool check_samples(const char* who, int S) {
    if (S >= 1 && S <= BBBP_IFOREST_MAX_SAMPLES) return true;
    bbbp_set_error("%s: max_samples %d outside 1..BBBP_IFOREST_MAX_SAMPLES %d", who, S, BBBP_IFOREST_MAX_SAMPLES);
    return false;
}

}  // namespace

extern "C" int bbbp_iforest_tree_capacity(int max_samples) {
    return check_samples("iforest_tree_capacity", max_samples) ? tree_capacity(max_samples) : 0;
}

extern "C" size_t bbbp_iforest_work_bytes(int max_samples) {
    return check_samples("iforest_work_bytes", max_samples) ? lds_layout(max_samples).total : 0;
}

extern "C" int bbbp_iforest_fit(void* stream, const float* X, long ld, int n, int d, int max_samples, int n_trees, unsigned long long seed,
                                int* left, int* right, int* feature, int* n_node_samples, double* threshold, int* samples,
                                int* n_nodes) {
    BBBP_CHECK_ARG(n >= 1 && d >= 1, "iforest_fit: n >= 1 and d >= 1 must hold, got n %d d %d", n, d);
    BBBP_CHECK_ARG(n <= BBBP_IFOREST_MAX_N, "iforest_fit: n %d exceeds BBBP_IFOREST_MAX_N %d", n, BBBP_IFOREST_MAX_N);
    BBBP_CHECK_ARG(d <= BBBP_IFOREST_MAX_D, "iforest_fit: d %d exceeds BBBP_IFOREST_MAX_D %d", d, BBBP_IFOREST_MAX_D);
    BBBP_CHECK_ARG(ld >= d, "iforest_fit: leading dimension %ld below d %d", ld, d);
    BBBP_CHECK_ARG(max_samples >= 1 && max_samples <= BBBP_IFOREST_MAX_SAMPLES, "iforest_fit: max_samples %d outside 1..BBBP_IFOREST_MAX_SAMPLES %d",
                   max_samples, BBBP_IFOREST_MAX_SAMPLES);
    BBBP_CHECK_ARG(max_samples <= n, "iforest_fit: max_samples %d above n %d", max_samples, n);
    BBBP_CHECK_ARG(n_trees >= 1 && n_trees <= 65535, "iforest_fit: n_trees %d outside 1..65535", n_trees);
    BBBP_CHECK_ARG(X && left && right && feature && n_node_samples && threshold && samples && n_nodes, "iforest_fit: null pointer");
    const size_t lds = lds_layout(max_samples).total;
    if (int rc = bbbp_ensure_dyn_lds(reinterpret_cast<const void*>(iforest_fit_kernel), lds)) return rc;
    FitArgs a{X, ld, n, d, max_samples, depth_limit(max_samples), tree_capacity(max_samples), seed, left, right, feature, n_node_samples,
              threshold, samples, n_nodes};
    hipLaunchKernelGGL(iforest_fit_kernel, dim3((unsigned)n_trees), dim3(IF_THREADS), lds, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_iforest_path_sum(void* stream, const float* X, long ld, int m, int d, const int* left, const int* right, const int* feature,
                                     const double* threshold, const double* term, const int* root, int n_trees, double* out) {
    BBBP_CHECK_ARG(m >= 1 && d >= 1, "iforest_path_sum: m and d must be positive, got m %d d %d", m, d);
    BBBP_CHECK_ARG(ld >= d, "iforest_path_sum: leading dimension %ld below d %d", ld, d);
    BBBP_CHECK_ARG(n_trees >= 1, "iforest_path_sum: n_trees %d must be >= 1", n_trees);
    BBBP_CHECK_ARG(X && left && right && feature && threshold && term && root && out, "iforest_path_sum: null pointer");
    PathArgs a{X, ld, m, d, left, right, feature, threshold, term, root, n_trees, out};
    hipLaunchKernelGGL(iforest_path_sum_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
