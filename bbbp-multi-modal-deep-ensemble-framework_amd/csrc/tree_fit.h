// What the level-by-level tree fits share (rf.hip: forests, node tables by slot in global memory; gbt.hip: boosted chains, 2^depth keys):
// inline device functions only, no kernel and no state.  Both fits keep every feature's row order partitioned into the level's nodes, score
// the positions of a feature with a segmented scan in passes of 256 positions (four waves of 64) and partition the orders stably by side.
//   Area                  offsets into a work area, every one a multiple of 16 bytes
//   row_of                a row index read from an order array, kept inside [0, n)
//   block_rank_before     the stable partition's rank: how many positions in front of this one carry the flag, across passes
//   wave_segmented_scan   the inclusive scan inside a wave, restarting where a flag is set; block_segment_prefix: what the waves in front add
//   encode_score          a non-negative score's bits as an integer that orders like the score, 0 kept for "none"
//   split_threshold       scikit-learn's threshold between two feature values
//   rf_hash               the counter-based hash of the forests' random choices (rf.hip, iforest.hip)
//   make_leaf             the four stores that make a node a leaf
// The scans take their values, their flags and their addition from the kernel: when a segment starts and what is summed differ per kernel,
// and the order of every addition is the kernel's (a float64 scan's result depends on it).  The tree walkers, the `choose` kernels and the
// node tables are per file on purpose: they share a shape, not code.  iforest.hip (isolation trees, one work-group per tree, everything in
// LDS) takes the scans for its segmented minimum / maximum, block_rank_before for its compaction and partition, make_leaf and the hash.
// xgb.hip (histogram-boosted trees over byte features: one row list per problem instead of an order per feature, integer histograms instead
// of float64 scans) takes Area, row_of and block_rank_before (the ranks of the splits and of the next level's slots in its `choose`); its
// leaf stores are its own, XGBoost's node arrays being others than scikit-learn's.  cat.hip (boosted symmetric trees over the same byte
// features: one split per level for all parts, a part table instead of nodes) takes Area, row_of and block_rank_before (the compaction of
// the children that hold a row in its `partition`).
// Members of a struct that are selected by a run-time index or address go to scratch: layouts here are filled member by member.
#pragma once
#include "common.h"

namespace {

struct Area {
    size_t at = 0;
    __host__ __device__ inline size_t take(size_t bytes) { const size_t o = at; at += (bytes + 15) / 16 * 16; return o; }
};

// A row index read from an order array, kept inside [0, n): a wrong order never gives a wild address.  It cannot happen while the kernels are
// right; if it does, the fit's error word is set (every writer stores the same 1) and the fit reports it instead of a node count
template <class Index, class State> __device__ inline int row_of(const Index* src, int p, int n, State* st) {
    const int i = src[p];
    if ((unsigned)i < (unsigned)n) return i;
    st->error = 1;
    return 0;
}

// The number of positions in front of this thread's, in this pass and in all earlier ones, whose `flag` is set: where a stable partition puts
// the row.  Work-groups of 256 threads; `wave_cnt` is the pass's row of a `__shared__ int[2][4]` (rows alternate from pass to pass, so one
// barrier per pass is enough); `running` is the total of the earlier passes and takes this one's.  Every thread of the group calls it.
__device__ inline int block_rank_before(bool flag, int* wave_cnt, int& running) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ballot = __ballot(flag);
    if (lane == 0) wave_cnt[wave] = __popcll(ballot);
    __syncthreads();
    int rank = running + __popcll(ballot & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += wave_cnt[w];
    running += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    return rank;
}

template <class T> __device__ inline T lane_up(T v, int off) { return __shfl_up(v, off); }      // a kernel's sum type brings its own overload

// Segmented inclusive scan inside the wave: on entry `flg` is 1 where a segment starts; on return `val` is the sum from the segment's start
// (or the wave's first lane) to this lane, `add(own, earlier)` at every step, and `flg` says whether a segment starts at or before this lane
template <class T, class Add> __device__ inline void wave_segmented_scan(T& val, int& flg, Add add) {
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const T pv = lane_up(val, off);
        const int pf = __shfl_up(flg, off);
        if (lane >= off) {
            if (!flg) val = add(val, pv);
            flg |= pf;
        }
    }
}
// What precedes this wave in its first segment: `carry` (the inclusive sum at the previous pass's last position) and the waves in front, whose
// last lanes left (wave_val, wave_flag); a wave that holds a segment start begins the sum again
template <class T, class Add> __device__ inline T block_segment_prefix(T carry, const T* wave_val, const int* wave_flag, Add add) {
    const int wave = threadIdx.x >> 6;
    T pre = carry;
    for (int w = 0; w < wave; ++w) pre = wave_flag[w] ? wave_val[w] : add(pre, wave_val[w]);
    return pre;
}

// scores are >= 0: their bits order as integers; 0 = none
__device__ inline unsigned long long encode_score(double score) { return (unsigned long long)__double_as_longlong(score) + 1ull; }

// scikit-learn's threshold between the feature values a < b on the two sides of a split: two divisions and one addition in float64
__device__ inline double split_threshold(float a, float b) {
    double thr = (double)a / 2.0 + (double)b / 2.0;
    if (thr == (double)b) thr = (double)a;
    return thr;
}

// The counter-based hash behind every random choice of the forests (rf.hip, iforest.hip; exported as bbbp_rf_hash): one value per (key, counter)
__host__ __device__ inline unsigned long long rf_mix(unsigned long long z) {          // the splitmix64 finaliser
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
__host__ __device__ inline unsigned long long rf_hash(unsigned long long a, unsigned long long b) {
    return rf_mix(rf_mix(a) + 0x9e3779b97f4a7c15ull * (b + 1ull));
}

template <class Desc, class Node> __device__ inline void make_leaf(const Desc& c, Node node) {
    c.left[node] = -1; c.right[node] = -1; c.feature[node] = 0; c.threshold[node] = -2.0;
}

}  // namespace
