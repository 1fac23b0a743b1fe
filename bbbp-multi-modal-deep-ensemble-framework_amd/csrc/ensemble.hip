// Device glue of the classifier stack: StackingClassifier(estimators, final_estimator=GradientBoostingClassifier(...), cv=5) and
// VotingClassifier(estimators, voting='soft') of the classification scripts (Models/model_opt.py:208-222 and its siblings).  The hot path of
// the stack is the base learners' fits, which have their own files; what is left keeps the stack's intermediate results on the device, and
// a numpy restatement (tests/ensemble_numpy.py) pins it bit for bit.  Each entry is one launch, however many estimators and folds there are.
//
//   meta_scatter   one table entry per (estimator, fold): lane i of the entry's blocks copies src[i * stride + col] to
//                  meta[rows[i]][dst] (rows NULL: row i, which is `transform`).  The folds partition the rows, so every cell of the M
//                  columns has exactly one writer: nothing is cleared, nothing is added, no atomics.  The host checks the partition and
//                  every row id before the launch; the kernel has no bounds check of its own.
//   soft_vote      one lane per row: s = P_0 (* w_0); s = s + P_j (* w_j) for j = 1 .. M - 1 in estimator order; s / scl (s / M without
//                  weights) -- numpy's np.average over the estimator axis, every product, sum and the quotient rounded once.  The label
//                  byte is numpy's argmax of the two averages: the first maximum, a NaN counting as one.
//   hard_vote      one lane per row: c_k = sum over j in estimator order of w_j (1.0 without weights) where estimator j predicts class k,
//                  in float64 from 0.0, as np.bincount(weights=) adds them; the label byte is the first maximum.
// No fused multiply-add: the file is compiled with -ffp-contract=off and the operations are written with the *_rn intrinsics.  Loads and
// stores are one element per lane (two adjacent doubles for a probability pair), so any base alignment and row stride are fine.
#include <vector>

#include "common.h"
#include "bbbp_hip.h"

namespace {

constexpr int ENS_THREADS = 256;

__global__ __launch_bounds__(ENS_THREADS) void ens_meta_scatter_kernel(const bbbp_ens_source* table, double* meta, long ld) {
    const bbbp_ens_source e = table[blockIdx.y];                                  // uniform over the block
    const long i = (long)blockIdx.x * ENS_THREADS + threadIdx.x;
    if (i >= e.count) return;
    const long row = e.rows ? e.rows[i] : i;
    meta[(size_t)row * (size_t)ld + (size_t)e.dst] = e.src[(size_t)i * (size_t)e.stride + (size_t)e.col];
}

__global__ __launch_bounds__(ENS_THREADS) void ens_soft_vote_kernel(const bbbp_ens_column* cols, int M, const double* w, double scl, int m, double* out,
                                                                    unsigned char* label) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * ENS_THREADS + threadIdx.x;
    if (i >= m) return;
    double s0 = 0.0, s1 = 0.0;
    for (int j = 0; j < M; ++j) {
        const bbbp_ens_column c = cols[j];                                        // the same address in every lane
        const double* p = static_cast<const double*>(c.src) + (size_t)i * (size_t)c.stride + (size_t)c.col;
        double p0 = p[0], p1 = p[1];
        if (w) {
            const double wj = w[j];
            p0 = __dmul_rn(p0, wj);
            p1 = __dmul_rn(p1, wj);
        }
        s0 = j ? __dadd_rn(s0, p0) : p0;                                          // the first term is taken as it is: no 0.0 + P_0 (-0.0 stays -0.0)
        s1 = j ? __dadd_rn(s1, p1) : p1;
    }
    s0 = __ddiv_rn(s0, scl);
    s1 = __ddiv_rn(s1, scl);
    out[2 * (size_t)i] = s0;
    out[2 * (size_t)i + 1] = s1;
    label[i] = (s1 > s0 || (s1 != s1 && s0 == s0)) ? 1 : 0;
}

__global__ __launch_bounds__(ENS_THREADS) void ens_hard_vote_kernel(const bbbp_ens_column* cols, int M, const double* w, int m, double* counts,
                                                                    unsigned char* label) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * ENS_THREADS + threadIdx.x;
    if (i >= m) return;
    double c0 = 0.0, c1 = 0.0;
    for (int j = 0; j < M; ++j) {
        const bbbp_ens_column c = cols[j];
        const unsigned char pred = static_cast<const unsigned char*>(c.src)[(size_t)i * (size_t)c.stride + (size_t)c.col];
        const double wj = w ? w[j] : 1.0;
        if (pred) c1 = __dadd_rn(c1, wj);
        else c0 = __dadd_rn(c0, wj);
    }
    counts[2 * (size_t)i] = c0;
    counts[2 * (size_t)i + 1] = c1;
    label[i] = (c1 > c0 || (c1 != c1 && c0 == c0)) ? 1 : 0;
}

// The M columns of a vote, checked on the host: `width` adjacent elements are read per row
int check_columns(const char* who, const bbbp_ens_column* cols, const void* cols_dev, int n_estimators, int m, int width) {
    BBBP_CHECK_ARG(n_estimators >= 1 && n_estimators <= BBBP_ENS_MAX_ESTIMATORS, "%s: n_estimators %d outside 1 .. %d", who, n_estimators,
                   BBBP_ENS_MAX_ESTIMATORS);
    BBBP_CHECK_ARG(m >= 0, "%s: m %d must not be negative", who, m);
    BBBP_CHECK_ARG(cols && cols_dev, "%s: null column table", who);
    for (int j = 0; j < n_estimators; ++j) {
        BBBP_CHECK_ARG(cols[j].src || m == 0, "%s: column %d: null source", who, j);
        BBBP_CHECK_ARG(cols[j].col >= 0 && cols[j].stride >= cols[j].col + width, "%s: column %d: row stride %ld below column offset %ld + %d", who, j,
                       cols[j].stride, cols[j].col, width);
    }
    return BBBP_OK;
}

}  // namespace

extern "C" int bbbp_ens_meta_scatter(void* stream, const bbbp_ens_source* table, const void* table_dev, int n_entries, const long* rows_host, int n,
                                     int n_columns, double* meta, long ld) {
    BBBP_CHECK_ARG(n_entries >= 1 && n_entries <= BBBP_ENS_MAX_ENTRIES, "ens_meta_scatter: n_entries %d outside 1 .. %d", n_entries, BBBP_ENS_MAX_ENTRIES);
    BBBP_CHECK_ARG(n >= 0 && n_columns >= 1, "ens_meta_scatter: n %d must not be negative and n_columns %d must be positive", n, n_columns);
    BBBP_CHECK_ARG(ld >= n_columns, "ens_meta_scatter: leading dimension %ld below n_columns %d", ld, n_columns);
    BBBP_CHECK_ARG(table && table_dev, "ens_meta_scatter: null table");
    BBBP_CHECK_ARG(meta || n == 0, "ens_meta_scatter: null destination");
    // every cell of the n_columns columns gets exactly one writer: counted here, on the host's copy of the row ids
    std::vector<unsigned char> seen((size_t)n * (size_t)n_columns, 0);
    long max_count = 0;
    const long* ids = rows_host;
    for (int e = 0; e < n_entries; ++e) {
        const bbbp_ens_source& s = table[e];
        BBBP_CHECK_ARG(s.count >= 0 && s.count <= n, "ens_meta_scatter: entry %d: count %ld outside 0 .. %d", e, s.count, n);
        BBBP_CHECK_ARG(s.dst >= 0 && s.dst < n_columns, "ens_meta_scatter: entry %d: destination column %ld outside 0 .. %d", e, s.dst, n_columns - 1);
        BBBP_CHECK_ARG(s.col >= 0 && s.stride >= s.col + 1, "ens_meta_scatter: entry %d: row stride %ld below column offset %ld + 1", e, s.stride, s.col);
        BBBP_CHECK_ARG(s.src || s.count == 0, "ens_meta_scatter: entry %d: null source", e);
        BBBP_CHECK_ARG(!s.rows || rows_host, "ens_meta_scatter: entry %d has row ids on the device but the host's copy is missing", e);
        for (long i = 0; i < s.count; ++i) {
            const long row = s.rows ? ids[i] : i;
            BBBP_CHECK_ARG(row >= 0 && row < n, "ens_meta_scatter: entry %d: row id %ld outside 0 .. %d", e, row, n - 1);
            unsigned char& cell = seen[(size_t)row * (size_t)n_columns + (size_t)s.dst];
            BBBP_CHECK_ARG(!cell, "ens_meta_scatter: entry %d: row %ld of column %ld is written twice (the folds do not partition the rows)", e, row, s.dst);
            cell = 1;
        }
        if (s.rows) ids += s.count;
        if (s.count > max_count) max_count = s.count;
    }
    for (size_t c = 0; c < seen.size(); ++c)
        BBBP_CHECK_ARG(seen[c], "ens_meta_scatter: row %ld of column %ld is never written (the folds do not partition the rows)", (long)(c / n_columns),
                       (long)(c % n_columns));
    if (n == 0) return BBBP_OK;
    hipLaunchKernelGGL(ens_meta_scatter_kernel, dim3((unsigned)cdiv((int)max_count, ENS_THREADS), (unsigned)n_entries), dim3(ENS_THREADS), 0,
                       static_cast<hipStream_t>(stream), static_cast<const bbbp_ens_source*>(table_dev), meta, ld);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_ens_soft_vote(void* stream, const bbbp_ens_column* cols, const void* cols_dev, int n_estimators, const double* weights, double scl,
                                  int m, double* out, unsigned char* label) {
    if (int rc = check_columns("ens_soft_vote", cols, cols_dev, n_estimators, m, 2)) return rc;
    BBBP_CHECK_ARG((out && label) || m == 0, "ens_soft_vote: null output");
    if (m == 0) return BBBP_OK;
    hipLaunchKernelGGL(ens_soft_vote_kernel, dim3((unsigned)cdiv(m, ENS_THREADS)), dim3(ENS_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bbbp_ens_column*>(cols_dev), n_estimators, weights, weights ? scl : (double)n_estimators, m, out, label);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_ens_hard_vote(void* stream, const bbbp_ens_column* cols, const void* cols_dev, int n_estimators, const double* weights, int m,
                                  double* counts, unsigned char* label) {
    if (int rc = check_columns("ens_hard_vote", cols, cols_dev, n_estimators, m, 1)) return rc;
    BBBP_CHECK_ARG((counts && label) || m == 0, "ens_hard_vote: null output");
    if (m == 0) return BBBP_OK;
    hipLaunchKernelGGL(ens_hard_vote_kernel, dim3((unsigned)cdiv(m, ENS_THREADS)), dim3(ENS_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bbbp_ens_column*>(cols_dev), n_estimators, weights, m, counts, label);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
