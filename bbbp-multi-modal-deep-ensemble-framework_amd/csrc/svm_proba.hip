// Class probabilities for the C-SVC of svm.hip by Platt scaling, float64.
//
//   bbbp_svm_oof_decision   decision values of the rows each fold left out, read from the kernel matrix the fold problems were solved over.
//   bbbp_svm_platt_fit      libsvm's sigmoid_train (Lin, Lin and Weng's Newton method with backtracking), one work-group per problem.
//   bbbp_svm_platt_proba    libsvm's sigmoid_predict with its clip, elementwise.
//
// Out-of-fold decision.  One wavefront per held-out row i: lane l adds alpha[s] y[s] K[i][rows[s]] for s = l, l + 64, ... in ascending
// order, a butterfly adds the 64 lanes (every lane ends with the same bits), lane 0 subtracts rho and stores.  Nothing is recomputed: row i
// of the matrix is already resident, which is why one matrix serves every fold and the final fit.
// Platt fit.  The whole Newton iteration runs inside the kernel.  A pass over dec gives either the objective (one sum) or the gradient and
// Hessian (five sums); a sum is a fixed tree: per thread its elements i = tid, tid + 1024, ... in ascending order, the 64 lanes of a wave by
// a butterfly, the 16 waves in ascending order, read by every thread from LDS, so that every thread holds the same bits and takes the same
// branches with no broadcast.  The LDS slots alternate between two banks from one reduction to the next: a thread that writes a bank for
// reduction k + 2 has passed the barrier of reduction k + 1, behind which nobody reads the values of reduction k any more -- one barrier
// per pass.  This file is compiled without floating-point contraction: A dec + B rounds as a product and a sum, as the numpy restatement
// (tests/platt_numpy.py) and libsvm round it.
#include "common.h"
#include "bbbp_hip.h"
#include <math.h>

namespace {

constexpr int OOF_THREADS = 256;          // four held-out rows per work-group
constexpr int OOF_WAVES = OOF_THREADS / 64;
constexpr int OOF_BATCH = 32;             // folds per launch: their descriptors travel as kernel arguments
constexpr int PLATT_THREADS = 1024;
constexpr int PLATT_WAVES = PLATT_THREADS / 64;
constexpr int PLATT_BATCH = 64;           // problems per launch
constexpr int PLATT_MAX_ITER = 100;       // libsvm's max_iter, min_step, sigma, eps and the Armijo constant
constexpr double PLATT_MIN_STEP = 1e-10;
constexpr double PLATT_SIGMA = 1e-12;
constexpr double PLATT_EPS = 1e-5;
constexpr double PLATT_ARMIJO = 1e-4;
constexpr double PLATT_MIN_PROB = 1e-7;
constexpr int PROBA_THREADS = 256;

struct OofBatch { bbbp_svm_oof_desc f[OOF_BATCH]; };
struct PlattBatch { bbbp_svm_platt_problem p[PLATT_BATCH]; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v += __shfl_xor(v, w);
    return v;
}

// ---- out-of-fold decision values ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OOF_THREADS) void svm_oof_kernel(OofBatch batch) {
    const bbbp_svm_oof_desc& f = batch.f[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = blockIdx.x * OOF_WAVES + wave;
    if (h >= f.n_held) return;                       // the same decision in every lane of a wave; the kernel has no barrier
    const int i = f.held[h];
    if (i < 0 || i >= f.n_rows) return;
    const double* Ki = f.K + (long)i * f.ldk;
    double sum = 0.0;
    for (int s = lane; s < f.n; s += 64) {
        const int r = f.rows ? f.rows[s] : s;
        if (r >= 0 && r < f.n_rows) sum += (f.alpha[s] * f.y[s]) * Ki[r];
    }
    sum = wave_sum(sum);
    if (lane == 0) f.out[i] = sum - *f.rho;
}

// ---- Platt fit ---------------------------------------------------------------------------------------------------------------------------
// One reduction of V sums over the work-group; `bank` alternates between calls (see the file header).
template <int V>
__device__ __forceinline__ void platt_reduce(double (&v)[V], double (*red)[5][PLATT_WAVES], int& bank, int wave, int lane) {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) red[bank][k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < V; ++k) {
        double s = red[bank][k][0];
#pragma unroll
        for (int w = 1; w < PLATT_WAVES; ++w) s += red[bank][k][w];
        v[k] = s;
    }
    bank ^= 1;
}

__device__ __forceinline__ double platt_objective(const double* dec, const double* y, int n, double hi, double lo, double A, double B,
                                                  double (*red)[5][PLATT_WAVES], int& bank, int tid, int wave, int lane) {
    double v[1] = {0.0};
    for (int i = tid; i < n; i += PLATT_THREADS) {
        const double t = y[i] > 0.0 ? hi : lo;
        const double f = dec[i] * A + B;
        v[0] += f >= 0.0 ? t * f + log(1.0 + exp(-f)) : (t - 1.0) * f + log(1.0 + exp(f));
    }
    platt_reduce<1>(v, red, bank, wave, lane);
    return v[0];
}

__global__ __launch_bounds__(PLATT_THREADS) void svm_platt_kernel(PlattBatch batch) {
    __shared__ double red[2][5][PLATT_WAVES];
    __shared__ int cnt[PLATT_WAVES];
    const bbbp_svm_platt_problem& pr = batch.p[blockIdx.x];
    const double* dec = pr.dec;
    const double* y = pr.y;
    const int n = pr.n;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int bank = 0;

    int pos = 0;
    for (int i = tid; i < n; i += PLATT_THREADS) pos += y[i] > 0.0 ? 1 : 0;
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) pos += __shfl_xor(pos, w);
    if (lane == 0) cnt[wave] = pos;
    __syncthreads();
    pos = 0;
#pragma unroll
    for (int w = 0; w < PLATT_WAVES; ++w) pos += cnt[w];
    const double prior1 = (double)pos, prior0 = (double)(n - pos);
    const double hi = (prior1 + 1.0) / (prior1 + 2.0), lo = 1.0 / (prior0 + 2.0);

    double A = 0.0, B = log((prior0 + 1.0) / (prior1 + 1.0));
    double fval = platt_objective(dec, y, n, hi, lo, A, B, red, bank, tid, wave, lane);
    int iter = 0, status = BBBP_PLATT_MAX_ITER;
    for (; iter < PLATT_MAX_ITER; ++iter) {
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                 // h11, h22, h21, g1, g2
        for (int i = tid; i < n; i += PLATT_THREADS) {
            const double d = dec[i];
            const double t = y[i] > 0.0 ? hi : lo;
            const double f = d * A + B;
            double p, q;
            if (f >= 0.0) { const double e = exp(-f); p = e / (1.0 + e); q = 1.0 / (1.0 + e); }
            else { const double e = exp(f); p = 1.0 / (1.0 + e); q = e / (1.0 + e); }
            const double d2 = p * q, d1 = t - p;
            v[0] += d * d * d2;
            v[1] += d2;
            v[2] += d * d2;
            v[3] += d * d1;
            v[4] += d1;
        }
        platt_reduce<5>(v, red, bank, wave, lane);
        const double h11 = PLATT_SIGMA + v[0], h22 = PLATT_SIGMA + v[1], h21 = v[2], g1 = v[3], g2 = v[4];
        if (fabs(g1) < PLATT_EPS && fabs(g2) < PLATT_EPS) { status = BBBP_PLATT_CONVERGED; break; }
        const double det = h11 * h22 - h21 * h21;
        const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
        const double gd = g1 * dA + g2 * dB;
        double step = 1.0;
        while (step >= PLATT_MIN_STEP) {                          // at most 34 halvings: the loop ends by construction
            const double nA = A + step * dA, nB = B + step * dB;
            const double nf = platt_objective(dec, y, n, hi, lo, nA, nB, red, bank, tid, wave, lane);
            if (nf < fval + PLATT_ARMIJO * step * gd) { A = nA; B = nB; fval = nf; break; }
            step /= 2.0;
        }
        if (step < PLATT_MIN_STEP) { status = BBBP_PLATT_LINE_SEARCH; break; }
    }
    if (tid == 0) { pr.ab[0] = A; pr.ab[1] = B; pr.info[0] = iter; pr.info[1] = status; }
}

// ---- probabilities -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PROBA_THREADS) void svm_platt_proba_kernel(const double* dec, long m, double A, double B, double* proba) {
    const long q = (long)blockIdx.x * PROBA_THREADS + threadIdx.x;
    if (q >= m) return;
    const double f = dec[q] * A + B;
    double p;
    if (f >= 0.0) { const double e = exp(-f); p = e / (1.0 + e); }
    else p = 1.0 / (1.0 + exp(f));
    p = fmin(fmax(p, PLATT_MIN_PROB), 1.0 - PLATT_MIN_PROB);
    proba[2 * q] = p;
    proba[2 * q + 1] = 1.0 - p;
}

}  // namespace

extern "C" int bbbp_svm_oof_decision(void* stream, const bbbp_svm_oof_desc* folds, int n_folds) {
    BBBP_CHECK_ARG(folds != nullptr, "bbbp_svm_oof_decision: null fold list");
    BBBP_CHECK_ARG(n_folds > 0, "bbbp_svm_oof_decision: n_folds %d must be positive", n_folds);
    for (int q = 0; q < n_folds; ++q) {
        const bbbp_svm_oof_desc& f = folds[q];
        BBBP_CHECK_ARG(f.n_rows > 0, "bbbp_svm_oof_decision: fold %d: n_rows %d must be positive", q, f.n_rows);
        BBBP_CHECK_ARG(f.n > 0 && f.n <= f.n_rows, "bbbp_svm_oof_decision: fold %d: n %d must be positive and at most n_rows %d", q, f.n, f.n_rows);
        BBBP_CHECK_ARG(f.n_held >= 0 && f.n_held <= f.n_rows, "bbbp_svm_oof_decision: fold %d: n_held %d must lie in [0, n_rows %d]", q, f.n_held,
                       f.n_rows);
        BBBP_CHECK_ARG(f.K && f.y && f.alpha && f.rho && f.out && (f.held || f.n_held == 0), "bbbp_svm_oof_decision: fold %d: null pointer", q);
        BBBP_CHECK_ARG(f.ldk >= f.n_rows, "bbbp_svm_oof_decision: fold %d: leading dimension %ld below n_rows %d", q, f.ldk, f.n_rows);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int q0 = 0; q0 < n_folds; q0 += OOF_BATCH) {
        const int nb = n_folds - q0 < OOF_BATCH ? n_folds - q0 : OOF_BATCH;
        OofBatch b = {};
        int most = 0;
        for (int q = 0; q < nb; ++q) { b.f[q] = folds[q0 + q]; most = folds[q0 + q].n_held > most ? folds[q0 + q].n_held : most; }
        if (most == 0) continue;
        hipLaunchKernelGGL(svm_oof_kernel, dim3((unsigned)cdiv(most, OOF_WAVES), (unsigned)nb), dim3(OOF_THREADS), 0, st, b);
        BBBP_CHECK_LAUNCH();
    }
    return BBBP_OK;
}

extern "C" int bbbp_svm_platt_fit(void* stream, const bbbp_svm_platt_problem* problems, int n_problems) {
    BBBP_CHECK_ARG(problems != nullptr, "bbbp_svm_platt_fit: null problem list");
    BBBP_CHECK_ARG(n_problems > 0, "bbbp_svm_platt_fit: n_problems %d must be positive", n_problems);
    for (int q = 0; q < n_problems; ++q) {
        const bbbp_svm_platt_problem& p = problems[q];
        BBBP_CHECK_ARG(p.n > 0, "bbbp_svm_platt_fit: problem %d: n %d must be positive", q, p.n);
        BBBP_CHECK_ARG(p.dec && p.y && p.ab && p.info, "bbbp_svm_platt_fit: problem %d: null pointer", q);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int q0 = 0; q0 < n_problems; q0 += PLATT_BATCH) {
        const int nb = n_problems - q0 < PLATT_BATCH ? n_problems - q0 : PLATT_BATCH;
        PlattBatch b = {};
        for (int q = 0; q < nb; ++q) b.p[q] = problems[q0 + q];
        hipLaunchKernelGGL(svm_platt_kernel, dim3((unsigned)nb), dim3(PLATT_THREADS), 0, st, b);
        BBBP_CHECK_LAUNCH();
    }
    return BBBP_OK;
}

extern "C" int bbbp_svm_platt_proba(void* stream, const double* dec, long m, double A, double B, double* proba) {
    BBBP_CHECK_ARG(m >= 0, "bbbp_svm_platt_proba: m %ld must not be negative", m);
    BBBP_CHECK_ARG(A == A && B == B && fabs(A) <= 1.79769313486231570815e+308 && fabs(B) <= 1.79769313486231570815e+308,
                   "bbbp_svm_platt_proba: A %g and B %g must be finite", A, B);
    if (m == 0) return BBBP_OK;
    BBBP_CHECK_ARG(dec && proba, "bbbp_svm_platt_proba: null pointer");
    const long blocks = (m + PROBA_THREADS - 1) / PROBA_THREADS;
    BBBP_CHECK_ARG(blocks <= 0x7fffffffL, "bbbp_svm_platt_proba: m %ld exceeds the grid", m);
    hipLaunchKernelGGL(svm_platt_proba_kernel, dim3((unsigned)blocks), dim3(PROBA_THREADS), 0, static_cast<hipStream_t>(stream), dec, m, A, B, proba);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
