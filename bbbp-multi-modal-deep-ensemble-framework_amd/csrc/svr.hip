// Epsilon-support-vector regression: libsvm's epsilon-SVR solver without shrinking, one work-group per problem.
//
//   bbbp_svr_smo   a bounded number of iterations per launch of every problem of a batch; the kernel matrix and the decision function
//                  are svm.hip's (bbbp_svm_kernel_matrix, bbbp_svm_decision).
//
// Problem.  2n variables over an n x n kernel matrix: variable k < n is alpha_k (sign +1, linear term epsilon - t_k), variable k + n is
// alpha*_k (sign -1, linear term epsilon + t_k), Q[k][l] = s_k s_l K[k mod n][l mod n], QD[k] = K[k mod n][k mod n].  Selection, the
// clipped pair update, tau, the stop rule and rho are libsvm's with s in the place of y.
// Ownership.  Thread `tid` owns the base rows r = tid, tid + 1024, ... and with each both of its variables r and r + n: one load of
// K_i[r] and K_j[r] serves both halves, and t = (s_i K_i[r]) d_alpha_i + (s_j K_j[r]) d_alpha_j goes to G[r] as +t and to G[r + n] as -t
// (Q_i[r + n] = -Q_i[r] exactly, so this is libsvm's G[k] += Q_i[k] d_alpha_i + Q_j[k] d_alpha_j bit for bit).
// State.  Up to SVR_REG_ROWS base rows per thread (n <= 4096) a thread keeps alpha, alpha*, G, G*, QD and the matrix row of each of its
// base rows in registers for the whole launch: read once at its start, written once at its end.  Beyond that the same loop runs on the
// state in global memory (every thread still touches only what it owns).  Nobody reads another thread's state: what the pair update
// needs of the two selected variables (alpha, G, matrix row) travels with the two arg-max reductions -- after the wave butterfly the one
// lane that owns the wave's winner puts them beside the wave's candidate in LDS.  An iteration therefore has two barriers, one per
// selection, and no global-memory round trip but the two matrix rows.
// Order.  Both selections are total orders on (value, index in the 2n ordering) that keep the LATER index among equals (k + n beats k),
// as libsvm's `>=` / `<=` scans do; the maxima of gmax2 and rho's bounds do not depend on the order; rho's sum over the free variables
// is a fixed tree: per thread its rows in ascending order (r, then r + n), the 64 lanes of a wave by a butterfly, the 16 waves in
// ascending order.  This file is compiled without floating-point contraction: every product and sum rounds on its own, as the numpy
// oracle's do, so a problem's result is bit-identical from run to run, for any launch length and whatever else is in the batch.
#include "common.h"
#include "bbbp_hip.h"
#include <math.h>

namespace {

constexpr double SVR_TAU = 1e-12;         // libsvm's curvature floor
constexpr int SVR_THREADS = 1024;
constexpr int SVR_WAVES = SVR_THREADS / 64;
constexpr int SVR_REG_ROWS = 4;           // base rows per thread whose state stays in registers: n <= 4096
constexpr int SVR_BATCH = 32;             // problems per launch: their descriptors travel as kernel arguments
constexpr int SVR_MAX_ITERS = 1 << 20;
constexpr int SVR_MAX_N = 1 << 30;        // 2n is an int

struct SvrBatch { bbbp_svr_problem p[SVR_BATCH]; };

// a thread's best candidate of one selection and what travels with it
struct SvrCand {
    double v;            // the selection's value
    int k;               // index in the 2n ordering, -1: none
    double a, g;         // the variable's alpha and G
    int row;             // its row of K
};

// (v, k) := the later of two candidates in the total order "larger value, then larger index"
__device__ __forceinline__ bool svr_later(double v, int k, double ov, int ok) { return ov > v || (ov == v && ok > k); }

__device__ __forceinline__ void svr_wave_later_max(double& v, int& k) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        const double ov = __shfl_xor(v, w);
        const int ok = __shfl_xor(k, w);
        if (svr_later(v, k, ov, ok)) { v = ov; k = ok; }
    }
}

// R > 0: the state of base rows tid + m * SVR_THREADS, m < R, in registers.  R == 0: in global memory, any n.
template <int R>
struct SvrState {
    double a[R], as[R], g[R], gs[R], qd[R];
    int row[R];
    // f(r, alpha, alpha*, G, G*, QD, row of K)
    template <typename F>
    __device__ __forceinline__ void each(const bbbp_svr_problem&, int tid, int n, F&& f) {
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int r = tid + m * SVR_THREADS;
            if (r < n) f(r, a[m], as[m], g[m], gs[m], qd[m], row[m]);
        }
    }
};

template <>
struct SvrState<0> {
    template <typename F>
    __device__ __forceinline__ void each(const bbbp_svr_problem& pr, int tid, int n, F&& f) {
        for (int r = tid; r < n; r += SVR_THREADS) {
            int row = pr.rows ? pr.rows[r] : r;
            f(r, pr.alpha[r], pr.alpha[r + n], pr.grad[r], pr.grad[r + n], pr.diag[r], row);
        }
    }
};

template <int R>
__global__ __launch_bounds__(SVR_THREADS) void svr_smo_kernel(SvrBatch batch, int iters) {
    __shared__ double red_v[2][SVR_WAVES], red_a[2][SVR_WAVES], red_g[2][SVR_WAVES], red_g2[SVR_WAVES];
    __shared__ int red_k[2][SVR_WAVES], red_row[2][SVR_WAVES];
    __shared__ double rho_ub[SVR_WAVES], rho_lb[SVR_WAVES], rho_sum[SVR_WAVES];
    __shared__ int rho_free[SVR_WAVES];
    const bbbp_svr_problem& pr = batch.p[blockIdx.x];
    const double* K = pr.K;
    const long ldk = pr.ldk;
    const int n = pr.n;
    const double C = pr.C, tol = pr.tol, eps = pr.epsilon;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (*pr.done) return;                            // the same word for every thread; nobody has written it yet
    const bool fresh = *pr.n_iter == 0;              // the first launch of a problem: alpha = 0, G = p, whatever the arrays hold

    SvrState<R> st;
    if constexpr (R > 0) {
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int r = tid + m * SVR_THREADS;
            st.a[m] = st.as[m] = st.g[m] = st.gs[m] = st.qd[m] = 0.0;
            st.row[m] = 0;
            if (r < n) {
                const int row = pr.rows ? pr.rows[r] : r;
                st.row[m] = row;
                st.qd[m] = K[(long)row * ldk + row];
                if (fresh) { const double t = pr.t[r]; st.g[m] = eps - t; st.gs[m] = eps + t; }
                else { st.a[m] = pr.alpha[r]; st.as[m] = pr.alpha[r + n]; st.g[m] = pr.grad[r]; st.gs[m] = pr.grad[r + n]; }
            }
        }
    } else {
        for (int r = tid; r < n; r += SVR_THREADS) {
            const long row = pr.rows ? pr.rows[r] : r;
            pr.diag[r] = K[row * ldk + row];
            if (fresh) { const double t = pr.t[r]; pr.alpha[r] = 0.0; pr.alpha[r + n] = 0.0; pr.grad[r] = eps - t; pr.grad[r + n] = eps + t; }
        }
    }

    int it = 0;
    bool finished = false;
    for (; it < iters; ++it) {
        // i: the largest -s G over I_up = {s = +1, alpha < C} and {s = -1, alpha > 0}, the last among equals
        SvrCand ci = {-INFINITY, -1, 0.0, 0.0, 0};
        st.each(pr, tid, n, [&](int r, double& a, double& as, double& g, double& gs, double& qd, int row) {
            if (a < C && svr_later(ci.v, ci.k, -g, r)) ci = {-g, r, a, g, row};
            if (as > 0.0 && svr_later(ci.v, ci.k, gs, r + n)) ci = {gs, r + n, as, gs, row};
        });
        double bv = ci.v;
        int bk = ci.k;
        svr_wave_later_max(bv, bk);
        if (lane == 0) { red_v[0][wave] = bv; red_k[0][wave] = bk; }
        if (bk >= 0 && bk == ci.k) { red_a[0][wave] = ci.a; red_row[0][wave] = ci.row; }      // the one lane that owns the wave's winner
        __syncthreads();
        double gmax = red_v[0][0];
        int i = red_k[0][0], wi = 0;
#pragma unroll
        for (int w = 1; w < SVR_WAVES; ++w)
            if (svr_later(gmax, i, red_v[0][w], red_k[0][w])) { gmax = red_v[0][w]; i = red_k[0][w]; wi = w; }
        if (i < 0) { finished = true; break; }       // I_up is empty (the same decision in every thread)
        const double ai0 = red_a[0][wi];
        const long ri = red_row[0][wi];
        const double si = i < n ? 1.0 : -1.0;
        const double gi = i < n ? -gmax : gmax;      // gmax = -s_i G_i, exactly
        const double* Ki = K + ri * ldk;
        const double qdi = Ki[ri];

        // j: over I_low = {s = +1, alpha > 0} and {s = -1, alpha < C} with b = gmax + s G > 0, the largest b^2 / a, the last among equals
        SvrCand cj = {-INFINITY, -1, 0.0, 0.0, 0};
        double g2 = -INFINITY;
        st.each(pr, tid, n, [&](int r, double& a, double& as, double& g, double& gs, double& qd, int row) {
            const bool lo = a > 0.0, los = as < C;
            if (!lo && !los) return;
            double quad = qdi + qd - 2.0 * Ki[row];
            if (!(quad > 0.0)) quad = SVR_TAU;
            if (lo) {
                g2 = fmax(g2, g);
                const double b = gmax + g;
                if (b > 0.0) {
                    const double s = (b * b) / quad;
                    if (svr_later(cj.v, cj.k, s, r)) cj = {s, r, a, g, row};
                }
            }
            if (los) {
                g2 = fmax(g2, -gs);
                const double b = gmax - gs;
                if (b > 0.0) {
                    const double s = (b * b) / quad;
                    if (svr_later(cj.v, cj.k, s, r + n)) cj = {s, r + n, as, gs, row};
                }
            }
        });
        double sv = cj.v;
        int sk = cj.k;
        svr_wave_later_max(sv, sk);
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) g2 = fmax(g2, __shfl_xor(g2, w));
        if (lane == 0) { red_v[1][wave] = sv; red_k[1][wave] = sk; red_g2[wave] = g2; }
        if (sk >= 0 && sk == cj.k) { red_a[1][wave] = cj.a; red_g[1][wave] = cj.g; red_row[1][wave] = cj.row; }
        __syncthreads();
        double best = red_v[1][0], gmax2 = red_g2[0];
        int j = red_k[1][0], wj = 0;
#pragma unroll
        for (int w = 1; w < SVR_WAVES; ++w) {
            if (svr_later(best, j, red_v[1][w], red_k[1][w])) { best = red_v[1][w]; j = red_k[1][w]; wj = w; }
            gmax2 = fmax(gmax2, red_g2[w]);
        }
        if (gmax + gmax2 < tol || j < 0) { finished = true; break; }

        // the pair: every thread computes the same update from what came with the reductions; a thread writes only what it owns
        const double aj0 = red_a[1][wj], gj = red_g[1][wj];
        const long rj = red_row[1][wj];
        const double sj = j < n ? 1.0 : -1.0;
        const double* Kj = K + rj * ldk;
        double quad = qdi + Kj[rj] - 2.0 * Ki[rj];
        if (!(quad > 0.0)) quad = SVR_TAU;
        double ai = ai0, aj = aj0;
        if (si != sj) {
            const double delta = (-gi - gj) / quad, diff = ai - aj;
            ai += delta; aj += delta;
            if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
            else if (ai < 0.0) { ai = 0.0; aj = -diff; }
            if (diff > 0.0) { if (ai > C) { ai = C; aj = C - diff; } }
            else if (aj > C) { aj = C; ai = C + diff; }
        } else {
            const double delta = (gi - gj) / quad, sum = ai + aj;
            ai -= delta; aj += delta;
            if (sum > C) { if (ai > C) { ai = C; aj = sum - C; } }
            else if (aj < 0.0) { aj = 0.0; ai = sum; }
            if (sum > C) { if (aj > C) { aj = C; ai = sum - C; } }
            else if (ai < 0.0) { ai = 0.0; aj = sum; }
        }
        const double dai = ai - ai0, daj = aj - aj0;
        st.each(pr, tid, n, [&](int r, double& a, double& as, double& g, double& gs, double& qd, int row) {
            const double t = (si * Ki[row]) * dai + (sj * Kj[row]) * daj;
            g += t;
            gs -= t;
            if (r == i) a = ai;
            if (r + n == i) as = ai;
            if (r == j) a = aj;
            if (r + n == j) as = aj;
        });
        // no barrier: the next iteration's first LDS writes go to the slots of selection 0, which every thread has finished reading
        // before it arrived at the barrier of selection 1
    }

    // rho (libsvm's calculate_rho) from the state this launch leaves: the mean of s G over the free variables, else the bounds' midpoint
    double ub = INFINITY, lb = -INFINITY, sum = 0.0;
    int nfree = 0;
    st.each(pr, tid, n, [&](int r, double& a, double& as, double& g, double& gs, double& qd, int row) {
        if (a >= C) lb = fmax(lb, g);
        else if (a <= 0.0) ub = fmin(ub, g);
        else { ++nfree; sum += g; }
        const double ygs = -gs;
        if (as >= C) ub = fmin(ub, ygs);
        else if (as <= 0.0) lb = fmax(lb, ygs);
        else { ++nfree; sum += ygs; }
    });
    if constexpr (R > 0) {
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int r = tid + m * SVR_THREADS;
            if (r < n) { pr.alpha[r] = st.a[m]; pr.alpha[r + n] = st.as[m]; pr.grad[r] = st.g[m]; pr.grad[r + n] = st.gs[m]; }
        }
    }
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        ub = fmin(ub, __shfl_xor(ub, w));
        lb = fmax(lb, __shfl_xor(lb, w));
        sum += __shfl_xor(sum, w);
        nfree += __shfl_xor(nfree, w);
    }
    if (lane == 0) { rho_ub[wave] = ub; rho_lb[wave] = lb; rho_sum[wave] = sum; rho_free[wave] = nfree; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SVR_WAVES; ++w) {
            ub = fmin(ub, rho_ub[w]); lb = fmax(lb, rho_lb[w]); sum += rho_sum[w]; nfree += rho_free[w];
        }
        *pr.rho = nfree > 0 ? sum / (double)nfree : (ub + lb) * 0.5;
        *pr.n_iter += it;
        *pr.done = finished ? 1 : 0;
    }
}

inline bool finite_pos(double v) { return v > 0.0 && v <= 1.79769313486231570815e+308; }

}  // namespace

extern "C" int bbbp_svr_smo(void* stream, const bbbp_svr_problem* problems, int n_problems, int iters) {
    BBBP_CHECK_ARG(problems != nullptr, "bbbp_svr_smo: null problem list");
    BBBP_CHECK_ARG(n_problems > 0, "bbbp_svr_smo: n_problems %d must be positive", n_problems);
    BBBP_CHECK_ARG(iters >= 1 && iters <= SVR_MAX_ITERS, "bbbp_svr_smo: iters %d outside [1, %d]", iters, SVR_MAX_ITERS);
    for (int q = 0; q < n_problems; ++q) {
        const bbbp_svr_problem& p = problems[q];
        BBBP_CHECK_ARG(p.n > 0 && p.n <= SVR_MAX_N, "bbbp_svr_smo: problem %d: n %d must be positive and at most %d", q, p.n, SVR_MAX_N);
        BBBP_CHECK_ARG(p.K && p.t && p.alpha && p.grad && p.diag && p.rho && p.n_iter && p.done, "bbbp_svr_smo: problem %d: null pointer", q);
        BBBP_CHECK_ARG(p.rows ? p.ldk > 0 : p.ldk >= p.n, "bbbp_svr_smo: problem %d: leading dimension %ld too small", q, p.ldk);
        BBBP_CHECK_ARG(finite_pos(p.C), "bbbp_svr_smo: problem %d: C %g must be positive and finite", q, p.C);
        BBBP_CHECK_ARG(finite_pos(p.tol), "bbbp_svr_smo: problem %d: tol %g must be positive and finite", q, p.tol);
        BBBP_CHECK_ARG(p.epsilon >= 0.0 && p.epsilon <= 1.79769313486231570815e+308, "bbbp_svr_smo: problem %d: epsilon %g must be non-negative and finite",
                       q, p.epsilon);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    // problems of one launch share a kernel form: a run of consecutive problems with the same rows-per-thread class, at most SVR_BATCH
    auto form = [](int n) { const int rows = cdiv(n, SVR_THREADS); return rows <= 1 ? 1 : rows <= 2 ? 2 : rows <= SVR_REG_ROWS ? 4 : 0; };
    for (int q0 = 0; q0 < n_problems;) {
        const int f = form(problems[q0].n);
        SvrBatch b = {};
        int nb = 0;
        while (q0 + nb < n_problems && nb < SVR_BATCH && form(problems[q0 + nb].n) == f) { b.p[nb] = problems[q0 + nb]; ++nb; }
        void (*k)(SvrBatch, int) = f == 1 ? svr_smo_kernel<1> : f == 2 ? svr_smo_kernel<2> : f == 4 ? svr_smo_kernel<4> : svr_smo_kernel<0>;
        hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(SVR_THREADS), 0, st, b, iters);
        BBBP_CHECK_LAUNCH();
        q0 += nb;
    }
    return BBBP_OK;
}
