// Support-vector classification in float64: the kernel matrix and the decision function on the float64 matrix pipe, and a batched SMO solver.
//
//   bbbp_svm_kernel_matrix   K[n][n] = X X^T (linear) or exp(-gamma |x_i - x_j|^2) (RBF), bitwise symmetric, RBF diagonal exactly 1.
//   bbbp_svm_smo             libsvm's C-SVC solver without shrinking, one work-group per problem, a bounded number of iterations per launch.
//   bbbp_svm_decision        f(x) = sum_s coef_s k(sv_s, x) + b, fused: the [m][n_sv] kernel block is never written.
//
// Kernel values.  A 64 x 64 block of inner products is one f64_tile_product (f64_tile.h).  Linear: the product itself, no shift.  RBF:
// s = |a - mu|^2 + |b - mu|^2 - 2 (a - mu).(b - mu) on rows centred at staging, as in knn.hip (the norms are bbbp_knn_row_norms with the same
// mu), clamped at 0, and exp(-gamma s) in the epilogue: the distance block lives in the accumulator registers only.  A value depends on its
// two rows alone (every pair runs the same k loop and the same expression).
// Matrix.  Only tiles on or below the diagonal run, only elements with row >= col are kept and each goes to (row, col) and (col, row); the
// RBF diagonal is written as exp(-gamma 0).
// Decision.  One work-group owns 64 queries and a contiguous range of support-vector tiles.  Per tile every thread multiplies its kernel
// values by their coefficients and adds its two columns, a butterfly over the 16 lanes of a row adds the 32 columns of a wave, LDS adds the
// two waves: one partial per (tile, query) goes to the workspace, and a second launch adds the tiles in ascending order plus b.  The unit of
// summation is the tile, never the slice: the result is bit-identical for every slice count.
// Solver.  State (alpha, G) lives in global memory and every launch runs at most `iters` iterations of every problem, so a launch ends by
// construction; the host reads the done flags and launches the unfinished problems again.  Work-groups share nothing and never wait on each
// other.  An iteration: block arg-max of -y G over I_up (i), block arg-max of b^2 / a over the violating part of I_low along row i of Q (j),
// libsvm's clipped pair update, and G += Q_i d_alpha_i + Q_j d_alpha_j.  Both selections keep the LATER index among equals, as libsvm's
// `>=` / `<=` scans do; every reduction is a total order on (value, index) or a fixed tree, so a problem's result is bit-identical from run
// to run and whatever else is in the batch.
#include "f64_tile.h"
#include <math.h>

namespace {

constexpr int SVM_SLICES = 64;            // largest forced slice count of the decision function
constexpr double SVM_TAU = 1e-12;         // libsvm's curvature floor
constexpr int SMO_THREADS = 1024;
constexpr int SMO_WAVES = SMO_THREADS / 64;
constexpr int SMO_BATCH = 32;             // problems per launch: their descriptors travel as kernel arguments
constexpr int SMO_MAX_ITERS = 1 << 20;

inline bool kernel_ok(int k) { return k == BBBP_SVM_LINEAR || k == BBBP_SVM_RBF; }

// one kernel value from the inner product of the (centred) rows and their squared norms
__device__ __forceinline__ double svm_kernel_value(int rbf, double gamma, double na, double nb, double dot) {
    if (!rbf) return dot;
    return exp(-gamma * fmax((na + nb) - 2.0 * dot, 0.0));
}

// ---- kernel matrix ----------------------------------------------------------------------------------------------------------------------
struct SvmMatParams {
    const void* X; const double* mu; const double* norms; double* K;
    long ldx, ldk, ntiles;
    int n, d, rbf;
    double gamma;
};

template <bool F32>
__global__ __launch_bounds__(F64_THREADS) void svm_matrix_kernel(SvmMatParams p) {
    __shared__ double lds[F64_TILE_LDS];
    const long tile = blockIdx.x;                    // -> (tm, tn) with tn <= tm, row by row of the lower triangle
    int tm = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
    while ((long)(tm + 1) * (tm + 2) / 2 <= tile) ++tm;
    while ((long)tm * (tm + 1) / 2 > tile) --tm;
    const int tn = (int)(tile - (long)tm * (tm + 1) / 2);
    const int m0 = tm * F64_TILE, n0 = tn * F64_TILE;
    const int nch = max((p.d + F64_CHUNK - 1) / F64_CHUNK, 1);

    const F64Frag f;
    f64x4 acc[2][2];
    f64_tile_product<false, F32, F32>(lds, f, p.X, p.ldx, m0, p.n, p.mu, p.X, p.ldx, n0, p.n, p.mu, p.d, 0, nch, acc);

    double* K = p.K;
    const long ldk = p.ldk;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = f.row(i, r, m0);
            if (row >= p.n) continue;
            const double nr = p.rbf ? p.norms[row] : 0.0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = f.col(j, n0);
                if (col > row) continue;             // col <= row < n
                const double v = (p.rbf && col == row) ? svm_kernel_value(1, p.gamma, 0.0, 0.0, 0.0)
                                                       : svm_kernel_value(p.rbf, p.gamma, nr, p.rbf ? p.norms[col] : 0.0, acc[i][j][r]);
                K[(size_t)row * ldk + col] = v;
                if (row != col) K[(size_t)col * ldk + row] = v;
            }
        }
}

// ---- decision function ------------------------------------------------------------------------------------------------------------------
struct SvmDecPlan {
    int tiles_q, tiles_sv, slices, tiles_per_slice;
    size_t part_bytes;           // tiles_sv * m doubles
};

// About two work-groups per CU; `forced` > 0 overrides (tests).  A slice past the last tile runs nothing.
SvmDecPlan svm_dec_plan(int m, int n_sv, int ncu, int forced) {
    SvmDecPlan pl;
    pl.tiles_q = cdiv(m, F64_TILE);
    pl.tiles_sv = cdiv(n_sv, F64_TILE);
    int s = forced;
    if (s <= 0) {
        const long want = 2L * ncu / pl.tiles_q;
        s = (int)(want < 1 ? 1 : want);
        if (s > pl.tiles_sv) s = pl.tiles_sv;
        if (s > SVM_SLICES) s = SVM_SLICES;
    }
    pl.slices = s;
    pl.tiles_per_slice = cdiv(pl.tiles_sv, s);
    pl.part_bytes = (size_t)pl.tiles_sv * m * sizeof(double);
    return pl;
}

struct SvmDecParams {
    const void* Q; const void* SV;
    const double* mu; const double* q_norm; const double* sv_norm; const double* coef;
    double* part; double* out;
    long ldq, ldsv;
    int m, n_sv, d, rbf;
    int tiles_q, tiles_sv, tiles_per_slice;
    double gamma, intercept;
};

template <bool QF32, bool SF32>
__global__ __launch_bounds__(F64_THREADS) void svm_decision_kernel(SvmDecParams p) {
    __shared__ double lds[F64_TILE_LDS];
    __shared__ double half[2][F64_TILE];             // [column half of the tile][query]
    const int tq = blockIdx.x % p.tiles_q, slice = blockIdx.x / p.tiles_q;
    const int m0 = tq * F64_TILE;
    const int t0 = slice * p.tiles_per_slice;
    const int t1 = min(t0 + p.tiles_per_slice, p.tiles_sv);
    const int nch = max((p.d + F64_CHUNK - 1) / F64_CHUNK, 1);
    const F64Frag f;

    for (int t = t0; t < t1; ++t) {
        const int n0 = t * F64_TILE;
        f64x4 acc[2][2];
        f64_tile_product<false, QF32, SF32>(lds, f, p.Q, p.ldq, m0, p.m, p.mu, p.SV, p.ldsv, n0, p.n_sv, p.mu, p.d, 0, nch, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lrow = f.row(i, r), row = m0 + lrow;
                double v = 0.0;
                if (row < p.m) {
                    const double qn = p.rbf ? p.q_norm[row] : 0.0;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int col = f.col(j, n0);
                        if (col < p.n_sv) v += svm_kernel_value(p.rbf, p.gamma, qn, p.rbf ? p.sv_norm[col] : 0.0, acc[i][j][r]) * p.coef[col];
                    }
                }
#pragma unroll
                for (int w = 1; w < 16; w <<= 1) v += __shfl_xor(v, w);      // the 16 lanes of a row: every lane ends with the same bits
                if (f.q == 0) half[f.wn >> 5][lrow] = v;
            }
        __syncthreads();
        if (threadIdx.x < F64_TILE && m0 + threadIdx.x < p.m)
            p.part[(size_t)t * p.m + m0 + threadIdx.x] = half[0][threadIdx.x] + half[1][threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void svm_decision_sum_kernel(SvmDecParams p) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= p.m) return;
    double v = 0.0;
    for (int t = 0; t < p.tiles_sv; ++t) v += p.part[(size_t)t * p.m + row];
    p.out[row] = v + p.intercept;
}

// ---- SMO --------------------------------------------------------------------------------------------------------------------------------
struct SmoBatch { bbbp_svm_problem p[SMO_BATCH]; };

// (v, i) := the later of two candidates in the total order "larger value, then larger index"
__device__ __forceinline__ void keep_later_max(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi > i)) { v = ov; i = oi; }
}

__device__ __forceinline__ void wave_later_max(double& v, int& i) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        const double ov = __shfl_xor(v, w);
        const int oi = __shfl_xor(i, w);
        keep_later_max(v, i, ov, oi);
    }
}

__global__ __launch_bounds__(SMO_THREADS) void svm_smo_kernel(SmoBatch batch, int iters) {
    __shared__ double red_v[2][SMO_WAVES];
    __shared__ int red_i[2][SMO_WAVES];
    __shared__ double red_g[SMO_WAVES];
    __shared__ double rho_ub[SMO_WAVES], rho_lb[SMO_WAVES], rho_sum[SMO_WAVES];
    __shared__ int rho_free[SMO_WAVES];
    const bbbp_svm_problem& pr = batch.p[blockIdx.x];
    const double* K = pr.K;
    const long ldk = pr.ldk;
    const int* rows = pr.rows;
    const double* y = pr.y;
    double* alpha = pr.alpha;
    double* G = pr.grad;
    double* qd = pr.diag;
    const int n = pr.n;
    const double C = pr.C, tol = pr.tol;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (*pr.done) return;                            // the same word for every thread; nobody has written it yet

    for (int k = tid; k < n; k += SMO_THREADS) {
        const long r = rows ? rows[k] : k;
        qd[k] = K[r * ldk + r];
    }
    __syncthreads();

    int it = 0;
    bool finished = false;
    for (; it < iters; ++it) {
        // i: the largest -y G over I_up = {y = +1, alpha < C} and {y = -1, alpha > 0}, the last among equals
        double bv = -INFINITY;
        int bi = -1;
        for (int k = tid; k < n; k += SMO_THREADS) {
            const double yk = y[k], a = alpha[k], g = G[k];
            const bool up = yk > 0.0 ? a < C : a > 0.0;
            const double v = yk > 0.0 ? -g : g;
            if (up && v >= bv) { bv = v; bi = k; }
        }
        wave_later_max(bv, bi);
        if (lane == 0) { red_v[0][wave] = bv; red_i[0][wave] = bi; }
        __syncthreads();
        double gmax = red_v[0][0];
        int i = red_i[0][0];
#pragma unroll
        for (int w = 1; w < SMO_WAVES; ++w) keep_later_max(gmax, i, red_v[0][w], red_i[0][w]);
        if (i < 0) { finished = true; break; }       // I_up is empty (the same decision in every thread)

        // j: over I_low = {y = +1, alpha > 0} and {y = -1, alpha < C} with b = gmax + y G > 0, the largest b^2 / a, the last among equals
        const long ri = rows ? rows[i] : i;
        const double* Ki = K + ri * ldk;
        const double qdi = qd[i];
        double sv = -INFINITY, g2 = -INFINITY;
        int sj = -1;
        for (int k = tid; k < n; k += SMO_THREADS) {
            const double yk = y[k], a = alpha[k], g = G[k];
            const bool low = yk > 0.0 ? a > 0.0 : a < C;
            if (!low) continue;
            const double yg = yk > 0.0 ? g : -g;
            g2 = fmax(g2, yg);
            const double b = gmax + yg;
            if (!(b > 0.0)) continue;
            const long rk = rows ? rows[k] : k;
            const double quad = qdi + qd[k] - 2.0 * Ki[rk];
            const double s = (b * b) / (quad > 0.0 ? quad : SVM_TAU);
            if (s >= sv) { sv = s; sj = k; }
        }
        wave_later_max(sv, sj);
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) g2 = fmax(g2, __shfl_xor(g2, w));
        if (lane == 0) { red_v[1][wave] = sv; red_i[1][wave] = sj; red_g[wave] = g2; }
        __syncthreads();
        double best = red_v[1][0], gmax2 = red_g[0];
        int j = red_i[1][0];
#pragma unroll
        for (int w = 1; w < SMO_WAVES; ++w) {
            keep_later_max(best, j, red_v[1][w], red_i[1][w]);
            gmax2 = fmax(gmax2, red_g[w]);
        }
        if (gmax + gmax2 < tol || j < 0) { finished = true; break; }

        // the pair: every thread reads it and computes the same update; owners write only behind the barrier
        const long rj = rows ? rows[j] : j;
        const double* Kj = K + rj * ldk;
        const double yi = y[i], yj = y[j], gi = G[i], gj = G[j], ai0 = alpha[i], aj0 = alpha[j];
        double quad = qdi + qd[j] - 2.0 * Ki[rj];
        if (!(quad > 0.0)) quad = SVM_TAU;
        __syncthreads();
        double ai = ai0, aj = aj0;
        if (yi != yj) {
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
        for (int k = tid; k < n; k += SMO_THREADS) {
            const long rk = rows ? rows[k] : k;
            const double yk = y[k];
            G[k] += (yi * yk * Ki[rk]) * dai + (yj * yk * Kj[rk]) * daj;
        }
        if (tid == 0) { alpha[i] = ai; alpha[j] = aj; }
        __syncthreads();
    }

    // rho (libsvm's calculate_rho) from the state this launch leaves: the mean of y G over the free variables, else the bounds' midpoint
    double ub = INFINITY, lb = -INFINITY, sum = 0.0;
    int nfree = 0;
    for (int k = tid; k < n; k += SMO_THREADS) {
        const double yk = y[k], a = alpha[k], yg = yk * G[k];
        if (a >= C) { if (yk < 0.0) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
        else if (a <= 0.0) { if (yk > 0.0) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
        else { ++nfree; sum += yg; }
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
        for (int w = 1; w < SMO_WAVES; ++w) {
            ub = fmin(ub, rho_ub[w]); lb = fmax(lb, rho_lb[w]); sum += rho_sum[w]; nfree += rho_free[w];
        }
        *pr.rho = nfree > 0 ? sum / (double)nfree : (ub + lb) * 0.5;
        *pr.n_iter += it;
        *pr.done = finished ? 1 : 0;
    }
}

// ---- descriptor checks (no pointer is dereferenced) -------------------------------------------------------------------------------------
int check_matrix(const bbbp_svm_kernel_desc* d) {
    BBBP_CHECK_ARG(d != nullptr, "bbbp_svm_kernel_matrix: null descriptor");
    BBBP_CHECK_ARG(d->n > 0 && d->d > 0, "bbbp_svm_kernel_matrix: n, d must be positive (got %d, %d)", d->n, d->d);
    BBBP_CHECK_ARG(kernel_ok(d->kernel), "bbbp_svm_kernel_matrix: kernel %d is neither linear (0) nor rbf (1)", d->kernel);
    BBBP_CHECK_ARG(dtype_ok(d->x_dtype), "bbbp_svm_kernel_matrix: unknown dtype %d: 0 = float32, 1 = float64", d->x_dtype);
    BBBP_CHECK_ARG(d->X && d->K, "bbbp_svm_kernel_matrix: null pointer");
    BBBP_CHECK_ARG(d->ldx >= d->d && d->ldk >= d->n, "bbbp_svm_kernel_matrix: leading dimension too small (ldx %ld, ldk %ld)", d->ldx, d->ldk);
    if (d->kernel == BBBP_SVM_RBF) {
        BBBP_CHECK_ARG(d->gamma > 0.0 && d->gamma <= 1.79769313486231570815e+308, "bbbp_svm_kernel_matrix: gamma %g must be positive and finite", d->gamma);
        BBBP_CHECK_ARG(d->norms != nullptr, "bbbp_svm_kernel_matrix: the rbf kernel needs the row norms (null pointer)");
    }
    return BBBP_OK;
}

int check_decision(const bbbp_svm_decision_desc* d, bool need_pointers) {
    BBBP_CHECK_ARG(d != nullptr, "bbbp_svm_decision: null descriptor");
    BBBP_CHECK_ARG(d->m > 0 && d->n_sv > 0 && d->d > 0, "bbbp_svm_decision: m, n_sv, d must be positive (got %d, %d, %d)", d->m, d->n_sv, d->d);
    BBBP_CHECK_ARG(kernel_ok(d->kernel), "bbbp_svm_decision: kernel %d is neither linear (0) nor rbf (1)", d->kernel);
    BBBP_CHECK_ARG(dtype_ok(d->q_dtype) && dtype_ok(d->sv_dtype), "bbbp_svm_decision: unknown dtype (q %d, sv %d): 0 = float32, 1 = float64", d->q_dtype,
                   d->sv_dtype);
    BBBP_CHECK_ARG(d->slices >= 0 && d->slices <= SVM_SLICES, "bbbp_svm_decision: slices %d outside [0, %d]", d->slices, SVM_SLICES);
    if (d->kernel == BBBP_SVM_RBF)
        BBBP_CHECK_ARG(d->gamma > 0.0 && d->gamma <= 1.79769313486231570815e+308, "bbbp_svm_decision: gamma %g must be positive and finite", d->gamma);
    if (need_pointers) {
        BBBP_CHECK_ARG(d->Q && d->SV && d->coef && d->out, "bbbp_svm_decision: null pointer");
        if (d->kernel == BBBP_SVM_RBF) BBBP_CHECK_ARG(d->q_norm && d->sv_norm, "bbbp_svm_decision: the rbf kernel needs both row norms (null pointer)");
        BBBP_CHECK_ARG(d->ldq >= d->d && d->ldsv >= d->d, "bbbp_svm_decision: leading dimension too small (ldq %ld, ldsv %ld, d %d)", d->ldq, d->ldsv, d->d);
    }
    return BBBP_OK;
}

}  // namespace

extern "C" int bbbp_svm_kernel_matrix(void* stream, const bbbp_svm_kernel_desc* d) {
    if (int rc = check_matrix(d)) return rc;
    const long tiles = cdiv(d->n, F64_TILE);
    SvmMatParams p;
    p.X = d->X; p.K = d->K; p.ldx = d->ldx; p.ldk = d->ldk;
    p.n = d->n; p.d = d->d; p.rbf = d->kernel == BBBP_SVM_RBF; p.gamma = d->gamma;
    p.mu = p.rbf ? d->mu : nullptr;                  // the linear form is the uncentred product
    p.norms = p.rbf ? d->norms : nullptr;
    p.ntiles = tiles * (tiles + 1) / 2;
    BBBP_CHECK_ARG(p.ntiles <= 0x7fffffffL, "bbbp_svm_kernel_matrix: %ld tiles exceed the grid", p.ntiles);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->x_dtype == BBBP_DTYPE_F32) hipLaunchKernelGGL(svm_matrix_kernel<true>, dim3((unsigned)p.ntiles), dim3(F64_THREADS), 0, st, p);
    else hipLaunchKernelGGL(svm_matrix_kernel<false>, dim3((unsigned)p.ntiles), dim3(F64_THREADS), 0, st, p);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

extern "C" int bbbp_svm_smo(void* stream, const bbbp_svm_problem* problems, int n_problems, int iters) {
    BBBP_CHECK_ARG(problems != nullptr, "bbbp_svm_smo: null problem list");
    BBBP_CHECK_ARG(n_problems > 0, "bbbp_svm_smo: n_problems %d must be positive", n_problems);
    BBBP_CHECK_ARG(iters >= 1 && iters <= SMO_MAX_ITERS, "bbbp_svm_smo: iters %d outside [1, %d]", iters, SMO_MAX_ITERS);
    for (int q = 0; q < n_problems; ++q) {
        const bbbp_svm_problem& p = problems[q];
        BBBP_CHECK_ARG(p.n > 0, "bbbp_svm_smo: problem %d: n %d must be positive", q, p.n);
        BBBP_CHECK_ARG(p.K && p.y && p.alpha && p.grad && p.diag && p.rho && p.n_iter && p.done, "bbbp_svm_smo: problem %d: null pointer", q);
        BBBP_CHECK_ARG(p.rows ? p.ldk > 0 : p.ldk >= p.n, "bbbp_svm_smo: problem %d: leading dimension %ld too small", q, p.ldk);
        BBBP_CHECK_ARG(p.C > 0.0 && p.C <= 1.79769313486231570815e+308, "bbbp_svm_smo: problem %d: C %g must be positive and finite", q, p.C);
        BBBP_CHECK_ARG(p.tol > 0.0 && p.tol <= 1.79769313486231570815e+308, "bbbp_svm_smo: problem %d: tol %g must be positive and finite", q, p.tol);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int q0 = 0; q0 < n_problems; q0 += SMO_BATCH) {
        const int nb = n_problems - q0 < SMO_BATCH ? n_problems - q0 : SMO_BATCH;
        SmoBatch b = {};
        for (int q = 0; q < nb; ++q) b.p[q] = problems[q0 + q];
        hipLaunchKernelGGL(svm_smo_kernel, dim3((unsigned)nb), dim3(SMO_THREADS), 0, st, b, iters);
        BBBP_CHECK_LAUNCH();
    }
    return BBBP_OK;
}

extern "C" size_t bbbp_svm_decision_workspace_bytes(const bbbp_svm_decision_desc* d) {
    if (check_decision(d, false) != BBBP_OK) return 0;
    return svm_dec_plan(d->m, d->n_sv, bbbp_num_cus(), d->slices).part_bytes;
}

extern "C" int bbbp_svm_decision(void* stream, const bbbp_svm_decision_desc* d, void* workspace, size_t workspace_bytes) {
    if (int rc = check_decision(d, true)) return rc;
    const SvmDecPlan pl = svm_dec_plan(d->m, d->n_sv, bbbp_num_cus(), d->slices);
    if (!workspace || workspace_bytes < pl.part_bytes) {
        bbbp_set_error("bbbp_svm_decision: workspace of %zu bytes, %zu needed", workspace_bytes, pl.part_bytes);
        return BBBP_ERR_WORKSPACE;
    }
    BBBP_CHECK_ARG((long)pl.tiles_q * pl.slices <= 0x7fffffffL, "bbbp_svm_decision: %d query tiles x %d slices exceed the grid", pl.tiles_q, pl.slices);
    SvmDecParams p;
    p.Q = d->Q; p.SV = d->SV; p.coef = d->coef;
    p.rbf = d->kernel == BBBP_SVM_RBF;
    p.mu = p.rbf ? d->mu : nullptr; p.q_norm = p.rbf ? d->q_norm : nullptr; p.sv_norm = p.rbf ? d->sv_norm : nullptr;
    p.part = static_cast<double*>(workspace); p.out = d->out;
    p.ldq = d->ldq; p.ldsv = d->ldsv;
    p.m = d->m; p.n_sv = d->n_sv; p.d = d->d;
    p.tiles_q = pl.tiles_q; p.tiles_sv = pl.tiles_sv; p.tiles_per_slice = pl.tiles_per_slice;
    p.gamma = d->gamma; p.intercept = d->intercept;
    void (*k)(SvmDecParams) = nullptr;
    with_bools(d->q_dtype == BBBP_DTYPE_F32, d->sv_dtype == BBBP_DTYPE_F32, [&](auto Q, auto S) { k = svm_decision_kernel<Q.value, S.value>; });
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k, dim3((unsigned)(pl.tiles_q * pl.slices)), dim3(F64_THREADS), 0, st, p);
    BBBP_CHECK_LAUNCH();
    hipLaunchKernelGGL(svm_decision_sum_kernel, dim3((unsigned)cdiv(d->m, 256)), dim3(256), 0, st, p);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
