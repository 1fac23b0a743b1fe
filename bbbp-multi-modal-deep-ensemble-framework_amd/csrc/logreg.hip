// Binary L2-regularised logistic regression in float64: a damped Newton solver that runs a batch of independent problems in lock step.
//
//   bbbp_logreg_rounds     `rounds` x (row pass, weighted Gram matrix, step) for every problem that is not done.
//   bbbp_logreg_eval       one evaluation (loss, gradient, Hessian) at a given point, no step: what the tests compare with numpy.
//   bbbp_logreg_decision   z = X w + b with the row pass's dot product.
//
// Objective (scikit-learn's scaling): f = 1/n sum log(1 + exp(s_i)) + |w|^2 / (2 C n), s_i = -z_i (t_i = 1) or z_i (t_i = 0).  Every term
// is formed without overflow or cancellation: the loss as log1p(exp(-|s|)) + max(s, 0), the residual p - t as -expit(-z) / expit(z), the
// curvature as expit(z) expit(-z), expit itself from exp of a non-positive argument only.
// Row pass.  A work-group owns 64 rows.  A wave reads a row with unit stride (lane k, k + 64, ...), multiplies by theta held in LDS and
// adds the 64 lane sums in a butterfly, which leaves the same bits in every lane.  Then thread k adds x[i][k] r_i and x[i][k] w_i over the
// group's rows in ascending order: one partial per (row block, column) of X^T r (the gradient) and X^T w (the Hessian's intercept row).
// Gram.  X^T diag(w) X is the TN form of f64_tile_product (k = rows) with w as the per-k scale of operand A.  A work-group owns a pair of
// 64-column tiles (i <= j) and a slab of rows; its 64 x 64 block goes to the workspace.
// Step.  One work-group per problem adds the row blocks' and the slabs' partials in ascending order, applies the accept / reject rule,
// and on an accepted, unconverged point factors H = U^T U in place (left-looking, thread i owns column i, packed upper triangle; in LDS up
// to p = 112, else in the problem's state) and solves U^T U s = -g.
// The block, tile and slab counts are functions of n and d alone and no work-group reads another problem's memory, so a problem's result
// is bit-identical whatever else is in the batch and however the rounds are cut into calls.
#include "f64_tile.h"
#include <math.h>

namespace {

constexpr int LR_ROWS = 64;               // rows per work-group of the row pass
constexpr int LR_THREADS = 256;
constexpr int LR_BATCH = 16;              // problems per launch: their descriptors travel as kernel arguments
constexpr int LR_P = BBBP_LOGREG_MAX_D + 1;
constexpr int LR_CHUNKS_PER_SLAB = 32;    // 512 rows per Gram slab ...
constexpr int LR_MAX_SLABS = 32;          // ... until that would exceed this many slabs
constexpr int LR_LDS_P = 112;             // largest p whose packed triangle is factored in LDS
constexpr int LR_LDS_U = LR_LDS_P * (LR_LDS_P + 1) / 2;
constexpr int LR_MAX_TRIALS = 21;
constexpr int LR_MAX_ROUNDS = 1 << 16;
constexpr int LR_TILE_ELEMS = F64_TILE * F64_TILE;

// Where everything lies in a problem's `state`, in doubles.  scal: 0 the loss at the last evaluated point, 1 the loss and 2 the gradient's
// 1-norm at the accepted point, 3 g.s of the current direction, 4 the current step length.
struct LogregLayout {
    int nb, tiles, pairs, nch, cps, slabs, rp;
    long scal, grad, dir, z, r, w, rowpart, grampart, U, total;
};

__host__ __device__ inline LogregLayout logreg_layout(int n, int d) {
    LogregLayout L;
    L.nb = (n + LR_ROWS - 1) / LR_ROWS;
    L.tiles = (d + F64_TILE - 1) / F64_TILE;
    L.pairs = L.tiles * (L.tiles + 1) / 2;
    L.nch = (n + F64_CHUNK - 1) / F64_CHUNK;
    const int spread = (L.nch + LR_MAX_SLABS - 1) / LR_MAX_SLABS;
    L.cps = spread > LR_CHUNKS_PER_SLAB ? spread : LR_CHUNKS_PER_SLAB;
    L.slabs = (L.nch + L.cps - 1) / L.cps;
    L.rp = 2 * d + 3;                      // X^T r [d], X^T w [d], sum r, sum w, sum loss
    L.scal = 0;
    L.grad = 8;
    L.dir = L.grad + LR_P;
    L.z = L.dir + LR_P;
    L.r = L.z + n;
    L.w = L.r + n;
    L.rowpart = L.w + n;
    L.grampart = L.rowpart + (long)L.nb * L.rp;
    L.U = L.grampart + (long)L.slabs * L.pairs * LR_TILE_ELEMS;
    L.total = L.U + (long)LR_P * (LR_P + 1) / 2;
    return L;
}

struct LogregBatch { bbbp_logreg_problem p[LR_BATCH]; };

__device__ __forceinline__ double lr_expit(double z) {
    if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
    const double e = exp(z);
    return e / (1.0 + e);
}

// sum_k X[row][k] th[k]: lane sums over k = lane, lane + 64, ... ascending, then a butterfly; every lane returns the same bits
template <bool F32>
__device__ __forceinline__ double lr_row_dot(const void* X, long ld, long row, int d, const double* th, int lane) {
    double acc = 0.0;
    for (int k = lane; k < d; k += 64) acc = fma(ld_elem<F32>(X, row * ld + k), th[k], acc);
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) acc += __shfl_xor(acc, w);
    return acc;
}

// ---- row pass -----------------------------------------------------------------------------------------------------------------------------
template <bool F32>
__device__ __forceinline__ void lr_row_block(const bbbp_logreg_problem& pr, const LogregLayout& L, double* th, double* rs, double* ws, double* ls) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = pr.n, d = pr.d;
    const long row0 = (long)blockIdx.x * LR_ROWS;
    for (int k = tid; k <= d; k += LR_THREADS) th[k] = pr.trial[k];
    __syncthreads();
    const double b = pr.fit_intercept ? th[d] : 0.0;
    double* st = pr.state;
    for (int q = wave; q < LR_ROWS; q += LR_THREADS / 64) {
        const long row = row0 + q;
        if (row >= n) {                                  // the same decision in the whole wave
            if (lane == 0) { rs[q] = 0.0; ws[q] = 0.0; ls[q] = 0.0; }
            continue;
        }
        const double z = lr_row_dot<F32>(pr.X, pr.ld, row, d, th, lane) + b;
        if (lane == 0) {
            const bool pos = pr.t[row] > 0.5;
            const double s = pos ? -z : z;
            const double up = lr_expit(z), dn = lr_expit(-z);
            const double r = pos ? -dn : up, w = up * dn;
            rs[q] = r; ws[q] = w; ls[q] = log1p(exp(-fabs(s))) + fmax(s, 0.0);
            st[L.z + row] = z; st[L.r + row] = r; st[L.w + row] = w;
        }
    }
    __syncthreads();
    const int rows = n - row0 < LR_ROWS ? (int)(n - row0) : LR_ROWS;
    double* part = st + L.rowpart + (long)blockIdx.x * L.rp;
    if (tid < d) {
        double sr = 0.0, sw = 0.0;
        for (int q = 0; q < rows; ++q) {
            const double x = ld_elem<F32>(pr.X, (row0 + q) * pr.ld + tid);
            sr = fma(x, rs[q], sr);
            sw = fma(x, ws[q], sw);
        }
        part[tid] = sr; part[d + tid] = sw;
    } else if (tid == d) {                               // d <= 255: this thread exists
        double sr = 0.0, sw = 0.0, sl = 0.0;
        for (int q = 0; q < rows; ++q) { sr += rs[q]; sw += ws[q]; sl += ls[q]; }
        part[2 * d] = sr; part[2 * d + 1] = sw; part[2 * d + 2] = sl;
    }
}

__global__ __launch_bounds__(LR_THREADS) void logreg_row_kernel(LogregBatch batch, int force) {
    __shared__ double th[LR_P], rs[LR_ROWS], ws[LR_ROWS], ls[LR_ROWS];
    const bbbp_logreg_problem& pr = batch.p[blockIdx.y];
    if (!force && pr.flags[2]) return;
    const LogregLayout L = logreg_layout(pr.n, pr.d);
    if ((int)blockIdx.x >= L.nb) return;
    if (pr.x_dtype == BBBP_DTYPE_F32) lr_row_block<true>(pr, L, th, rs, ws, ls);
    else lr_row_block<false>(pr, L, th, rs, ws, ls);
}

struct LogregDecParams { const void* X; const double* theta; double* out; long ld; int m, d, fit_intercept; };

template <bool F32>
__global__ __launch_bounds__(LR_THREADS) void logreg_decision_kernel(LogregDecParams p) {
    __shared__ double th[LR_P];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int k = tid; k <= p.d; k += LR_THREADS) th[k] = p.theta[k];
    __syncthreads();
    const double b = p.fit_intercept ? th[p.d] : 0.0;
    const long row0 = (long)blockIdx.x * LR_ROWS;
    for (int q = wave; q < LR_ROWS; q += LR_THREADS / 64) {
        const long row = row0 + q;
        if (row >= p.m) continue;
        const double z = lr_row_dot<F32>(p.X, p.ld, row, p.d, th, lane) + b;
        if (lane == 0) p.out[row] = z;
    }
}

// ---- weighted Gram matrix -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(F64_THREADS) void logreg_gram_kernel(LogregBatch batch, int force) {
    __shared__ double lds[F64_TILE_LDS];
    const bbbp_logreg_problem& pr = batch.p[blockIdx.y];
    if (!force && pr.flags[2]) return;
    const LogregLayout L = logreg_layout(pr.n, pr.d);
    if ((int)blockIdx.x >= L.pairs * L.slabs) return;
    const int pair = blockIdx.x % L.pairs, slab = blockIdx.x / L.pairs;
    int ti = 0, rem = pair;                              // pair -> (ti, tj), ti <= tj, row by row of the upper triangle
    while (rem >= L.tiles - ti) { rem -= L.tiles - ti; ++ti; }
    const int tj = ti + rem;
    const int c0 = slab * L.cps, c1 = min(c0 + L.cps, L.nch);
    const double* w = pr.state + L.w;
    const F64Frag f;
    f64x4 acc[2][2];
    if (pr.x_dtype == BBBP_DTYPE_F32)
        f64_tile_product<true, true, true, true>(lds, f, pr.X, pr.ld, ti * F64_TILE, pr.d, nullptr, pr.X, pr.ld, tj * F64_TILE, pr.d, nullptr, pr.n, c0, c1,
                                                 acc, w);
    else
        f64_tile_product<true, false, false, true>(lds, f, pr.X, pr.ld, ti * F64_TILE, pr.d, nullptr, pr.X, pr.ld, tj * F64_TILE, pr.d, nullptr, pr.n, c0,
                                                   c1, acc, w);
    double* out = pr.state + L.grampart + ((long)slab * L.pairs + pair) * LR_TILE_ELEMS;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) out[f.row(i, r) * F64_TILE + f.col(j)] = acc[i][j][r];
}

// ---- step ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long lr_off(int a, int p) { return (long)a * p - (long)a * (a - 1) / 2; }      // row a of the packed upper triangle

// sum of v[0 .. m) in ascending order: every thread reads the same LDS words and gets the same bits
__device__ __forceinline__ double lr_sum(const double* v, int m) {
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += v[k];
    return s;
}

__global__ __launch_bounds__(LR_THREADS) void logreg_step_kernel(LogregBatch batch, int eval_only) {
    __shared__ double u_lds[LR_LDS_U];
    __shared__ double th[LR_P], g[LR_P], hb[LR_P], bs[LR_P], ys[LR_P];
    __shared__ double piv;
    const bbbp_logreg_problem& pr = batch.p[blockIdx.x];
    int* flags = pr.flags;
    if (!eval_only && flags[2]) return;
    const int tid = threadIdx.x;
    const int n = pr.n, d = pr.d, p = d + (pr.fit_intercept ? 1 : 0);
    const LogregLayout L = logreg_layout(n, d);
    double* st = pr.state;
    const double inv_n = 1.0 / (double)n, pen = 1.0 / (pr.C * (double)n);
    const int n_iter = flags[0], trials = flags[3];
    const double f_old = st[L.scal + 1], g1_old = st[L.scal + 2], gts_old = st[L.scal + 3], alpha = st[L.scal + 4];

    // the row blocks' partials, block by block: thread k < d its column of X^T r and X^T w, thread d the sums of r and w
    th[tid] = tid <= d ? pr.trial[tid] : 0.0;
    {
        double sr = 0.0, sw = 0.0;
        if (tid <= d) {
            const double* part = st + L.rowpart + (tid < d ? tid : 2 * d);
            const int second = tid < d ? d : 1;
            for (int b = 0; b < L.nb; ++b) { sr += part[(long)b * L.rp]; sw += part[(long)b * L.rp + second]; }
        }
        const double tk = tid < d ? th[tid] : 0.0;
        g[tid] = tid < p ? sr * inv_n + tk * pen : 0.0;
        hb[tid] = sw * inv_n;
        double sl = 0.0;
        for (int b = tid; b < L.nb; b += LR_THREADS) sl += st[L.rowpart + (long)b * L.rp + 2 * d + 2];
        bs[tid] = sl;
        ys[tid] = tk * tk;
    }
    __syncthreads();
    const double f_new = lr_sum(bs, LR_THREADS) * inv_n + 0.5 * pen * lr_sum(ys, d);
    double g1_new = 0.0, gmax = 0.0;
    for (int k = 0; k < p; ++k) {
        const double a = fabs(g[k]);
        g1_new += a;
        gmax = a == a ? fmax(gmax, a) : INFINITY;        // fmax drops a NaN: a NaN gradient must not pass for a converged one
    }
    if (tid < p) st[L.grad + tid] = g[tid];
    if (tid == 0) st[L.scal] = f_new;
    __syncthreads();                                     // bs and ys are free again

    double* U = (!eval_only && p <= LR_LDS_P) ? u_lds : st + L.U;
    bool factor = eval_only != 0;
    if (!eval_only) {
        bool accept = trials == 0;                       // the starting point
        if (!accept) {
            const double diff = f_new - f_old;
            if (diff <= 0x1p-11 * alpha * gts_old) accept = true;
            else if (fabs(diff) <= fabs(f_old) * (16.0 * 0x1p-52) && g1_new < g1_old) accept = true;
        }
        if (!accept) {
            if (trials >= LR_MAX_TRIALS) {
                if (tid == 0) { flags[1] = BBBP_LOGREG_LINE_SEARCH; flags[2] = 1; }
                return;
            }
            const double half = 0.5 * alpha;
            if (tid < p) pr.trial[tid] = pr.theta[tid] + half * st[L.dir + tid];
            if (tid == 0) { st[L.scal + 4] = half; flags[3] = trials + 1; }
            return;
        }
        const int it = n_iter + (trials > 0 ? 1 : 0);
        if (tid < p) pr.theta[tid] = th[tid];
        if (tid == 0) { st[L.scal + 1] = f_new; st[L.scal + 2] = g1_new; flags[0] = it; }
        if (gmax <= pr.tol) {
            if (tid == 0) { flags[1] = BBBP_LOGREG_CONVERGED; flags[2] = 1; }
            return;
        }
        if (it >= pr.max_iter) {
            if (tid == 0) { flags[1] = BBBP_LOGREG_MAX_ITER; flags[2] = 1; }
            return;
        }
        factor = true;
    }
    if (!factor) return;

    // H = 1/n X^T diag(w) X + I / (C n), bordered by the intercept's row; the slabs' partials in ascending order
    for (int idx = tid; idx < p * p; idx += LR_THREADS) {
        const int a = idx / p, b = idx - a * p;
        if (b < a) continue;
        double v;
        if (b < d) {
            const int ta = a / F64_TILE, tb = b / F64_TILE;
            const int pair = ta * L.tiles - ta * (ta - 1) / 2 + (tb - ta);
            const double* part = st + L.grampart + (long)pair * LR_TILE_ELEMS + (a % F64_TILE) * F64_TILE + (b % F64_TILE);
            double s = 0.0;
            for (int sl = 0; sl < L.slabs; ++sl) s += part[(long)sl * L.pairs * LR_TILE_ELEMS];
            v = s * inv_n + (a == b ? pen : 0.0);
        } else {
            v = hb[a];                                   // b == d: the intercept's column
        }
        U[lr_off(a, p) + (b - a)] = v;
    }
    __syncthreads();
    if (eval_only) return;

    // Cholesky H = U^T U in place, left-looking: thread i owns column i
    for (int j = 0; j < p; ++j) {
        double acc = 0.0;
        if (tid >= j && tid < p) {
            acc = U[lr_off(j, p) + (tid - j)];
            long off = 0;
            for (int k = 0; k < j; ++k) {
                acc = fma(-U[off + (tid - k)], U[off + (j - k)], acc);
                off += p - k;
            }
            if (tid == j) piv = acc;
        }
        __syncthreads();
        const double pv = piv;
        if (!(pv > 0.0)) {                               // the same word in every thread
            if (tid == 0) { flags[1] = BBBP_LOGREG_PIVOT; flags[2] = 1; }
            return;
        }
        const double dg = sqrt(pv);
        if (tid >= j && tid < p) U[lr_off(j, p) + (tid - j)] = tid == j ? dg : acc / dg;
        __syncthreads();
    }
    // U^T y = -g, then U s = y
    bs[tid] = tid < p ? -g[tid] : 0.0;
    for (int k = 0; k < p; ++k) {
        __syncthreads();
        const long off = lr_off(k, p);
        const double yk = bs[k] / U[off];
        if (tid == k) ys[k] = yk;
        if (tid > k && tid < p) bs[tid] = fma(-U[off + (tid - k)], yk, bs[tid]);
    }
    for (int k = p - 1; k >= 0; --k) {
        __syncthreads();
        const double sk = ys[k] / U[lr_off(k, p)];
        if (tid == k) bs[k] = sk;
        if (tid < k) ys[tid] = fma(-U[lr_off(tid, p) + (k - tid)], sk, ys[tid]);
    }
    __syncthreads();
    if (tid < p) {
        st[L.dir + tid] = bs[tid];
        pr.trial[tid] = th[tid] + bs[tid];
    }
    double gts = 0.0;
    for (int k = 0; k < p; ++k) gts = fma(g[k], bs[k], gts);
    if (tid == 0) { st[L.scal + 3] = gts; st[L.scal + 4] = 1.0; flags[3] = 1; }
}

// ---- argument checks (no pointer is dereferenced) -------------------------------------------------------------------------------------------
inline bool positive_finite(double v) { return v > 0.0 && v <= 1.79769313486231570815e+308; }

int check_shape(const char* who, int n, int d) {
    BBBP_CHECK_ARG(n > 0 && d > 0, "%s: n, d must be positive (got %d, %d)", who, n, d);
    BBBP_CHECK_ARG(d <= BBBP_LOGREG_MAX_D, "%s: d %d exceeds %d features", who, d, BBBP_LOGREG_MAX_D);
    return BBBP_OK;
}

int check_problem(const char* who, const bbbp_logreg_problem& p, int q) {
    BBBP_CHECK_ARG(p.n > 0 && p.d > 0, "%s: problem %d: n, d must be positive (got %d, %d)", who, q, p.n, p.d);
    BBBP_CHECK_ARG(p.d <= BBBP_LOGREG_MAX_D, "%s: problem %d: d %d exceeds %d features", who, q, p.d, BBBP_LOGREG_MAX_D);
    BBBP_CHECK_ARG(dtype_ok(p.x_dtype), "%s: problem %d: unknown dtype %d: 0 = float32, 1 = float64", who, q, p.x_dtype);
    BBBP_CHECK_ARG(p.X && p.t && p.theta && p.trial && p.state && p.flags, "%s: problem %d: null pointer", who, q);
    BBBP_CHECK_ARG(p.ld >= p.d, "%s: problem %d: leading dimension %ld too small for d %d", who, q, p.ld, p.d);
    BBBP_CHECK_ARG(positive_finite(p.C), "%s: problem %d: C %g must be positive and finite", who, q, p.C);
    BBBP_CHECK_ARG(positive_finite(p.tol), "%s: problem %d: tol %g must be positive and finite", who, q, p.tol);
    BBBP_CHECK_ARG(p.fit_intercept == 0 || p.fit_intercept == 1, "%s: problem %d: fit_intercept %d is neither 0 nor 1", who, q, p.fit_intercept);
    BBBP_CHECK_ARG(p.max_iter >= 1, "%s: problem %d: max_iter %d must be positive", who, q, p.max_iter);
    return BBBP_OK;
}

int launch_round(hipStream_t st, const LogregBatch& b, int nb, int eval_only) {
    int row_blocks = 0, gram_blocks = 0;
    for (int q = 0; q < nb; ++q) {
        const LogregLayout L = logreg_layout(b.p[q].n, b.p[q].d);
        row_blocks = L.nb > row_blocks ? L.nb : row_blocks;
        gram_blocks = L.pairs * L.slabs > gram_blocks ? L.pairs * L.slabs : gram_blocks;
    }
    hipLaunchKernelGGL(logreg_row_kernel, dim3((unsigned)row_blocks, (unsigned)nb), dim3(LR_THREADS), 0, st, b, eval_only);
    BBBP_CHECK_LAUNCH();
    hipLaunchKernelGGL(logreg_gram_kernel, dim3((unsigned)gram_blocks, (unsigned)nb), dim3(F64_THREADS), 0, st, b, eval_only);
    BBBP_CHECK_LAUNCH();
    hipLaunchKernelGGL(logreg_step_kernel, dim3((unsigned)nb), dim3(LR_THREADS), 0, st, b, eval_only);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}

}  // namespace

extern "C" size_t bbbp_logreg_state_bytes(int n, int d) {
    if (check_shape("bbbp_logreg_state_bytes", n, d) != BBBP_OK) return 0;
    return (size_t)logreg_layout(n, d).total * sizeof(double);
}

extern "C" int bbbp_logreg_state_layout(int n, int d, long out[6]) {
    if (int rc = check_shape("bbbp_logreg_state_layout", n, d)) return rc;
    BBBP_CHECK_ARG(out != nullptr, "bbbp_logreg_state_layout: null pointer");
    const LogregLayout L = logreg_layout(n, d);
    out[0] = L.scal; out[1] = L.grad; out[2] = L.z; out[3] = L.r; out[4] = L.w; out[5] = L.U;
    return BBBP_OK;
}

extern "C" int bbbp_logreg_rounds(void* stream, const bbbp_logreg_problem* problems, int n_problems, int rounds) {
    BBBP_CHECK_ARG(problems != nullptr, "bbbp_logreg_rounds: null problem list");
    BBBP_CHECK_ARG(n_problems > 0, "bbbp_logreg_rounds: n_problems %d must be positive", n_problems);
    BBBP_CHECK_ARG(rounds >= 1 && rounds <= LR_MAX_ROUNDS, "bbbp_logreg_rounds: rounds %d outside [1, %d]", rounds, LR_MAX_ROUNDS);
    for (int q = 0; q < n_problems; ++q)
        if (int rc = check_problem("bbbp_logreg_rounds", problems[q], q)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int r = 0; r < rounds; ++r)
        for (int q0 = 0; q0 < n_problems; q0 += LR_BATCH) {
            const int nb = n_problems - q0 < LR_BATCH ? n_problems - q0 : LR_BATCH;
            LogregBatch b = {};
            for (int q = 0; q < nb; ++q) b.p[q] = problems[q0 + q];
            if (int rc = launch_round(st, b, nb, 0)) return rc;
        }
    return BBBP_OK;
}

extern "C" int bbbp_logreg_eval(void* stream, const bbbp_logreg_problem* problem) {
    BBBP_CHECK_ARG(problem != nullptr, "bbbp_logreg_eval: null problem");
    if (int rc = check_problem("bbbp_logreg_eval", *problem, 0)) return rc;
    LogregBatch b = {};
    b.p[0] = *problem;
    return launch_round(static_cast<hipStream_t>(stream), b, 1, 1);
}

extern "C" int bbbp_logreg_decision(void* stream, const void* X, int x_dtype, long ld, int m, int d, const double* theta, int fit_intercept,
                                    double* out) {
    if (int rc = check_shape("bbbp_logreg_decision", m, d)) return rc;
    BBBP_CHECK_ARG(dtype_ok(x_dtype), "bbbp_logreg_decision: unknown dtype %d: 0 = float32, 1 = float64", x_dtype);
    BBBP_CHECK_ARG(X && theta && out, "bbbp_logreg_decision: null pointer");
    BBBP_CHECK_ARG(ld >= d, "bbbp_logreg_decision: leading dimension %ld too small for d %d", ld, d);
    BBBP_CHECK_ARG(fit_intercept == 0 || fit_intercept == 1, "bbbp_logreg_decision: fit_intercept %d is neither 0 nor 1", fit_intercept);
    LogregDecParams p;
    p.X = X; p.theta = theta; p.out = out; p.ld = ld; p.m = m; p.d = d; p.fit_intercept = fit_intercept;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)cdiv(m, LR_ROWS));
    if (x_dtype == BBBP_DTYPE_F32) hipLaunchKernelGGL(logreg_decision_kernel<true>, grid, dim3(LR_THREADS), 0, st, p);
    else hipLaunchKernelGGL(logreg_decision_kernel<false>, grid, dim3(LR_THREADS), 0, st, p);
    BBBP_CHECK_LAUNCH();
    return BBBP_OK;
}
