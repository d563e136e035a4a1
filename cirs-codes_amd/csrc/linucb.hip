// linucb.hip -- the disjoint-arm LinUCB bandit of the Kuaishou baselines: accumulation, solve, scoring and prediction, all float64.
//   replaces  core/policy/linucb.py:11-68 (linucb_disjoint_arm: reward_update, the A_inv / theta properties, calc_reward, calc_UCB),
//             :77-103 (select_arm), :109-131 (evaluate_data's per-row loop), :133-159 (recommend_k_item's per-arm loop) and
//             :162-180 (linucb_trainer's per-row loop).
//
// State: arm a of K keeps A_a [d, d] (identity at start) and b_a [d] (zero at start); 2 <= d <= 16, d = 7 is the Kuaishou shape.
//
// linucb_update_kernel   one wavefront per arm.  Element e of the arm's d*d + d values (A row-major, then b) belongs to lane e & 63
//                        (d = 7: 56 values, one per lane; d = 16: 272 values, up to five per lane).  The lane walks the arm's rows in
//                        log order and does acc = acc + u * v per row: a rounded product, then a rounded sum, exactly the two
//                        roundings of numpy's `A += np.dot(x, x.T)` and `b += reward * x`.  The order of a sum of floats is part of
//                        its value, so no row of an arm is ever added out of order and nothing is split across lanes: A and b come
//                        out bit-identical to the reference's loop.  The rows of an arm lie anywhere in the log, so a lane that
//                        fetched them one after the other would pay one memory latency per row; instead the arm's rows are taken 64
//                        at a time: lane k reads row index k of the chunk (coalesced) and fetches that row whole into the
//                        wavefront's LDS stage, 64 rows in flight at once, then every lane walks the staged rows in order, reading
//                        its two factors from LDS (all lanes read the same row: broadcasts).
// linucb_solve_kernel    one thread per (arm, right-hand side): the d unit vectors give the columns of inv(A), b gives theta.  The
//                        thread factors A = L L^T (A = I + sum x x^T is symmetric positive definite) and solves; then three steps of
//                        iterative refinement whose residual rhs - A z is accumulated in twice the working precision (error-free
//                        products through fma, compensated sums).  cond(A) reaches 1e12 on this workload (within an arm only the
//                        user id varies, so sum x x^T has rank 2 with entries ~ n id^2); the plain factorisation loses up to 12 of
//                        the 16 digits there, refinement gives them back as long as cond * 2^-53 < 1.
// linucb_score_kernel    one workgroup per user (or one for the single x of select_arm): a thread takes arms t, t + 256, ...,
//                        builds x = [user, arm, item_feats[arm]], computes mean = theta^T x and var = x^T inv(A) x with compensated
//                        dot products, ucb = mean + alpha sqrt(var), and keeps its best (ucb, arm); the workgroup reduces to the
//                        FIRST arg-max (lowest arm on ties, numpy's argmax) and writes that arm and its mean.
// linucb_predict_kernel  one thread per row: theta[arm[r]]^T x[r], 0 where arm[r] is outside [0, K).
#include "common.h"

namespace cirs {

constexpr int luMaxD = 16;
constexpr int luMinD = 2;
constexpr int luThreads = 256;
constexpr int luRefine = 3;
constexpr int luStageLd = luMaxD + 1;      // a staged row: d <= 16 values of x, the reward at index luMaxD (odd stride: no bank pile-up)

// ---- arithmetic in twice the working precision: s + e is the exact sum / product of the operands ----------------------------------
struct dd { double hi, lo; };
__device__ __forceinline__ void dd_add(dd& acc, double t_hi, double t_lo) {
    const double s = acc.hi + t_hi;
    const double z = s - acc.hi;
    const double e = (acc.hi - (s - z)) + (t_hi - z);
    acc.hi = s;
    acc.lo += e + t_lo;
}
__device__ __forceinline__ void dd_add_prod(dd& acc, double a, double b) {
    const double p = a * b;
    dd_add(acc, p, fma(a, b, -p));
}
__device__ __forceinline__ double dd_value(const dd& acc) { return acc.hi + acc.lo; }

template <int NQ>
__global__ __launch_bounds__(luThreads) void linucb_update_kernel(double* __restrict__ A, double* __restrict__ b, int K, int d,
                                                                  const double* __restrict__ x, long ld, long n,
                                                                  const double* __restrict__ y, const int64_t* __restrict__ order, long m,
                                                                  const int64_t* __restrict__ seg) {
    __shared__ double stage[luThreads / CIRS_WAVE][CIRS_WAVE][luStageLd];      // per wavefront: 64 rows [x (d) | pad | y]
    const int lane = threadIdx.x & 63;
    const long arm = (long)blockIdx.x * (luThreads / CIRS_WAVE) + (threadIdx.x >> 6);
    if (arm >= K) return;
    long s = seg[arm], e = seg[arm + 1];
    s = s < 0 ? 0 : s;
    e = e > m ? m : e;
    if (e <= s) return;
    const int dd2 = d * d, ne = dd2 + d;
    double acc[NQ];
    double* dst[NQ];
    int ci[NQ], cj[NQ];      // the element is x[ci] * x[cj], cj < 0: x[ci] * y
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int el = lane + CIRS_WAVE * q;
        const bool on = el < ne;
        const bool inA = el < dd2;
        ci[q] = !on ? 0 : (inA ? el / d : el - dd2);
        cj[q] = !on ? 0 : (inA ? el % d : -1);
        dst[q] = !on ? nullptr : (inA ? A + arm * dd2 + el : b + arm * d + (el - dd2));
        acc[q] = on ? *dst[q] : 0.0;
    }
    double* st = &stage[threadIdx.x >> 6][0][0];
    for (long base = s; base < e; base += CIRS_WAVE) {
        // lane k fetches row k of the chunk whole (its d values and its reward): 64 independent rows in flight, one memory latency
        // per chunk instead of one per row
        const long row = base + lane < e ? order[base + lane] : -1;
        const bool ok = (unsigned long)row < (unsigned long)n;          // an index outside the log adds nothing
        if (ok) {
            for (int c = 0; c < d; ++c) st[lane * luStageLd + c] = x[row * ld + c];
            st[lane * luStageLd + luMaxD] = y[row];
        }
        const unsigned long long live = __ballot(ok);
        __builtin_amdgcn_wave_barrier();
        const int cnt = e - base < CIRS_WAVE ? (int)(e - base) : CIRS_WAVE;
        auto add_row = [&](int k) {
            const double* xr = st + k * luStageLd;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const double u = xr[ci[q]];
                const double v = xr[cj[q] >= 0 ? cj[q] : luMaxD];
                const double p = u * v;                                  // rounded product ...
                acc[q] = acc[q] + p;                                     // ... then rounded sum: never one fused operation
            }
        };
        // every index inside the log (the usual case): the LDS reads of eight rows go out together, the sums still follow one another
        if (live == (cnt == CIRS_WAVE ? ~0ull : (1ull << cnt) - 1ull)) {
#pragma unroll 8
            for (int k = 0; k < cnt; ++k) add_row(k);
        } else {
            for (int k = 0; k < cnt; ++k)
                if ((live >> k) & 1ull) add_row(k);                      // wave-uniform
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (dst[q]) *dst[q] = acc[q];
}

// z = inv(L L^T) r, L lower triangular [d, d] row-major in `L`
__device__ __forceinline__ void chol_solve(const double* L, int d, const double* r, double* z) {
    for (int i = 0; i < d; ++i) {
        double v = r[i];
        for (int k = 0; k < i; ++k) v -= L[i * d + k] * z[k];
        z[i] = v / L[i * d + i];
    }
    for (int i = d - 1; i >= 0; --i) {
        double v = z[i];
        for (int k = i + 1; k < d; ++k) v -= L[k * d + i] * z[k];
        z[i] = v / L[i * d + i];
    }
}

template <int D>      // D = 0: d at run time
__global__ __launch_bounds__(luThreads) void linucb_solve_kernel(const double* __restrict__ A, const double* __restrict__ b, int d_rt,
                                                                 const int32_t* __restrict__ arms, long n_arms, int K,
                                                                 double* __restrict__ A_inv, double* __restrict__ theta) {
    const int d = D ? D : d_rt;
    constexpr int MD = D ? D : luMaxD;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_arms * (d + 1)) return;
    const long slot = t / (d + 1);
    const int col = (int)(t % (d + 1));                    // col < d: unit vector col -> column col of inv(A); col == d: b -> theta
    const long arm = arms ? arms[slot] : slot;
    if (arm < 0 || arm >= K) return;
    const double* Aa = A + arm * d * d;
    double L[MD * MD], rhs[MD], z[MD], r[MD], dz[MD];
    for (int i = 0; i < d; ++i) {
        for (int j = 0; j <= i; ++j) {
            double v = Aa[i * d + j];
            for (int k = 0; k < j; ++k) v -= L[i * d + k] * L[j * d + k];
            L[i * d + j] = i == j ? sqrt(v) : v / L[j * d + j];
        }
    }
    for (int i = 0; i < d; ++i) rhs[i] = col < d ? (i == col ? 1.0 : 0.0) : b[arm * d + i];
    chol_solve(L, d, rhs, z);
    for (int it = 0; it < luRefine; ++it) {
        for (int i = 0; i < d; ++i) {
            dd acc{rhs[i], 0.0};
            for (int k = 0; k < d; ++k) dd_add_prod(acc, -Aa[i * d + k], z[k]);
            r[i] = dd_value(acc);
        }
        chol_solve(L, d, r, dz);
        for (int i = 0; i < d; ++i) z[i] += dz[i];
    }
    if (col < d) {
        for (int i = 0; i < d; ++i) A_inv[arm * d * d + i * d + col] = z[i];
    } else {
        for (int i = 0; i < d; ++i) theta[arm * d + i] = z[i];
    }
}

// mean = theta^T x and var = x^T X x of one arm, both as compensated dot products
__device__ __forceinline__ void arm_score(const double* __restrict__ X, const double* __restrict__ th, const double* xv, int d, double& mean,
                                          double& var) {
    dd m{0.0, 0.0}, v{0.0, 0.0};
    for (int i = 0; i < d; ++i) {
        dd_add_prod(m, th[i], xv[i]);
        dd row{0.0, 0.0};
        for (int j = 0; j < d; ++j) dd_add_prod(row, X[i * d + j], xv[j]);
        const double p = xv[i] * row.hi;
        dd_add(v, p, fma(xv[i], row.hi, -p) + xv[i] * row.lo);
    }
    mean = dd_value(m);
    var = dd_value(v);
}

__global__ __launch_bounds__(luThreads) void linucb_score_kernel(const double* __restrict__ A_inv, const double* __restrict__ theta, int K, int d,
                                                                 const double* __restrict__ users, const double* __restrict__ item_feats,
                                                                 const double* __restrict__ x_fixed, double alpha, int64_t* __restrict__ best_arm,
                                                                 double* __restrict__ best_mean, double* __restrict__ ucb_out,
                                                                 double* __restrict__ mean_out, double* __restrict__ var_out) {
    __shared__ double s_ucb[luThreads], s_mean[luThreads];
    __shared__ int s_arm[luThreads];
    const int tid = threadIdx.x;
    const long u = blockIdx.x;
    double xv[luMaxD];
    if (x_fixed) {
        for (int i = 0; i < d; ++i) xv[i] = x_fixed[i];
    } else {
        xv[0] = users[u];
    }
    double top = 0.0, top_mean = 0.0;
    int top_arm = -1;
    for (int arm = tid; arm < K; arm += luThreads) {
        if (!x_fixed) {
            xv[1] = (double)arm;
            for (int i = 2; i < d; ++i) xv[i] = item_feats[(long)arm * (d - 2) + (i - 2)];
        }
        double mean, var;
        arm_score(A_inv + (long)arm * d * d, theta + (long)arm * d, xv, d, mean, var);
        const double ucb = mean + alpha * sqrt(var);
        if (ucb_out) ucb_out[u * K + arm] = ucb;
        if (mean_out) mean_out[u * K + arm] = mean;
        if (var_out) var_out[u * K + arm] = var;
        if (top_arm < 0 || ucb > top) { top = ucb; top_mean = mean; top_arm = arm; }      // arms ascend: the first maximum stays
    }
    s_ucb[tid] = top; s_mean[tid] = top_mean; s_arm[tid] = top_arm;
    __syncthreads();
    for (int half = luThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
            const int oa = s_arm[tid + half], ma = s_arm[tid];
            if (oa >= 0 && (ma < 0 || s_ucb[tid + half] > s_ucb[tid] || (s_ucb[tid + half] == s_ucb[tid] && oa < ma))) {
                s_ucb[tid] = s_ucb[tid + half]; s_mean[tid] = s_mean[tid + half]; s_arm[tid] = oa;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (best_arm) best_arm[u] = s_arm[0];
        if (best_mean) best_mean[u] = s_mean[0];
    }
}

__global__ __launch_bounds__(luThreads) void linucb_predict_kernel(const double* __restrict__ theta, int K, int d, const double* __restrict__ x,
                                                                   long ld, const int64_t* __restrict__ arm, long n, double* __restrict__ y_pred) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const long a = arm[r];
    double out = 0.0;
    if (a >= 0 && a < K) {
        dd m{0.0, 0.0};
        for (int i = 0; i < d; ++i) dd_add_prod(m, theta[a * d + i], x[r * ld + i]);
        out = dd_value(m);
    }
    y_pred[r] = out;
}

static int linucb_check_d(int32_t d) {
    if (d < luMinD || d > luMaxD) return fail(CIRS_E_UNSUPPORTED, "linucb: d must lie in [2, 16]");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_linucb_update(double* A, double* b, int32_t n_arms, int32_t d, const double* x, int64_t ld, int64_t n_rows, const double* y,
                                  const int64_t* order, int64_t m, const int64_t* seg, void* stream) {
    using namespace cirs;
    if (int rc = linucb_check_d(d)) return rc;
    CIRS_REQUIRE(n_arms >= 0 && m >= 0 && n_rows >= 0, "linucb update: negative size");
    if (n_arms == 0 || m == 0) return CIRS_OK;
    CIRS_REQUIRE(A && b && x && y && order && seg, "linucb update: null pointer");
    CIRS_REQUIRE(ld >= d, "linucb update: ld < d");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(n_arms, luThreads / CIRS_WAVE)), block(luThreads);
    switch (cdiv(d * d + d, CIRS_WAVE)) {
        case 1: hipLaunchKernelGGL(linucb_update_kernel<1>, grid, block, 0, s, A, b, n_arms, d, x, (long)ld, (long)n_rows, y, order, (long)m, seg); break;
        case 2: hipLaunchKernelGGL(linucb_update_kernel<2>, grid, block, 0, s, A, b, n_arms, d, x, (long)ld, (long)n_rows, y, order, (long)m, seg); break;
        case 3: hipLaunchKernelGGL(linucb_update_kernel<3>, grid, block, 0, s, A, b, n_arms, d, x, (long)ld, (long)n_rows, y, order, (long)m, seg); break;
        case 4: hipLaunchKernelGGL(linucb_update_kernel<4>, grid, block, 0, s, A, b, n_arms, d, x, (long)ld, (long)n_rows, y, order, (long)m, seg); break;
        default: hipLaunchKernelGGL(linucb_update_kernel<5>, grid, block, 0, s, A, b, n_arms, d, x, (long)ld, (long)n_rows, y, order, (long)m, seg); break;
    }
    CIRS_CHECK_LAUNCH("linucb_update_kernel");
    return CIRS_OK;
}

extern "C" int cirs_linucb_solve(const double* A, const double* b, int32_t n_arms, int32_t d, const int32_t* arms, int32_t n_listed, double* A_inv,
                                 double* theta, void* stream) {
    using namespace cirs;
    if (int rc = linucb_check_d(d)) return rc;
    CIRS_REQUIRE(n_arms >= 0 && n_listed >= 0, "linucb solve: negative size");
    const long todo = arms ? n_listed : n_arms;
    if (n_arms == 0 || todo == 0) return CIRS_OK;
    CIRS_REQUIRE(A && b && A_inv && theta, "linucb solve: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(todo * (d + 1), luThreads)), block(luThreads);
    if (d == 7)
        hipLaunchKernelGGL(linucb_solve_kernel<7>, grid, block, 0, s, A, b, d, arms, todo, n_arms, A_inv, theta);
    else
        hipLaunchKernelGGL(linucb_solve_kernel<0>, grid, block, 0, s, A, b, d, arms, todo, n_arms, A_inv, theta);
    CIRS_CHECK_LAUNCH("linucb_solve_kernel");
    return CIRS_OK;
}

extern "C" int cirs_linucb_score(const double* A_inv, const double* theta, int32_t n_arms, int32_t d, const double* users, int32_t n_users,
                                 const double* item_feats, const double* x_fixed, double alpha, int64_t* best_arm, double* best_mean,
                                 double* ucb_out, double* mean_out, double* var_out, void* stream) {
    using namespace cirs;
    if (int rc = linucb_check_d(d)) return rc;
    CIRS_REQUIRE(n_arms >= 0 && n_users >= 0, "linucb score: negative size");
    const int rows = x_fixed ? 1 : n_users;
    if (n_arms == 0 || rows == 0) return CIRS_OK;
    CIRS_REQUIRE(A_inv && theta, "linucb score: null pointer");
    CIRS_REQUIRE(x_fixed || (users && (d == 2 || item_feats)), "linucb score: users / item_feats null");
    hipLaunchKernelGGL(linucb_score_kernel, dim3((unsigned)rows), dim3(luThreads), 0, (hipStream_t)stream, A_inv, theta, n_arms, d, users, item_feats,
                       x_fixed, alpha, best_arm, best_mean, ucb_out, mean_out, var_out);
    CIRS_CHECK_LAUNCH("linucb_score_kernel");
    return CIRS_OK;
}

extern "C" int cirs_linucb_predict(const double* theta, int32_t n_arms, int32_t d, const double* x, int64_t ld, const int64_t* arm, int64_t n,
                                   double* y_pred, void* stream) {
    using namespace cirs;
    if (int rc = linucb_check_d(d)) return rc;
    CIRS_REQUIRE(n_arms >= 0 && n >= 0, "linucb predict: negative size");
    if (n == 0) return CIRS_OK;
    CIRS_REQUIRE(theta && x && arm && y_pred, "linucb predict: null pointer");
    CIRS_REQUIRE(ld >= d, "linucb predict: ld < d");
    hipLaunchKernelGGL(linucb_predict_kernel, dim3((unsigned)cdiv(n, luThreads)), dim3(luThreads), 0, (hipStream_t)stream, theta, n_arms, d, x, (long)ld,
                       arm, (long)n, y_pred);
    CIRS_CHECK_LAUNCH("linucb_predict_kernel");
    return CIRS_OK;
}
