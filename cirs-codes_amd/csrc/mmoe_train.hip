// mmoe_train.hip -- training of the VirtualTaobao MMoE user model (CIRS-UserModel-taobao.py) on the device:
//   cirs_mmoe_train_step / _epoch   one optimiser step of UserModel_MMOE.fit_data's inner loop (reference core/user_model.py:150-170,
//                                   core/user_model_mmoe.py:144-233, core/layers.py MMOELayer / Linear, loss_taobao of
//                                   CIRS-UserModel-taobao.py:185-191) for the all-dense one-regression-task build.
//   cirs_vtb_exposure_history       compute_exposure_effect_virtualTaobao (CIRS-UserModel-taobao.py:52-70).
//
// A step is a latency chain on a 15 k - 36 k parameter model, so it is TWO launches:
//   mmoe_rows_kernel       one workgroup per tile of 16 batch rows: forward (activations in LDS), the rows' loss terms and
//                          d loss / d y_pred, backward down to the pre-activation gradients of both hidden layers.  Per-row
//                          operands of the weight gradients (x, h1, h2, mixture, dz1, dz2, d experts | d gate, dy) go to the
//                          workspace; the tile's loss sum (fp64) to a partial.  Eight more workgroups compute the
//                          regulariser of the CURRENT parameters as 64 fixed chunks (fp64 partials).
//   grad_adam_kernel       (train_step.h, shared with mlp_train.hip) dW = dZ^T A of the six jobs listed in launch_step on the matrix
//                          cores, bias gradients, g += 2 l2 p and torch.optim.Adam; its last workgroup decays the unused duplicate
//                          `linear_model.weight` and sums the loss / regulariser partials in index order into loss_out.
// Every sum has a fixed order and there are no float atomics: two runs from one state give identical bits, and an epoch
// (the same two launches per step, queued back to back without any host synchronisation) equals the step-by-step loop bit for bit.
#include <vector>

#include "common.h"
#include "train_step.h"

namespace cirs {
namespace mmt {

constexpr int kIn = 118, kExperts = 4, kExpertDim = 8, kEx = kExperts * kExpertDim, kEg = kEx + kExperts;
constexpr int kTile = 16, kThreads = 256, kLd = 132, kLdE = 40;
static_assert(kThreads == tstep::kThreads, "reg_chunks runs in the row kernel's workgroups");

struct Layout {  // offsets (floats) into the flat parameter / gradient / moment buffers
    int w2, we, wg, w1t, b1, b2, be, wt, lin_model, lin_task, out_bias, total;
};
__host__ __device__ inline Layout layout(int H1, int H2) {   // the matrices read in float4 pieces first: their offsets are multiples of 4
    Layout L;
    int o = 0;
    L.w2 = o; o += H2 * H1;
    L.we = o; o += kEx * H2;
    L.wg = o; o += kExperts * H2;
    L.w1t = o; o += kIn * H1;
    L.b1 = o; o += H1; L.b2 = o; o += H2; L.be = o; o += kEx;
    L.wt = o; o += kExpertDim;
    L.lin_model = o; o += kIn;
    L.lin_task = o; o += kIn;
    L.out_bias = o; o += 1;
    L.total = o;
    return L;
}

struct Rows {  // per-row outputs of mmoe_rows_kernel
    float *X, *H1, *H2, *M, *DZ1, *DZ2, *DEG, *DY;  // [n,118] [n,H1] [n,H2] [n,8] [n,H1] [n,H2] [n,36] [n]
    double *loss_part, *reg_part;                   // [tiles] [tstep::kRegChunks]
};

// Y[s][o] = relu(b[o] + sum_k X[s][k] Wt[k][o]): weights stored [K][O], lanes o read consecutive dwords
__device__ __forceinline__ void fwd_t(const float* __restrict__ Wt, const float* __restrict__ b, const float* X, int K, int O, float* Y) {
    for (int u = threadIdx.x; u < O * (kTile / 4); u += kThreads) {
        const int o = u % O, g = u / O;
        const float* x = X + 4 * g * kLd;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
        for (int k = 0; k < K; ++k) {
            const float w = Wt[k * O + o];
            a0 = __builtin_fmaf(x[k], w, a0);
            a1 = __builtin_fmaf(x[kLd + k], w, a1);
            a2 = __builtin_fmaf(x[2 * kLd + k], w, a2);
            a3 = __builtin_fmaf(x[3 * kLd + k], w, a3);
        }
        const float bias = b[o];
        Y[(4 * g) * kLd + o] = fmaxf(a0 + bias, 0.f);
        Y[(4 * g + 1) * kLd + o] = fmaxf(a1 + bias, 0.f);
        Y[(4 * g + 2) * kLd + o] = fmaxf(a2 + bias, 0.f);
        Y[(4 * g + 3) * kLd + o] = fmaxf(a3 + bias, 0.f);
    }
    __syncthreads();
}

// Y[s][o] = act(b[o] + sum_k X[s][k] W[o][k]): torch layout [O][K], K % 4 == 0; every lane walks its own row in float4 pieces
template <bool kRelu>
__device__ __forceinline__ void fwd_n(const float* __restrict__ W, const float* __restrict__ b, const float* X, int K, int O, float* Y, int ldy) {
    for (int u = threadIdx.x; u < O * (kTile / 4); u += kThreads) {
        const int o = u % O, g = u / O;
        const float* x = X + 4 * g * kLd;
        const float4* wr = reinterpret_cast<const float4*>(W + (size_t)o * K);
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k4 = 0; k4 < K / 4; ++k4) {
            const float4 w = wr[k4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 xv = *reinterpret_cast<const float4*>(x + i * kLd + 4 * k4);
                a[i] = __builtin_fmaf(xv.x, w.x, a[i]);
                a[i] = __builtin_fmaf(xv.y, w.y, a[i]);
                a[i] = __builtin_fmaf(xv.z, w.z, a[i]);
                a[i] = __builtin_fmaf(xv.w, w.w, a[i]);
            }
        }
        const float bias = b ? b[o] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float y = a[i] + bias;
            Y[(4 * g + i) * ldy + o] = kRelu ? fmaxf(y, 0.f) : y;
        }
    }
    __syncthreads();
}

// DZ[s][k] = (H[s][k] > 0) * sum_o D[s][o] W[o][k]: torch layout [O][K], lanes k read consecutive dwords.  D rows have stride ldd.
__device__ __forceinline__ void bwd_n(const float* __restrict__ W, const float* D, int ldd, int O, int K, const float* H, float* DZ) {
    for (int u = threadIdx.x; u < K * (kTile / 4); u += kThreads) {
        const int k = u % K, g = u / K;
        const float* d = D + 4 * g * ldd;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
        for (int o = 0; o < O; ++o) {
            const float w = W[(size_t)o * K + k];
            a0 = __builtin_fmaf(d[o], w, a0);
            a1 = __builtin_fmaf(d[ldd + o], w, a1);
            a2 = __builtin_fmaf(d[2 * ldd + o], w, a2);
            a3 = __builtin_fmaf(d[3 * ldd + o], w, a3);
        }
        DZ[(4 * g) * kLd + k] = H[(4 * g) * kLd + k] > 0.f ? a0 : 0.f;
        DZ[(4 * g + 1) * kLd + k] = H[(4 * g + 1) * kLd + k] > 0.f ? a1 : 0.f;
        DZ[(4 * g + 2) * kLd + k] = H[(4 * g + 2) * kLd + k] > 0.f ? a2 : 0.f;
        DZ[(4 * g + 3) * kLd + k] = H[(4 * g + 3) * kLd + k] > 0.f ? a3 : 0.f;
    }
    __syncthreads();
}

struct alignas(16) RowsSmem {
    float x[kTile * kLd], h1[kTile * kLd], h2[kTile * kLd], dz2[kTile * kLd], dz1[kTile * kLd];
    float eg[kTile * kLdE], deg[kTile * kLdE];   // experts (column d * 4 + e) | gate logits;  their gradients
    double rowloss[kTile];
};

// data rows: x [N,118], y [N], exposure [N]; batch row r is data row idx[r0 + r] (idx null: r0 + r); rows outside [0, N) read row 0
__global__ __launch_bounds__(kThreads) void mmoe_rows_kernel(const float* __restrict__ P, int H1, int H2, const float* __restrict__ x,
                                                             const float* __restrict__ y, const float* __restrict__ exposure,
                                                             const int64_t* __restrict__ idx, long r0, long N, int n, int n_tiles,
                                                             float l2_linear, float l2_all, Rows out) {
    __shared__ RowsSmem S;
    __shared__ double red[kThreads];
    const Layout L = layout(H1, H2);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_tiles) {
        tstep::reg_chunks(P, L.total, L.lin_model, L.lin_task, l2_linear, l2_all, n_tiles, red, out.reg_part);
        return;
    }
    const int row0 = blockIdx.x * kTile;
    for (int i = tid; i < kTile * kIn; i += kThreads) {
        const int s = i / kIn, k = i % kIn;
        float v = 0.f;
        if (row0 + s < n) {
            long src = idx ? (long)idx[r0 + row0 + s] : r0 + row0 + s;
            if (src < 0 || src >= N) src = 0;
            v = x[src * kIn + k];
            out.X[(size_t)(row0 + s) * kIn + k] = v;
        }
        S.x[s * kLd + k] = v;
    }
    __syncthreads();
    fwd_t(P + L.w1t, P + L.b1, S.x, kIn, H1, S.h1);
    fwd_n<true>(P + L.w2, P + L.b2, S.h1, H1, H2, S.h2, kLd);
    // experts and gate logits in one pass: 36 outputs per row (we | be | wg are laid out so that the gate rows follow `be`)
    for (int u = tid; u < kEg * (kTile / 4); u += kThreads) {
        const int o = u % kEg, g = u / kEg;
        const float* hx = S.h2 + 4 * g * kLd;
        const float4* wr = reinterpret_cast<const float4*>(o < kEx ? P + L.we + (size_t)o * H2 : P + L.wg + (size_t)(o - kEx) * H2);
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k4 = 0; k4 < H2 / 4; ++k4) {
            const float4 w = wr[k4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 xv = *reinterpret_cast<const float4*>(hx + i * kLd + 4 * k4);
                a[i] = __builtin_fmaf(xv.x, w.x, a[i]);
                a[i] = __builtin_fmaf(xv.y, w.y, a[i]);
                a[i] = __builtin_fmaf(xv.z, w.z, a[i]);
                a[i] = __builtin_fmaf(xv.w, w.w, a[i]);
            }
        }
        const float bias = o < kEx ? P[L.be + o] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) S.eg[(4 * g + i) * kLdE + o] = a[i] + bias;
    }
    __syncthreads();
    // per row: gate softmax, mixture, tower, prediction, loss term, d loss / d y_pred, gradients of the experts and gate logits
    if (tid < kTile) {
        const int s = tid, r = row0 + s;
        double term = 0.0;
        float* dg = S.deg + s * kLdE;
        if (r < n) {
            long src = idx ? (long)idx[r0 + r] : r0 + r;
            if (src < 0 || src >= N) src = 0;
            const float* ex = S.eg + s * kLdE;
            const float* gl = ex + kEx;
            float mx = gl[0];
            for (int e = 1; e < kExperts; ++e) mx = fmaxf(mx, gl[e]);
            float p[kExperts], sum = 0.f;
            for (int e = 0; e < kExperts; ++e) { p[e] = expf(gl[e] - mx); sum += p[e]; }
            for (int e = 0; e < kExperts; ++e) p[e] = p[e] / sum;
            float m[kExpertDim], tower = 0.f;
            for (int d = 0; d < kExpertDim; ++d) {
                float md = 0.f;
                for (int e = 0; e < kExperts; ++e) md = __builtin_fmaf(ex[d * kExperts + e], p[e], md);
                m[d] = md;
                tower = __builtin_fmaf(md, P[L.wt + d], tower);
                out.M[(size_t)r * kExpertDim + d] = md;
            }
            float lin = 0.f;
            for (int k = 0; k < kIn; ++k) lin = __builtin_fmaf(S.x[s * kLd + k], P[L.lin_task + k], lin);
            const float yp = (lin + tower) + P[L.out_bias];
            const float yt = y[src], inv = 1.0f / (1.0f + exposure[src]);
            const float diff = inv * yp - yt;
            term = (double)(diff * diff * (yt + 1.0f));
            const float dy = 2.0f * diff * (yt + 1.0f) * inv / (float)n;
            out.DY[r] = dy;
            float dp[kExperts] = {0.f, 0.f, 0.f, 0.f};
            for (int d = 0; d < kExpertDim; ++d) {
                const float dm = dy * P[L.wt + d];
                for (int e = 0; e < kExperts; ++e) {
                    dg[d * kExperts + e] = dm * p[e];
                    dp[e] = __builtin_fmaf(dm, ex[d * kExperts + e], dp[e]);
                }
            }
            float dot = 0.f;
            for (int e = 0; e < kExperts; ++e) dot = __builtin_fmaf(p[e], dp[e], dot);
            for (int e = 0; e < kExperts; ++e) dg[kEx + e] = p[e] * (dp[e] - dot);
            for (int c = 0; c < kEg; ++c) out.DEG[(size_t)r * kEg + c] = dg[c];
        } else {
            for (int c = 0; c < kEg; ++c) dg[c] = 0.f;
        }
        S.rowloss[s] = term;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < kTile; ++s) t += S.rowloss[s];
        out.loss_part[blockIdx.x] = t;
    }
    // d h2 = d experts We + d gate Wg  (36 contraction terms: the gate rows follow the expert rows in `deg`), through relu
    for (int u = tid; u < H2 * (kTile / 4); u += kThreads) {
        const int k = u % H2, g = u / H2;
        const float* d = S.deg + 4 * g * kLdE;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int o = 0; o < kEg; ++o) {
            const float w = o < kEx ? P[L.we + (size_t)o * H2 + k] : P[L.wg + (size_t)(o - kEx) * H2 + k];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = __builtin_fmaf(d[i * kLdE + o], w, a[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) S.dz2[(4 * g + i) * kLd + k] = S.h2[(4 * g + i) * kLd + k] > 0.f ? a[i] : 0.f;
    }
    __syncthreads();
    bwd_n(P + L.w2, S.dz2, kLd, H2, H1, S.h1, S.dz1);
    for (int i = tid; i < kTile * H1; i += kThreads) {
        const int s = i / H1, k = i % H1;
        if (row0 + s < n) {
            out.H1[(size_t)(row0 + s) * H1 + k] = S.h1[s * kLd + k];
            out.DZ1[(size_t)(row0 + s) * H1 + k] = S.dz1[s * kLd + k];
        }
    }
    for (int i = tid; i < kTile * H2; i += kThreads) {
        const int s = i / H2, k = i % H2;
        if (row0 + s < n) {
            out.H2[(size_t)(row0 + s) * H2 + k] = S.h2[s * kLd + k];
            out.DZ2[(size_t)(row0 + s) * H2 + k] = S.dz2[s * kLd + k];
        }
    }
}

// compute_exposure_effect_virtualTaobao: one wavefront per row, lanes stride the session's earlier rows
__global__ __launch_bounds__(256) void vtb_exposure_kernel(const int64_t* __restrict__ start, const double* __restrict__ action, long n_rows,
                                                           double tau, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const long s0 = start[r];
    double acc = 0.0;
    if (tau > 0.0) {
        const double* ar = action + r * CIRS_VTB_ACTION_DIM;
        for (long j = s0 + lane; j < r; j += CIRS_WAVE) {
            const double* aj = action + j * CIRS_VTB_ACTION_DIM;
            double d2 = 0.0;
#pragma unroll
            for (int c = 0; c < CIRS_VTB_ACTION_DIM; ++c) {
                const double d = ar[c] - aj[c];
                d2 = fma(d, d, d2);
            }
            acc += exp(-(double)(r - j) * sqrt(d2) / tau);
        }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) out[r] = acc;
}

static int check_cfg(const cirs_mmoe_train_cfg* cfg) {
    CIRS_REQUIRE(cfg, "null cfg");
    if (cfg->d_in != kIn || cfg->n_experts != kExperts || cfg->expert_dim != kExpertDim || cfg->n_tasks != 1 || cfg->task_dim != 1)
        return fail(CIRS_E_UNSUPPORTED, "mmoe train: only the VirtualTaobao build is supported (118 dense inputs, 4 experts of dim 8, one regression task of logit dim 1)");
    if ((cfg->h1 != 64 && cfg->h1 != 128) || (cfg->h2 != 64 && cfg->h2 != 128))
        return fail(CIRS_E_UNSUPPORTED, "mmoe train: two hidden layers with widths from {64, 128}");
    return CIRS_OK;
}

static size_t ws_floats(const cirs_mmoe_train_cfg* cfg, long n) {
    auto pad = [](size_t c) { return (c + 3) & ~(size_t)3; };
    const long tiles = (n + kTile - 1) / kTile;
    return pad((size_t)n * kIn) + 2 * pad((size_t)n * cfg->h1) + 2 * pad((size_t)n * cfg->h2) + pad((size_t)n * kExpertDim) + pad((size_t)n * kEg) +
           pad((size_t)n) + 2 * pad((size_t)tiles) + 2 * tstep::kRegChunks + 64;
}

// the two launches of one step on batch rows r0 .. r0 + n - 1 of the index array (or of the data when idx is null)
static int launch_step(const cirs_mmoe_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t step_before,
                       const float* x, const float* y, const float* exposure, const int64_t* idx, long r0, long N, int n, float* loss_out,
                       void* workspace, hipStream_t s) {
    const int H1 = cfg->h1, H2 = cfg->h2;
    const Layout L = layout(H1, H2);
    const int tiles = (n + kTile - 1) / kTile;
    float* p = (float*)workspace;
    auto take = [&](size_t cnt) { float* r = p; p += (cnt + 3) & ~(size_t)3; return r; };
    Rows o;
    o.X = take((size_t)n * kIn); o.H1 = take((size_t)n * H1); o.DZ1 = take((size_t)n * H1); o.H2 = take((size_t)n * H2); o.DZ2 = take((size_t)n * H2);
    o.M = take((size_t)n * kExpertDim); o.DEG = take((size_t)n * kEg); o.DY = take(n);
    o.loss_part = (double*)take(2 * (size_t)tiles); o.reg_part = (double*)take(2 * tstep::kRegChunks);
    hipLaunchKernelGGL(mmoe_rows_kernel, dim3(tiles + tstep::kRegBlocks), dim3(kThreads), 0, s, (const float*)params, H1, H2, x, y, exposure, idx, r0, N, n,
                       tiles, cfg->l2_linear, cfg->l2_all, o);
    CIRS_CHECK_LAUNCH("mmoe_rows_kernel");
    tstep::Jobs jobs{};   // a job with a bias passes b_n = O
    tstep::add_job(jobs, o.DZ1, H1, H1, o.X, kIn, kIn, L.w1t, 1, H1, L.b1, H1);          // w1 is stored transposed: (o, k) at k * H1 + o
    tstep::add_job(jobs, o.DZ2, H2, H2, o.H1, H1, H1, L.w2, H1, 1, L.b2, H2);
    tstep::add_job(jobs, o.DEG, kEg, kEx, o.H2, H2, H2, L.we, H2, 1, L.be, kEx);
    tstep::add_job(jobs, o.DEG + kEx, kEg, kExperts, o.H2, H2, H2, L.wg, H2, 1, -1, 0);
    tstep::add_job(jobs, o.DY, 1, 1, o.X, kIn, kIn, L.lin_task, 0, 1, L.out_bias, 1);
    tstep::add_job(jobs, o.DY, 1, 1, o.M, kExpertDim, kExpertDim, L.wt, 0, 1, -1, 0);
    const tstep::Tail tail{L.lin_model, kIn, tiles, 1, {(double)n, 0.0}, o.loss_part, o.reg_part, loss_out};
    return tstep::launch_grad_adam(params, grads, adam_m, adam_v, jobs, n,
                                   tstep::adam_args(cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->l2_linear, cfg->l2_all, step_before), tail, s);
}

}  // namespace mmt
}  // namespace cirs

extern "C" int64_t cirs_mmoe_train_param_count(const cirs_mmoe_train_cfg* cfg) {
    if (cirs::mmt::check_cfg(cfg) != CIRS_OK) return 0;
    return cirs::mmt::layout(cfg->h1, cfg->h2).total;
}

extern "C" int64_t cirs_mmoe_train_workspace_bytes(const cirs_mmoe_train_cfg* cfg, int32_t n) {
    if (n <= 0 || cirs::mmt::check_cfg(cfg) != CIRS_OK) return 0;
    return (int64_t)cirs::mmt::ws_floats(cfg, n) * 4;
}

extern "C" int cirs_mmoe_train_step(const cirs_mmoe_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                                    int64_t step_before, const float* x, const float* y, const float* exposure, int32_t n, float* loss_out,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = mmt::check_cfg(cfg)) return rc;
    return tstep::run_steps(params, grads, adam_m, adam_v, loss_out, workspace, x && y && exposure, "null batch column", n >= 1, "empty batch",
                            step_before, workspace_bytes, cirs_mmoe_train_workspace_bytes(cfg, n), n, n, [&](int64_t, int64_t, int nb) {
                                return mmt::launch_step(cfg, params, grads, adam_m, adam_v, step_before, x, y, exposure, nullptr, 0, nb, nb, loss_out,
                                                        workspace, (hipStream_t)stream);
                            });
}

extern "C" int cirs_mmoe_train_epoch(const cirs_mmoe_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                                     int64_t step_before, const float* x, const float* y, const float* exposure, int64_t n_rows,
                                     const int64_t* order, int64_t n_order, int32_t batch_size, float* losses_out, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = mmt::check_cfg(cfg)) return rc;
    const int64_t bmax = batch_size < n_order ? batch_size : n_order;
    return tstep::run_steps(params, grads, adam_m, adam_v, losses_out, workspace, x && y && exposure && order, "null data column or index array",
                            n_rows >= 1 && n_order >= 1 && batch_size >= 1, "empty data set, index array or batch", step_before, workspace_bytes,
                            cirs_mmoe_train_workspace_bytes(cfg, (int32_t)bmax), n_order, batch_size, [&](int64_t st, int64_t r0, int nb) {
                                return mmt::launch_step(cfg, params, grads, adam_m, adam_v, step_before + st, x, y, exposure, order, r0, n_rows, nb,
                                                        losses_out + 2 * st, workspace, (hipStream_t)stream);
                            });
}

extern "C" int cirs_vtb_exposure_history(const int32_t* timestamp_host, const double* action, int64_t n_rows, double tau,
                                         int64_t* start_scratch, double* exposure_out, void* stream) {
    using namespace cirs;
    if (n_rows <= 0) return CIRS_OK;
    CIRS_REQUIRE(timestamp_host && action && start_scratch && exposure_out, "null argument");
    // the reference reads an undefined `start` for a row in front of the first session start: refuse such a log
    CIRS_REQUIRE(timestamp_host[0] == 1, "the first row of the log must open a session (timestamp column == 1)");
    std::vector<int64_t> start((size_t)n_rows);
    int64_t cur = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (timestamp_host[r] == 1) cur = r;
        start[(size_t)r] = cur;
    }
    CIRS_HIP(hipMemcpy(start_scratch, start.data(), sizeof(int64_t) * (size_t)n_rows, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mmt::vtb_exposure_kernel, dim3(cdiv(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, (const int64_t*)start_scratch, action,
                       (long)n_rows, tau, exposure_out);
    CIRS_CHECK_LAUNCH("vtb_exposure_kernel");
    return CIRS_OK;
}
