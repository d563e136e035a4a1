// train_step.h -- the back half of an optimiser step, shared by the VirtualTaobao trainers (mmoe_train.hip: the one-task MMoE user
// model; mlp_train.hip: the two-task MLP baselines).  Each trainer keeps its own row kernel (forward, loss, backward down to the
// pre-activation gradients, per-row operands to the workspace) and describes its weight gradients as a table of jobs; everything
// after that exists once, here and in train_step.hip:
//   reg_chunks          the regulariser of the CURRENT parameters as 64 fixed chunks (fp64 partials), run by eight extra workgroups
//                       of either row kernel.
//   grad_adam_kernel    one workgroup per 32 x 32 tile of a weight matrix: dW = dZ^T A over the batch rows on the fp32 matrix cores
//                       (v_mfma_f32_32x32x2_f32, operand layout of small_gemm.h), the rows split into four contiguous slabs (one
//                       wavefront each) whose accumulators are added as (s0 + s1) + (s2 + s3); bias gradients as column sums in the
//                       same waves; then g += 2 l2 p and torch.optim.Adam on the tile's own parameters.  The last workgroup decays
//                       the unused duplicate `linear_model.weight` (no data gradient) and sums the loss / regulariser partials in
//                       index order into loss_out.
//   run_steps           the argument checks of the _step / _epoch entries and the back-to-back loop over the batches.
// The bias corrections (adam_bias) and the block sum (block_sum) are optim.h's; adam_one states optim.h's adam_update on the buffers.
// Every sum has a fixed order and there are no float atomics.
#pragma once
#include "common.h"
#include "optim.h"

namespace cirs {
namespace tstep {

constexpr int kThreads = 256;
constexpr int kRegChunks = 64, kRegBlocks = 8;
constexpr int kMaxJobs = CIRS_VTB_STATIC_MAX_DNN + 4;   // the larger trainer: hidden layers, experts | gates, two towers, linear_model_task
constexpr int kMaxLossCols = 2;

// regulariser of the current parameters by workgroups first_block .. first_block + kRegBlocks - 1: chunk c covers [c * cs, (c + 1) * cs);
// red: kThreads doubles of LDS
__device__ __forceinline__ void reg_chunks(const float* __restrict__ P, int total, int lin_model, int lin_task, float l2_linear, float l2_all,
                                           int first_block, double* red, double* __restrict__ reg_part) {
    const int tid = threadIdx.x;
    const int cs = (total + kRegChunks - 1) / kRegChunks;
    for (int c = blockIdx.x - first_block; c < kRegChunks; c += kRegBlocks) {
        const int lo = c * cs, hi = min(total, lo + cs);
        double acc = 0.0;
        for (int i = lo + tid; i < hi; i += kThreads) {
            const double p = (double)P[i];
            const double coef = (double)l2_all + (i >= lin_model && i < lin_task ? (double)l2_linear : 0.0);   // linear_model.weight is in both lists
            acc = fma(coef * p, p, acc);
        }
        const double t = block_sum<kThreads>(acc, red);
        if (tid == 0) reg_part[c] = t;
    }
}

// one weight-gradient problem: G[i][j] = sum_r Lm[r][i] Rm[r][j], i < O, j < K; parameter of (i, j) at p_off + i * si + j * sj;
// b_off >= 0: parameter b_off + i, i < b_n, takes sum_r Lm[r][i] (bias)
struct Job {
    const float *Lm, *Rm;
    int ldl, ldr, O, K, p_off, si, sj, b_off, b_n, tile0, k_tiles;
};
struct Jobs {
    Job j[kMaxJobs];
    int n_jobs, n_tiles;
};
inline void add_job(Jobs& jobs, const float* Lm, int ldl, int O, const float* Rm, int ldr, int K, int p_off, int si, int sj, int b_off, int b_n) {
    Job& J = jobs.j[jobs.n_jobs++];
    J.Lm = Lm; J.ldl = ldl; J.O = O; J.Rm = Rm; J.ldr = ldr; J.K = K; J.p_off = p_off; J.si = si; J.sj = sj; J.b_off = b_off; J.b_n = b_n;
    J.tile0 = jobs.n_tiles; J.k_tiles = (K + 31) / 32;
    jobs.n_tiles += ((O + 31) / 32) * J.k_tiles;
}

struct AdamArgs {
    float beta1, beta2, eps, step_size, bc2s, l2_linear, l2_all;
};
inline AdamArgs adam_args(float lr, float beta1, float beta2, float eps, float l2_linear, float l2_all, int64_t step_before) {
    const AdamBias b = adam_bias(lr, beta1, beta2, step_before + 1);
    AdamArgs a;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.l2_linear = l2_linear; a.l2_all = l2_all;
    a.step_size = b.step_size; a.bc2s = b.bc2s;
    return a;
}

__device__ __forceinline__ void adam_one(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int i,
                                         float data_grad, float c2, const AdamArgs& a) {
    // adam_update's statements (optim.h) on the buffers themselves: through the register form grad_adam_kernel is scheduled differently and the
    // 100-row epoch of the (128, 128) MMoE trainer took 58.13 us per step against 57.88 us (profiles/r09_optim_refactor_ab.md)
    const float pi = p[i];
    const float gi = __builtin_fmaf(c2, pi, data_grad);   // d/dp of l2 * p^2 joins the data gradient
    const float mi = m[i] + (1.0f - a.beta1) * (gi - m[i]);
    const float vi = v[i] * a.beta2 + (1.0f - a.beta2) * gi * gi;
    g[i] = gi; m[i] = mi; v[i] = vi;
    p[i] = pi - a.step_size * (mi / (sqrtf(vi) / a.bc2s + a.eps));
}

// the work of grad_adam_kernel's last workgroup: the lin_n parameters of `linear_model.weight` at lin_model, and
// loss_out = {sum over the loss columns c, in order, of (sum over the row tiles q, in order, of loss_part[q * n_loss_cols + c]) / loss_div[c],
//             sum of the kRegChunks entries of reg_part}
struct Tail {
    int lin_model, lin_n, n_row_tiles, n_loss_cols;
    double loss_div[kMaxLossCols];
    const double *loss_part, *reg_part;
    float* loss_out;
};

// launches grad_adam_kernel (train_step.hip) on n batch rows: jobs.n_tiles + 1 workgroups
int launch_grad_adam(float* params, float* grads, float* adam_m, float* adam_v, const Jobs& jobs, int n, const AdamArgs& a, const Tail& tail,
                     hipStream_t s);

// what the _step and _epoch entries of both trainers share after their check_cfg: the argument checks, in the entries' order, and the
// loop over the batches of `batch_size` rows of n_order (the last one short).  launch(st, r0, n) queues step `st` on rows r0 .. r0 + n - 1;
// the steps are queued back to back: the host never waits for the device.  need_bytes: the workspace of the largest batch.
template <class Launch>
int run_steps(const void* params, const void* grads, const void* adam_m, const void* adam_v, const void* loss_out, const void* workspace,
              bool cols_ok, const char* cols_msg, bool sizes_ok, const char* sizes_msg, int64_t step_before, int64_t workspace_bytes,
              int64_t need_bytes, int64_t n_order, int64_t batch_size, Launch launch) {
    CIRS_REQUIRE(params && grads && adam_m && adam_v && loss_out && workspace, "null argument");
    CIRS_REQUIRE(cols_ok, cols_msg);
    CIRS_REQUIRE(sizes_ok, sizes_msg);
    CIRS_REQUIRE(step_before >= 0, "negative step count");
    CIRS_REQUIRE(((uintptr_t)params & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "params and workspace must be 16-byte aligned");
    CIRS_REQUIRE(workspace_bytes >= need_bytes, "workspace too small");
    int64_t st = 0;
    for (int64_t r0 = 0; r0 < n_order; r0 += batch_size, ++st) {
        const int n = (int)(n_order - r0 < batch_size ? n_order - r0 : batch_size);
        if (int rc = launch(st, r0, n)) return rc;
    }
    return CIRS_OK;
}

}  // namespace tstep
}  // namespace cirs
