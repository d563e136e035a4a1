// optim.h -- what every optimiser kernel of the library shares, once:
//   adam_bias           the bias corrections of torch.optim.Adam for step t, formed in fp64 on the host and rounded to float (torch forms them
//                       once per step on the host; no kernel raises a power).
//   adam_update         torch's element update (_single_tensor_adam: lerp_, mul_ / addcmul_, addcdiv_) on registers, with the correctly
//                       rounded division and square root: adam_l2_kernel (table_step.h) and adam_kernel (ppo.hip).  tstep::adam_one
//                       (train_step.h) has the same statements on its buffers: through the register form its kernel was scheduled
//                       differently and measured slower.  ppo.hip's adam_elem, the documented fast form on the hardware reciprocal and
//                       square root, and vtb_learn.hip's update, whose second moment is one fused multiply-add, are different bits.
//   clip_coef           the coefficient of clip_grad_norm_ from the total norm.
//   block_sum<N>        the fixed-order halving tree over the N threads of a workgroup.  Every sum across a workgroup has this tree's
//                       order, which is why two runs of anything in this library give the same bits.  Four sites keep the tree written
//                       out: adam_next_rest (ppo.hip: three loss terms and the norm), loss_means4 (deepfm_tower.h: four loss terms)
//                       and validate_final_kernel (userval.hip: two fp64 sums), where several sums share the tree's barriers, and
//                       norm_coef_block (ppo.hip), which does without the closing barrier.  The arg-max of static_policy.hip and
//                       the (min, max) of deepfm.hip are halving trees of another operation.  The measurements behind the two that
//                       were tried with block_sum are in profiles/r09_optim_refactor_ab.md.
#pragma once
#include <cmath>

#include "common.h"

namespace cirs {

struct AdamBias {
    float step_size;   // lr / (1 - beta1^t)
    float bc2s;        // sqrt(1 - beta2^t)
    float rbc2s;       // 1 / sqrt(1 - beta2^t)
};
inline AdamBias adam_bias(float lr, float beta1, float beta2, int64_t t) {
    const double td = (double)t;
    const double s2 = sqrt(1.0 - pow((double)beta2, td));
    AdamBias b;
    b.step_size = (float)((double)lr / (1.0 - pow((double)beta1, td)));
    b.bc2s = (float)s2;
    b.rbc2s = (float)(1.0 / s2);
    return b;
}

__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, float step_size, float bc2s, float beta1, float beta2, float eps) {
    m = m + (1.0f - beta1) * (g - m);                      // exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + (1.0f - beta2) * g * g;                // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    p = p - step_size * (m / (sqrtf(v) / bc2s + eps));     // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ float clip_coef(float total_norm, float max_grad_norm) { return fminf(max_grad_norm / (total_norm + 1e-6f), 1.0f); }

// sum of one value per thread of a workgroup of N threads (sh: N elements of LDS): sh[t] += sh[t + s] for s = N/2, N/4, .. 1.  Every thread
// gets the sum, and the last barrier lets the caller reuse sh at once.  Contract: a one-dimensional workgroup of exactly N threads (the
// kernel's __launch_bounds__(N) launch), N a power of two, and EVERY thread of it reaches the call (it holds barriers).
template <int N, class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
    static_assert(N >= 2 && (N & (N - 1)) == 0, "block_sum: N is a power of two");
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

}  // namespace cirs
