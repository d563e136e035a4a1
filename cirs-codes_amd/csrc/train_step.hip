// train_step.hip -- grad_adam_kernel and its launcher: the weight-gradient + Adam launch of an optimiser step of both VirtualTaobao
// trainers (train_step.h describes the scheme; mmoe_train.hip and mlp_train.hip build the job tables).
#include "train_step.h"

namespace cirs {
namespace tstep {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(kThreads) void grad_adam_kernel(float* __restrict__ P, float* __restrict__ G, float* __restrict__ M,
                                                             float* __restrict__ V, Jobs jobs, int n, AdamArgs a, Tail tail) {
    __shared__ float part[3][17][64];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == jobs.n_tiles) {
        // linear_model.weight: decayed by both regulariser lists, no data gradient (UserModel_MMOE's forward never reads it)
        if (tid < tail.lin_n) {
            const float pi = P[tail.lin_model + tid];
            adam_one(P, G, M, V, tail.lin_model + tid, 2.0f * a.l2_linear * pi, 2.0f * a.l2_all, a);
        }
        if (tid == 128) {
            double sum = 0.0;
            for (int c = 0; c < tail.n_loss_cols; ++c) {
                double t = 0.0;
                for (int q = 0; q < tail.n_row_tiles; ++q) t += tail.loss_part[q * tail.n_loss_cols + c];
                sum += t / tail.loss_div[c];
            }
            tail.loss_out[0] = (float)sum;
        }
        if (tid == 192) {
            double t = 0.0;
            for (int q = 0; q < kRegChunks; ++q) t += tail.reg_part[q];
            tail.loss_out[1] = (float)t;
        }
        return;
    }
    int ji = 0;
#pragma unroll
    for (int q = 1; q < kMaxJobs; ++q)
        if (q < jobs.n_jobs && (int)blockIdx.x >= jobs.j[q].tile0) ji = q;
    const Job& J = jobs.j[ji];
    const int t = blockIdx.x - J.tile0;
    const int o0 = (t / J.k_tiles) * 32, k0 = (t % J.k_tiles) * 32;
    const int wave = tid >> 6, lane = tid & 63, hi = lane >> 5, lo = lane & 31;
    const int rps = (((n + 3) / 4) + 1) & ~1;     // rows per slab (even): wave w owns rows [w * rps, min(n, (w + 1) * rps))
    const int r_beg = wave * rps, r_end = min(n, r_beg + rps);
    const int o = o0 + lo, k = k0 + lo;
    const bool o_ok = o < J.O, k_ok = k < J.K;
    f32x16 acc;
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.f;
    float bsum = 0.f;
    for (int r = r_beg; r < r_end; r += 32) {   // 16 MFMA steps (32 rows) per batch: the loads go out first, row order unchanged
        float av[16], bv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int rr = r + 2 * j + hi;
            const bool r_ok = rr < r_end;
            av[j] = (r_ok && o_ok) ? J.Lm[(size_t)rr * J.ldl + o] : 0.f;
            bv[j] = (r_ok && k_ok) ? J.Rm[(size_t)rr * J.ldr + k] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            bsum += av[j];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
        }
    }
    bsum += __shfl_xor(bsum, 32, CIRS_WAVE);
    if (wave > 0) {
#pragma unroll
        for (int s = 0; s < 16; ++s) part[wave - 1][s][lane] = acc[s];
        part[wave - 1][16][lane] = bsum;
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = (acc[s] + part[0][s][lane]) + (part[1][s][lane] + part[2][s][lane]);
    bsum = (bsum + part[0][16][lane]) + (part[1][16][lane] + part[2][16][lane]);
    const float c2 = 2.0f * a.l2_all;
    if (k_ok) {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int oo = o0 + (s & 3) + 8 * (s >> 2) + 4 * hi;
            if (oo < J.O) adam_one(P, G, M, V, J.p_off + oo * J.si + k * J.sj, acc[s], c2, a);
        }
    }
    if (k0 == 0 && J.b_off >= 0 && hi == 0 && o < J.b_n) adam_one(P, G, M, V, J.b_off + o, bsum, c2, a);
}

int launch_grad_adam(float* params, float* grads, float* adam_m, float* adam_v, const Jobs& jobs, int n, const AdamArgs& a, const Tail& tail,
                     hipStream_t s) {
    hipLaunchKernelGGL(grad_adam_kernel, dim3(jobs.n_tiles + 1), dim3(kThreads), 0, s, params, grads, adam_m, adam_v, jobs, n, a, tail);
    CIRS_CHECK_LAUNCH("grad_adam_kernel");
    return CIRS_OK;
}

}  // namespace tstep
}  // namespace cirs
