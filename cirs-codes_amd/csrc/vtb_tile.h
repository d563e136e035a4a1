// vtb_tile.h -- the pieces of the VirtualTaobao env that more than one kernel runs: sizes, the Philox noise convention, the
// row-tile dense layer and the user draw.  virtualtb.hip (one launch per vector step) and vtb_static.hip (one launch per whole
// evaluation) include it; each instantiates the templates for its own tile of rows, so the arithmetic of a row -- the order of
// every sum -- is the same in both and does not depend on the tile.
//
// Noise (INTEGRATION.md "Sampler noise"): Philox4x32-10, key = seed, counter = (env id, event, block, tag); tag 0 = the 21
// Gumbels of a step, tag 1 = a user draw (128 uniforms, then 88 Gumbels), tag 2 = the epsilon-greedy draw of the static-baseline
// evaluation (one uniform, then 27 exploration uniforms).
#pragma once
#include "common.h"
#include "rng.h"

namespace cirs {
namespace {

constexpr int kTile = 16;        // envs per workgroup of the step kernels
constexpr int kThreads = 256;
constexpr int kLd = 260;         // LDS row stride of the activation buffers (widest layer: 256)
constexpr int kUser = CIRS_VTB_USER_DIM, kAct = CIRS_VTB_ACTION_DIM, kGroups = CIRS_VTB_GROUPS;
constexpr int kZ = 128, kGenH = 128;
constexpr int kActIn = kUser + 1 + kAct, kActH1 = 128, kActH2 = 256, kActOut = 21;
constexpr int kStepWords = 21, kUserWords = kZ + kUser;   // 216 words = 54 Philox blocks
constexpr uint32_t kTagStep = 0u, kTagUser = 1u, kTagEps = 2u;

__constant__ int c_group_lo[kGroups + 1] = {0, 8, 16, 27, 38, 49, 60, 62, 64, 67, 85, 88};

__device__ __forceinline__ int group_of(int c) {
    int g = 0;
#pragma unroll
    for (int i = 1; i < kGroups; ++i) g += c >= c_group_lo[i];
    return g;
}

__device__ __forceinline__ uint32_t noise_word(uint64_t seed, uint32_t env, uint32_t ev, uint32_t tag, uint32_t w) {
    return block_word(philox4x32_10(env, ev, w >> 2, tag, (uint32_t)seed, (uint32_t)(seed >> 32)), w & 3u);
}

enum { kActNone = 0, kActLeaky = 1, kActRelu = 2 };

// Y[s][o] = act(b[o] + sum_k X[s][k] W[k][o]) for the ROWS rows of the tile.  Unit = (column o, rows 4g..4g+3).
// ACC = float: an fp32 fma chain (action model, generator: their outputs only feed Gumbel-max draws, checked under a margin).
// ACC = double: the fp32 products summed in fp64 and rounded once per output (user model: its output is the reward, and an fp32
// chain over 118-128 terms that largely cancel is off by up to ~3e-5 absolute -- torch's fp32 CPU result is off by as much).
template <int ACT, typename ACC = float, int ROWS = kTile>
__device__ __forceinline__ void dense_tile(const float* __restrict__ W, const float* __restrict__ b, const float* X, int K,
                                           int O, float* Y) {
    for (int u = threadIdx.x; u < O * (ROWS / 4); u += kThreads) {
        const int o = u % O, g = u / O;
        const float* x = X + 4 * g * kLd;
        ACC a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const ACC w = W[k * O + o];
            a0 = fma((ACC)x[k], w, a0);
            a1 = fma((ACC)x[kLd + k], w, a1);
            a2 = fma((ACC)x[2 * kLd + k], w, a2);
            a3 = fma((ACC)x[3 * kLd + k], w, a3);
        }
        const ACC bias = b ? (ACC)b[o] : (ACC)0;
        float v[4] = {(float)(a0 + bias), (float)(a1 + bias), (float)(a2 + bias), (float)(a3 + bias)};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float y = v[i];
            if (ACT == kActLeaky) y = y > 0.f ? y : 0.01f * y;
            if (ACT == kActRelu) y = fmaxf(y, 0.f);
            Y[(4 * g + i) * kLd + o] = y;
        }
    }
    __syncthreads();
}

// generator + per-group Gumbel-max for the slots with need[s]; writes T.user[s][*] and task_user (and sim_user if given).
// TileT: kRows rows with xa / xb (kLd-strided activations), gum, env, ev, need, user.
template <class TileT>
__device__ void draw_users(TileT& T, const cirs_vtb_weights& w, uint64_t seed, int32_t* task_user, int32_t* sim_user) {
    constexpr int kRows = TileT::kRows;
    for (int i = threadIdx.x; i < kRows * (kUserWords / 4); i += kThreads) {
        const int s = i / (kUserWords / 4), blk = i % (kUserWords / 4);
        const bool on = T.need[s] != 0;
        const u32x4 r = on ? philox4x32_10((uint32_t)T.env[s], T.ev[s], blk, 1u, (uint32_t)seed, (uint32_t)(seed >> 32))
                           : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int wd = 4 * blk + q;
            const uint32_t x = block_word(r, q);
            if (wd < kZ) T.xa[s * kLd + wd] = on ? u01_from_bits(x) : 0.f;
            else T.gum[s][wd - kZ] = on ? gumbel_from_bits(x) : 0.f;
        }
    }
    __syncthreads();
    dense_tile<kActLeaky, float, kRows>(w.gen_w1, w.gen_b1, T.xa, kZ, kGenH, T.xb);
    dense_tile<kActNone, float, kRows>(w.gen_w2, w.gen_b2, T.xb, kGenH, kUser, T.xa);
    for (int i = threadIdx.x; i < kRows * kGroups; i += kThreads) {
        const int s = i / kGroups, g = i % kGroups;
        if (!T.need[s]) continue;
        const int lo = c_group_lo[g], hi = c_group_lo[g + 1];
        int best = lo;
        float bv = T.xa[s * kLd + lo] + T.gum[s][lo];
        for (int c = lo + 1; c < hi; ++c) {
            const float v = T.xa[s * kLd + c] + T.gum[s][c];
            if (v > bv) { bv = v; best = c; }        // ties -> lowest index (torch.argmax)
        }
        T.user[s][g] = best;
        task_user[(long)T.env[s] * kGroups + g] = best;
        if (sim_user) sim_user[(long)T.env[s] * kGroups + g] = best;
    }
    __syncthreads();
}

// the action model on T.xa[s][0..116) = [task user | t | action] and the two Gumbel-max draws with the step Gumbels sg[s][0..21):
// ab[s] = (clicks 0..10, second draw 0..9).  Clobbers xa / xb; ends on a barrier.
template <class TileT>
__device__ __forceinline__ void action_draw(TileT& T, const cirs_vtb_weights& w) {
    constexpr int kRows = TileT::kRows;
    dense_tile<kActLeaky, float, kRows>(w.act_w1, w.act_b1, T.xa, kActIn, kActH1, T.xb);
    dense_tile<kActLeaky, float, kRows>(w.act_w2, w.act_b2, T.xb, kActH1, kActH2, T.xa);
    dense_tile<kActNone, float, kRows>(w.act_w3, w.act_b3, T.xa, kActH2, kActOut, T.xb);
    if (threadIdx.x < 2 * kRows) {
        const int s = threadIdx.x >> 1, which = threadIdx.x & 1;
        const int lo = which ? 11 : 0, hi = which ? kActOut : 11;
        int best = lo;
        float bv = T.xb[s * kLd + lo] + T.sg[s][lo];
        for (int c = lo + 1; c < hi; ++c) {
            const float v = T.xb[s * kLd + c] + T.sg[s][c];
            if (v > bv) { bv = v; best = c; }
        }
        T.ab[s][which] = best - lo;
    }
    __syncthreads();
}

}  // namespace
}  // namespace cirs
