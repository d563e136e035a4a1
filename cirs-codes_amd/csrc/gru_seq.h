// gru_seq.h -- the GRU recurrence over the buffer rows, shared by the two trackers whose encoder is a torch.nn.GRU layer (gru_tracker.hip: every layer of
// its stack; narm_tracker.hip: its one encoder layer): the sizes of a staged cell matrix, what the forward keeps of every row (GruRows), and the two
// sequential kernels of the recompute-based BPTT -- one wavefront per env, forward over p = 0 .. len-1 and backward over p = len-1 .. 0.
#pragma once
#include "slot_tracker.h"

namespace cirs {

constexpr int gG = 3 * tD;                                 // gate rows of a cell matrix
constexpr int kGruLds = tD + 65;                           // LDS stride of one k of a staged [k][96] matrix: 97 (odd: conflict-free both ways)
constexpr int kGruMat = tD * kGruLds;                      // 3104 floats; = 32 mod 64: the two matrices of a layer start half the banks apart

struct GruRows { float *r, *z, *n, *hn, *h, *hp; };      // [R, 32] each: the gates, W_hn h + b_hn, the new and the previous h of every row

// (B) one wavefront per env.  Lane (half, d): half 0 forms row d of W_hr h and the first 16 terms of row d of W_hz h, half 1 row d of W_hn h and the other 16.
static __global__ __launch_bounds__(64) void gru_seq_fwd(const float* __restrict__ Gi, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
                                                  const int32_t* __restrict__ offsets, const int32_t* __restrict__ lens, GruRows a) {
    __shared__ float sW[kGruMat];
    __shared__ float sb[gG];
    __shared__ float sh[tD];
    const int lane = threadIdx.x, d = lane & (tD - 1), half = lane >> 5;
    for (int q = lane; q < gG * tD; q += 64) sW[(q & 31) * kGruLds + (q >> 5)] = w_hh[q];
    for (int q = lane; q < gG; q += 64) sb[q] = b_hh[q];
    __syncthreads();
    const int b = blockIdx.x, len = lens[b], off = offsets[b];
    if (len <= 0) return;
    const int oa = half ? 2 * tD + d : d;
    float h = 0.f;
    float p_r = Gi[(size_t)off * gG + d], p_z = Gi[(size_t)off * gG + tD + d], p_n = Gi[(size_t)off * gG + 2 * tD + d];
    for (int p = 0; p < len; ++p) {
        const size_t row = (size_t)off + p;
        const float gi_r = p_r, gi_z = p_z, gi_n = p_n;
        if (p + 1 < len) { p_r = Gi[(row + 1) * gG + d]; p_z = Gi[(row + 1) * gG + tD + d]; p_n = Gi[(row + 1) * gG + 2 * tD + d]; }
        if (lane < tD) sh[lane] = h;
        __builtin_amdgcn_wave_barrier();
        float acc = sb[oa];
#pragma unroll
        for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(sW[k * kGruLds + oa], sh[k], acc);
        float c = half ? 0.f : sb[tD + d];
#pragma unroll
        for (int k = 0; k < tD / 2; ++k) c = __builtin_fmaf(sW[(k + 16 * half) * kGruLds + tD + d], sh[k + 16 * half], c);
        const float oacc = __shfl_xor(acc, 32, CIRS_WAVE), oc = __shfl_xor(c, 32, CIRS_WAVE);
        const float gh_r = half ? oacc : acc, gh_n = half ? acc : oacc;
        const float gh_z = (half ? oc : c) + (half ? c : oc);
        const float r = cell_sigmoid(gi_r + gh_r), z = cell_sigmoid(gi_z + gh_z);
        const float nn = tanhf(gi_n + r * gh_n);
        const float hnew = (1.0f - z) * nn + z * h;
        __builtin_amdgcn_wave_barrier();
        if (lane < tD) {
            const size_t o = row * tD + d;
            a.r[o] = r; a.z[o] = z; a.n[o] = nn; a.hn[o] = gh_n; a.hp[o] = h; a.h[o] = hnew;
        }
        h = hnew;
    }
}

// (D) one wavefront per env, positions in reverse.  carry[k] = dh[k] z[k] + sum_o dGh[o] W_hh[o][k]: lane (half, k) adds the rows o of its half in ascending order.
static __global__ __launch_bounds__(64) void gru_seq_bwd(const float* __restrict__ dH, GruRows a, const float* __restrict__ w_hh, const int32_t* __restrict__ offsets,
                                                  const int32_t* __restrict__ lens, float* __restrict__ dGi, float* __restrict__ dGh) {
    __shared__ float sW[gG * tD];
    __shared__ float sg[gG];
    const int lane = threadIdx.x, d = lane & (tD - 1), half = lane >> 5;
    for (int q = lane; q < gG * tD; q += 64) sW[q] = w_hh[q];
    __syncthreads();
    const int b = blockIdx.x, len = lens[b], off = offsets[b];
    float carry = 0.f;
    for (int p = len - 1; p >= 0; --p) {
        const size_t row = (size_t)off + p, o = row * tD + d;
        const float r = a.r[o], z = a.z[o], nn = a.n[o], hn = a.hn[o], hp = a.hp[o];
        const float dh = dH[o] + carry;
        const float dan = dh * (1.0f - z) * (1.0f - nn * nn);
        const float daz = dh * (hp - nn) * z * (1.0f - z);
        const float dar = dan * hn * r * (1.0f - r);
        const float ghn = dan * r;
        if (lane < tD) {
            dGi[row * gG + d] = dar; dGi[row * gG + tD + d] = daz; dGi[row * gG + 2 * tD + d] = dan;
            dGh[row * gG + d] = dar; dGh[row * gG + tD + d] = daz; dGh[row * gG + 2 * tD + d] = ghn;
            sg[d] = dar; sg[tD + d] = daz; sg[2 * tD + d] = ghn;
        }
        __builtin_amdgcn_wave_barrier();
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < gG / 2; ++q) {
            const int oo = q + (gG / 2) * half;
            acc = __builtin_fmaf(sg[oo], sW[oo * tD + d], acc);
        }
        const float other = __shfl_xor(acc, 32, CIRS_WAVE);
        carry = dh * z + ((half ? other : acc) + (half ? acc : other));
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace cirs
