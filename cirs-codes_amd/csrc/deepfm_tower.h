// deepfm_tower.h -- the front half of an optimiser step that the Kuaishou trainers share (deepfm_train.hip: one tower over six fields;
// dice_train.hip: a main tower over eight fields and a ui tower over two).  A tower is the FM cross term over the embedding values of x
// plus two 64-wide ReLU layers, a 64 -> 1 layer and an output bias; one wavefront runs it on one row, activations in LDS.
//   TowerNet / TowerRows   a tower's offsets in the flat parameter buffer / its per-row GEMM operands in the workspace
//   tower_forward          cross term and DNN output of one row, as two values: each model adds them to its linear part in its own order
//   tower_backward         the row's GEMM operands and d loss / d x (DNN input gradient + FM)
//   write_feat_contrib     the four feature contribution rows + keys of one row (padding_idx = 0)
//   step_row               sample i of a step -> its row of the resident data set
//   loss_means4            fixed-order means of the four per-sample loss terms
//   launch_tower_dw        the three weight-gradient GEMMs of one tower
// What follows the row kernel (scatter, regulariser + Adam) and the workspace allocator are in table_step.h.
#pragma once
#include "small_gemm.h"
#include "table_step.h"

namespace cirs {

constexpr int kTowerH = 64;

struct TowerNet { long w1, b1, w2, b2, last, out; };   // [64, K] [64] [64, 64] [64] [64] [1]
__host__ __device__ inline TowerNet tower_net(long& o, long K) {   // the tower's slots from offset o on; o moves past them
    TowerNet N;
    N.w1 = o; o += kTowerH * K; N.b1 = o; o += kTowerH; N.w2 = o; o += kTowerH * kTowerH; N.b2 = o; o += kTowerH;
    N.last = o; o += kTowerH; N.out = o; o += 1;
    return N;
}

struct TowerRows { float *X, *H1, *H2, *DA1, *DA2, *DY; };   // R rows: [R,K] [R,64] [R,64] [R,64] [R,64] [R]
inline TowerRows tower_rows(Bump& w, size_t R, int K) {
    TowerRows o;
    o.X = w.take(R * K); o.H1 = w.take(R * kTowerH); o.H2 = w.take(R * kTowerH); o.DA1 = w.take(R * kTowerH); o.DA2 = w.take(R * kTowerH);
    o.DY = w.take(R);
    return o;
}

struct TowerOut { float cross, dnn; };   // sum_e (S_e^2 - Q_e) (the FM term is half of it); last . relu(a2) + out bias

// one tower by one wavefront over x [K] (NF * E embedding values, then the dense ones); S / a1 / a2 stay in LDS for the backward
__device__ __forceinline__ TowerOut tower_forward(const float* __restrict__ P, const TowerNet& N, int NF, int E, int K, int lane, const float* x,
                                                  float* S, float* a1, float* a2) {
    float cross = 0.f;
    for (int e = lane; e < E; e += CIRS_WAVE) {
        float s = 0.f, q = 0.f;
        for (int fl = 0; fl < NF; ++fl) { const float v = x[fl * E + e]; s += v; q += v * v; }
        S[e] = s;
        cross += s * s - q;
    }
    cross = wave_sum_f32(cross);
    float acc = P[N.b1 + lane];
    const float* w1r = P + N.w1 + (size_t)lane * K;
    for (int k = 0; k < K; ++k) acc = __builtin_fmaf(w1r[k], x[k], acc);
    a1[lane] = acc;
    __builtin_amdgcn_wave_barrier();
    acc = P[N.b2 + lane];
    const float* w2r = P + N.w2 + (size_t)lane * kTowerH;
    for (int k = 0; k < kTowerH; ++k) acc = __builtin_fmaf(w2r[k], fmaxf(a1[k], 0.f), acc);
    a2[lane] = acc;
    const float dnn = wave_sum_f32(P[N.last + lane] * fmaxf(acc, 0.f));
    __builtin_amdgcn_wave_barrier();
    return {cross, dnn + P[N.out]};
}

// backward of one tower row r given dy: writes the row's GEMM operands; dxs[k], k < NF * E = d loss / d x[k] (DNN input gradient + FM)
__device__ __forceinline__ void tower_backward(const float* __restrict__ P, const TowerNet& N, int NF, int E, int K, float dy, int lane, size_t r,
                                               const float* x, const float* S, const float* a1, const float* a2, float* t64, float* dxs,
                                               const TowerRows& o) {
    // da2 = dy * last * relu'(a2); dh1 = W2^T da2; da1 = dh1 * relu'(a1); dx = W1^T da1
    const float da2 = a2[lane] > 0.f ? dy * P[N.last + lane] : 0.f;
    o.DA2[r * kTowerH + lane] = da2;
    o.H2[r * kTowerH + lane] = fmaxf(a2[lane], 0.f);
    o.H1[r * kTowerH + lane] = fmaxf(a1[lane], 0.f);
    t64[lane] = da2;
    __builtin_amdgcn_wave_barrier();
    float dh1 = 0.f;
    for (int q = 0; q < kTowerH; ++q) dh1 = __builtin_fmaf(P[N.w2 + (size_t)q * kTowerH + lane], t64[q], dh1);
    const float da1 = a1[lane] > 0.f ? dh1 : 0.f;
    o.DA1[r * kTowerH + lane] = da1;
    __builtin_amdgcn_wave_barrier();
    t64[lane] = da1;
    __builtin_amdgcn_wave_barrier();
    for (int k = lane; k < K; k += CIRS_WAVE) {
        o.X[r * K + k] = x[k];
        if (k < NF * E) {
            float dx = 0.f;
            for (int q = 0; q < kTowerH; ++q) dx = __builtin_fmaf(P[N.w1 + (size_t)q * K + k], t64[q], dx);
            // FM: d/dv_f,e of 0.5 * sum_e (S_e^2 - Q_e) = S_e - v_f,e
            dxs[k] = __builtin_fmaf(dy, S[k % E] - x[k], dx);
        }
    }
    if (lane == 0) o.DY[r] = dy;
    __builtin_amdgcn_wave_barrier();
}

// the feature contribution rows [d embedding row | d linear weight] and keys of tower row `slot`, whose features f4 are the fields
// field0 .. field0 + 3 of dxs.  padding_idx = 0: the embedding row gets no gradient, the 1-d weight does
__device__ __forceinline__ void write_feat_contrib(float* __restrict__ CF, int32_t* __restrict__ KF, size_t slot, int E, const int32_t* f4,
                                                   const float* dxs, int field0, float dy, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int fid = f4[q];
        for (int e = lane; e < E + 1; e += CIRS_WAVE)
            CF[(slot * 4 + q) * (E + 1) + e] = e < E ? (fid == 0 ? 0.f : dxs[(field0 + q) * E + e]) : dy;
        if (lane == 0) KF[slot * 4 + q] = fid;
    }
}

// sample i of a step reads row order[r0 + i] of the data set (r0 + i when order is null).  An index outside the data set is not read
// there: the sample takes row 0 and `bad` tells the row kernel to make the step's loss NaN
__device__ __forceinline__ long step_row(const int64_t* __restrict__ order, long r0, int i, long n_rows, bool& bad) {
    const long row = order ? (long)order[r0 + i] : r0 + i;
    bad = row < 0 || row >= n_rows;
    return bad ? 0 : row;
}

// means over the n samples of the four per-sample loss terms LP [n,4] by one workgroup of 256: fixed-order sums; m valid in thread 0
__device__ __forceinline__ void loss_means4(const float* __restrict__ LP, int n, float* m) {
    // (four sums share the nine barriers of one tree in block_sum's order: as four block_sum calls the DICE epoch took 1531 us per step against 1524 us, profiles/r09_optim_refactor_ab.md)
    __shared__ float sh[4][256];
    const int tid = threadIdx.x;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < n; i += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += LP[(size_t)i * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) sh[q][tid] = a[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int q = 0; q < 4; ++q) sh[q][tid] += sh[q][tid + s];
        __syncthreads();
    }
    const float inv = 1.0f / (float)n;
#pragma unroll
    for (int q = 0; q < 4; ++q) m[q] = sh[q][0] * inv;
}

// dense layers of one tower: dW = dY^T X over its R rows.  `partial` >= tower_partial_floats(R, K): the slab partials of the largest
// of the three problems, [64, K] or [64, 64]
inline size_t tower_partial_floats(long R, int K) { return dwg_partial_floats(R, kTowerH, K > kTowerH ? K : kTowerH); }
inline void launch_tower_dw(const TowerRows& o, int R, int K, float* grads, const TowerNet& N, bool with_out_bias, float* partial, hipStream_t s) {
    launch_dw_gemm(o.DA1, kTowerH, o.X, K, R, kTowerH, K, grads + N.w1, grads + N.b1, partial, s);
    launch_dw_gemm(o.DA2, kTowerH, o.H1, kTowerH, R, kTowerH, kTowerH, grads + N.w2, grads + N.b2, partial, s);
    launch_dw_gemm(o.DY, 1, o.H2, kTowerH, R, 1, kTowerH, grads + N.last, with_out_bias ? grads + N.out : nullptr, partial, s);
}

}  // namespace cirs
