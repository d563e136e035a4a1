// fmlp_tracker.hip -- StateTrackerFMLP for gfx950: a learnable frequency-domain filter and a LayerNorm / GELU feed-forward block over the window of the last
// item slots (FMLP-Rec, Zhou et al., WWW 2022).
//
// The reference has no counterpart; the model is defined here, in include/cirs_hip.h and in DESIGN.md 7.10:
//   inputs    the other trackers' slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k -- no sqrt(D) scale, no positional encoding
//   tile      Y^{-1}[i] = x_{p-W+1+i} if p-W+1+i >= 1 else 0, i = 0 .. W-1 (row W-1 = the newest item; zero rows at the input of layer 0 ONLY)
//   layer l   h_l = irfft(complex_weight_l, n = W);  F[i,d] = sum_{m<W} h_l[(i-m) mod W, d] Y^{l-1}[m,d];  A = LayerNorm(Y^{l-1} + F);
//             M = dense_2(gelu(dense_1(A))) (32 -> 128 -> 32, erf GELU);  Y^l = LayerNorm(A + M)
//   state     h_p = x_0 + Y^{L-1}[W-1] (p >= 1), h_0 = x_0;  s_p = decoder(h_p)
// The parameters live in the frequency domain, the kernels work in the time domain: every workgroup forms the taps h_l [W][32] from complex_weight while it
// stages the weights, the phase index k n reduced modulo W as an integer before cospif / sinpif see it (h_l at float32 rounding for every W).
// The tile has 16 rows; rows W .. 15 are don't-cares: they are loaded as zero rows, every product carries them along (a row of an MFMA product depends on
// its own row only), and no filter sum ever reads them (m < W).
// Step (one launch appends one position for n envs): ONE env per wavefront, four per workgroup.  A workgroup stages both layers' dense_1 ([out][36]) and
// dense_2 ([out][132]) as the MFMA's B operands, the taps, the decoder [k][33] and the slot's matrix [d][33] in LDS once, a wavefront its tile [16][36] and
// its hidden tile [16][132].  The filter is plain FMAs (8 W per lane and layer).  dense_1 is a [16] x [32 -> 128] product on v_mfma_f32_16x16x4_f32 in eight
// independent accumulator chains, dense_2 a [16] x [128 -> 32] product in two; the biases start in the accumulators.  Both layers are computed on the whole
// tile (of the last layer only row W-1 is read: the two mat-vecs instead of the dense tile are not built).  Everything per env is predicated, not branched.
//
// Backward (rows = (env b, position p < len_b), env-major; no sequential pass):
//   F  fmlp_rows_fwd: the forward of every row again from the stored slots (the step kernel's device functions) -> per layer the input tile (YIN), both
//      LayerNorms' normalised values and inverse deviations (XH1, RSTD1, XH2, RSTD2), A and the hidden pre-activations (U); h
//   C  G = gather(dstate); dH = G W_dec and the decoder's weight gradient in one launch (rows_gemm + dw_gemm, as the other trackers' stage C)
//   B  fmlp_rows_bwd, one row per wavefront, top layer down, dY^{top} = dH at row W-1: LayerNorm backward (DN2 -> DM); dU = (DM W2) gelu'(U) -- the
//      forward's 32 -> 128 product on W2 staged transposed; dA = DM + DU W1 -- the 128 -> 32 product on W1 staged transposed; LayerNorm backward
//      (DN1 -> dPre); the filter's two correlations: dY^{l-1}[m] = dPre[m] + sum_i h[(i-m) mod W] dPre[i] and the row's share of the tap gradient
//      DHP[n] = sum_i dPre[i] Y^{l-1}[(i-n) mod W].  U is overwritten by gelu(U): the operand of dense_2's weight gradient.  Ends in DWIN [R, 16, 32]
//   W  weight gradients through the slab partials: per layer dense_2 = DM^T gelu(U), dense_1 = DU^T A, the two LayerNorms in the diag form, over the
//      R 16 (row, tile row) pairs; the tap gradient dh_l = the column sums of DHP over the R rows (a problem over a column of ones)
//   X  fmlp_window_bwd: dX[b,0] = sum_p dH[b,p];  dX[b,k] = sum_{p=k}^{min(len_b-1, k+W-1)} DWIN_p[W-1-(p-k)]  -- p ascending, every row on its own
//   E  the slot stage of the recurrent trackers (slot_tracker.h), whose last launch sums every slab partial of the pass
//   T  fmlp_filter_grad: dh_l -> d complex_weight_l by the closed form of d irfft, the exact zeros written
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include "slot_tracker.h"

namespace cirs {

constexpr int fTile = CIRS_FMLP_MAX_WINDOW;                // 16 rows of a tile: row i = slot p - W + 1 + i
constexpr int fMaxL = CIRS_FMLP_MAX_LAYERS;                // 2
constexpr int fHid = CIRS_FMLP_HIDDEN;                     // 128
constexpr int fXLd = tD + 4;                               // LDS stride of a row of 32: 36 (16-byte aligned rows, row starts spread over the banks)
constexpr int fULd = fHid + 4;                             // LDS stride of a row of 128: 132
constexpr int fUpFloats = fHid * fXLd;                     // a staged [128][36] operand (32 -> 128): 4608 floats
constexpr int fDownFloats = tD * fULd;                     // a staged [32][132] operand (128 -> 32): 4224 floats
constexpr int fCwFloats = (fTile / 2 + 1) * tD * 2;        // a staged complex_weight at W = 16: 576 floats
constexpr int fLds = tD + 1;                              // LDS stride of a staged 32-row matrix, as in avg_tracker.hip
constexpr int fEnvsPerWg = 4;                              // one env (or buffer row) per wavefront
constexpr int fWgPerCu = 1;                                // 131 328 bytes of LDS per workgroup of the step kernel: one fits in a CU's 160 KB
constexpr float fEps = 1e-5f;

// both layers' dense weights, once per workgroup, coalesced dword reads (the tensors are views of one flat buffer: no alignment beyond a float's).
// Forward: sUp[l] = dense_1 [out 128][36], sDown[l] = dense_2 [out 32][132].  kT (the backward's transposed products): sUp[l] = dense_2^T [hidden 128][36],
// sDown[l] = dense_1^T [in 32][132].  sCw[l] = complex_weight_l, flat.  Fixed trip counts, predicated on the layer count: a thread's 70 loads are all
// issued before its first LDS store, one round trip to the L2 instead of one per layer.
template <bool kT>
__device__ __forceinline__ void fmlp_stage(const cirs_fmlp_cfg& cfg, const cirs_fmlp_weights& w, float* sUp, float* sDown, float* sCw) {
    float v1[fMaxL][16], v2[fMaxL][16], vc[fMaxL][3];
    const int ncw = (cfg.window / 2 + 1) * tD * 2;         // <= fCwFloats = 576 <= 3 x 256
#pragma unroll
    for (int lay = 0; lay < fMaxL; ++lay) {
        const bool on = lay < cfg.nlayers;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            v1[lay][u] = on ? w.d1_w[lay][threadIdx.x + 256 * u] : 0.f;
            v2[lay][u] = on ? w.d2_w[lay][threadIdx.x + 256 * u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) vc[lay][u] = (on && (int)threadIdx.x + 256 * u < ncw) ? w.cw[lay][threadIdx.x + 256 * u] : 0.f;
    }
#pragma unroll
    for (int lay = 0; lay < fMaxL; ++lay) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int q = threadIdx.x + 256 * u;
            const int j = q >> 5, c = q & 31;          // dense_1 [j][c]
            const int o = q >> 7, k = q & 127;         // dense_2 [o][k]
            if (kT) {
                sUp[lay * fUpFloats + k * fXLd + o] = v2[lay][u];
                sDown[lay * fDownFloats + c * fULd + j] = v1[lay][u];
            } else {
                sUp[lay * fUpFloats + j * fXLd + c] = v1[lay][u];
                sDown[lay * fDownFloats + o * fULd + k] = v2[lay][u];
            }
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if ((int)threadIdx.x + 256 * u < fCwFloats) sCw[lay * fCwFloats + threadIdx.x + 256 * u] = vc[lay][u];
    }
}

// the time-domain taps of both layers from the staged complex_weight (a workgroup barrier after fmlp_stage, one after this):
// sTap[l][n][d] = irfft(complex_weight_l, n = W)[n, d]
//   = (1 / W) sum_{k <= W/2} c_k (re_k cos(2 pi (k n mod W) / W) - im_k sin(2 pi (k n mod W) / W)),  c_k = 1 for k = 0 and (W even) k = W/2, else 2.
// The imaginary parts of those two bins are not read.  k ascending; rows n >= W are zero.
__device__ __forceinline__ void fmlp_taps(const cirs_fmlp_cfg& cfg, const float* sCw, float* sTap) {
    const int W = cfg.window;
    for (int idx = threadIdx.x; idx < fMaxL * fTile * tD; idx += 256) {
        const int lay = idx >> 9, n = (idx >> 5) & (fTile - 1), d = idx & (tD - 1);
        float acc = 0.f;
        if (lay < cfg.nlayers && n < W) {
            const float* cw = sCw + lay * fCwFloats;
            for (int k = 0; 2 * k <= W; ++k) {
                const bool real_bin = k == 0 || 2 * k == W;
                const float re = cw[(k * tD + d) * 2], im = real_bin ? 0.f : cw[(k * tD + d) * 2 + 1];
                const float x = (float)(2 * ((k * n) % W)) / (float)W;      // the phase in units of pi, reduced as an integer
                const float term = __builtin_fmaf(re, cospif(x), -(im * sinpif(x)));
                acc += real_bin ? term : 2.0f * term;
            }
            acc = acc / (float)W;
        }
        sTap[idx] = acc;
    }
}

// acc[c][r] += sum_{k<32} tile[4 q + r][k] * sW[16 c + l][k] for the 16 rows and the 128 columns, on v_mfma_f32_16x16x4_f32: lane (l = lane & 15,
// q = lane >> 4) supplies row l of A and column 16 c + l of B for each of the eight output tiles c; of a block of 16 contraction indices it holds
// 4 q .. 4 q + 3 (one ds_read_b128 each), MFMA i of the block contracts {i, 4 + i, 8 + i, 12 + i}: a fixed order.  Eight independent chains.
__device__ __forceinline__ void fmlp_up(const float* tile, const float* sW, int l, int q, f32x4 (&acc)[8]) {
    const float* ar = tile + l * fXLd + 4 * q;
    const float* wr = sW + l * fXLd + 4 * q;
#pragma unroll
    for (int kk = 0; kk < tD; kk += 16) {
        const float4 a = *reinterpret_cast<const float4*>(ar + kk);
        float4 b[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) b[c] = *reinterpret_cast<const float4*>(wr + c * 16 * fXLd + kk);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[c].x, acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[c].y, acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[c].z, acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[c].w, acc[c], 0, 0, 0);
    }
}

// acc0[r] / acc1[r] += sum_{k<128} ut[4 q + r][k] * sW[l | 16 + l][k]: the same lane roles over a contraction of 128, two independent chains
__device__ __forceinline__ void fmlp_down(const float* ut, const float* sW, int l, int q, f32x4& acc0, f32x4& acc1) {
    const float* ar = ut + l * fULd + 4 * q;
    const float* w0 = sW + l * fULd + 4 * q;
    const float* w1 = w0 + 16 * fULd;
#pragma unroll
    for (int kk = 0; kk < fHid; kk += 16) {
        const float4 a = *reinterpret_cast<const float4*>(ar + kk);
        const float4 b0 = *reinterpret_cast<const float4*>(w0 + kk);
        const float4 b1 = *reinterpret_cast<const float4*>(w1 + kk);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1.w, acc1, 0, 0, 0);
    }
}

// the sum over the 32 channels of a tile row: the lane's two tiles, then the 16 lanes of its quarter (xor 1, 2, 4, 8): the same order in every lane
__device__ __forceinline__ float fmlp_row_sum(float a, float b) {
    float s = a + b;
#pragma unroll
    for (int sft = 1; sft <= 8; sft <<= 1) s += __shfl_xor(s, sft, CIRS_WAVE);
    return s;
}

// LayerNorm of a tile row in the accumulator layout: the normalised pair and the inverse deviation
__device__ __forceinline__ void fmlp_ln(float x0, float x1, float& h0, float& h1, float& rstd) {
    const float mean = fmlp_row_sum(x0, x1) * (1.0f / tD);
    const float c0 = x0 - mean, c1 = x1 - mean;
    const float var = fmlp_row_sum(c0 * c0, c1 * c1) * (1.0f / tD);
    rstd = 1.0f / sqrtf(var + fEps);
    h0 = c0 * rstd; h1 = c1 * rstd;
}

// ... and its backward: d0 / d1 = the gradient at the output, g = the weight, h = the normalised values -> the gradient at the input
__device__ __forceinline__ void fmlp_ln_bwd(float d0, float d1, float h0, float h1, float g0, float g1, float rstd, float& o0, float& o1) {
    const float a0 = d0 * g0, a1 = d1 * g1;
    const float m1 = fmlp_row_sum(a0, a1) * (1.0f / tD), m2 = fmlp_row_sum(a0 * h0, a1 * h1) * (1.0f / tD);
    o0 = rstd * (a0 - m1 - h0 * m2); o1 = rstd * (a1 - m1 - h1 * m2);
}

// what the backward keeps of a row's forward, per layer: YIN, XH1, A, XH2 [L][R 16 32], RSTD1, RSTD2 [L][R 16], U [L][R 16 128]
struct FmlpKeep { float *YIN, *XH1, *A, *XH2, *RSTD1, *RSTD2, *U; };

// the layers over a wavefront's tile [16][36] (rows >= W zero on entry), in place; ut: the wavefront's hidden tile [16][132].  Values live in the layout of
// the MFMA's accumulators: lane (l, q) holds rows 4 q .. 4 q + 3 of columns l and 16 + l.  kKeep: the backward's copy of row r (of R).
template <bool kKeep>
__device__ __forceinline__ void fmlp_layers(const cirs_fmlp_cfg& cfg, const cirs_fmlp_weights& w, const float* sUp, const float* sDown, const float* sTap,
                                            float* tile, float* ut, int lane, const FmlpKeep& keep, long r, long R, bool live) {
    const int l = lane & 15, q = lane >> 4, W = cfg.window;
    for (int lay = 0; lay < cfg.nlayers; ++lay) {
        const float* tap = sTap + lay * fTile * tD;
        const size_t rows16 = ((size_t)lay * R + r) * fTile;
        // ---- the filter (m ascending; a don't-care row i >= W takes row 0's taps and is dropped), the residual, LayerNorm -> A, in place
        //      (the m loop runs to W; a build with the fixed trip count of 16 predicated on m < W was slower: DESIGN.md 7.10) ----
        float a0[4], a1[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = 4 * q + rr;
            const bool valid = i < W;
            const int iv = valid ? i : 0;
            float f0 = 0.f, f1 = 0.f;
            for (int m = 0; m < W; ++m) {
                int n = iv - m;
                n += n < 0 ? W : 0;
                f0 = __builtin_fmaf(tap[n * tD + l], tile[m * fXLd + l], f0);
                f1 = __builtin_fmaf(tap[n * tD + 16 + l], tile[m * fXLd + 16 + l], f1);
            }
            const float y0 = tile[i * fXLd + l], y1 = tile[i * fXLd + 16 + l];
            a0[rr] = y0 + (valid ? f0 : 0.f); a1[rr] = y1 + (valid ? f1 : 0.f);
            if (kKeep && live) { keep.YIN[(rows16 + i) * tD + l] = y0; keep.YIN[(rows16 + i) * tD + 16 + l] = y1; }
        }
        __builtin_amdgcn_wave_barrier();
        {
            const float g0 = w.fln_w[lay][l], g1 = w.fln_w[lay][16 + l], e0 = w.fln_b[lay][l], e1 = w.fln_b[lay][16 + l];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = 4 * q + rr;
                float h0, h1, rstd;
                fmlp_ln(a0[rr], a1[rr], h0, h1, rstd);
                a0[rr] = __builtin_fmaf(h0, g0, e0); a1[rr] = __builtin_fmaf(h1, g1, e1);
                tile[i * fXLd + l] = a0[rr]; tile[i * fXLd + 16 + l] = a1[rr];
                if (kKeep && live) {
                    keep.XH1[(rows16 + i) * tD + l] = h0; keep.XH1[(rows16 + i) * tD + 16 + l] = h1;
                    keep.A[(rows16 + i) * tD + l] = a0[rr]; keep.A[(rows16 + i) * tD + 16 + l] = a1[rr];
                    if (l == 0) keep.RSTD1[rows16 + i] = rstd;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- dense_1 and the exact GELU -> the hidden tile ----
        {
            f32x4 acc[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) { const float b = w.d1_b[lay][16 * c + l]; acc[c] = f32x4{b, b, b, b}; }
            fmlp_up(tile, sUp + lay * fUpFloats, l, q, acc);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int i = 4 * q + rr;
                    const float u = acc[c][rr];
                    ut[i * fULd + 16 * c + l] = 0.5f * u * (1.0f + erff(u * 0.70710678118654752f));
                    if (kKeep && live) keep.U[(rows16 + i) * fHid + 16 * c + l] = u;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- dense_2, the residual, LayerNorm -> Y^l, in place ----
        {
            const float b0 = w.d2_b[lay][l], b1 = w.d2_b[lay][16 + l];
            f32x4 acc0 = f32x4{b0, b0, b0, b0}, acc1 = f32x4{b1, b1, b1, b1};
            fmlp_down(ut, sDown + lay * fDownFloats, l, q, acc0, acc1);
            const float g0 = w.ln_w[lay][l], g1 = w.ln_w[lay][16 + l], e0 = w.ln_b[lay][l], e1 = w.ln_b[lay][16 + l];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = 4 * q + rr;
                float h0, h1, rstd;
                fmlp_ln(a0[rr] + acc0[rr], a1[rr] + acc1[rr], h0, h1, rstd);
                tile[i * fXLd + l] = __builtin_fmaf(h0, g0, e0); tile[i * fXLd + 16 + l] = __builtin_fmaf(h1, g1, e1);
                if (kKeep && live) {
                    keep.XH2[(rows16 + i) * tD + l] = h0; keep.XH2[(rows16 + i) * tD + 16 + l] = h1;
                    if (l == 0) keep.RSTD2[rows16 + i] = rstd;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(256) void fmlp_step_kernel(cirs_fmlp_cfg cfg, cirs_fmlp_weights w, cirs_fmlp_state st, const int32_t* __restrict__ users,
                                                        const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                        const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                        float* __restrict__ state_out, long state_stride, int walks) {
    __shared__ __attribute__((aligned(16))) float sUp[fMaxL * fUpFloats];
    __shared__ __attribute__((aligned(16))) float sDown[fMaxL * fDownFloats];
    __shared__ float sTap[fMaxL * fTile * tD];
    __shared__ __attribute__((aligned(16))) float sY[fEnvsPerWg * fTile * fXLd];
    __shared__ __attribute__((aligned(16))) float sU[fEnvsPerWg * fTile * fULd];
    __shared__ float sDec[tD * fLds];                      // [k][s]: decoder, transposed
    __shared__ float sIn[tD * fLds];                       // [d][c]: fnn_gate [32][33] (step) or ffn_user [32][32] (init), row-major
    __shared__ float sVec[fEnvsPerWg * tD];                // per wave: the slot's input vector, then h
    __shared__ float sCw[fMaxL * fCwFloats];               // both layers' complex_weight: what the taps are formed from
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state, W = cfg.window;
    const bool is_init = users != nullptr;
    for (int q = threadIdx.x; q < S * tD; q += 256) sDec[(q & 31) * fLds + (q >> 5)] = w.dec_w[q];
    if (is_init) {                                         // position 0 is h_0 = x_0: no layer, nothing of them staged
        for (int q = threadIdx.x; q < tD * tD; q += 256) sIn[(q >> 5) * fLds + (q & 31)] = w.ffn_user_w[q];
    } else {
        for (int q = threadIdx.x; q < tD * (tD + 1); q += 256) sIn[q] = w.gate_w[q];
        fmlp_stage<false>(cfg, w, sUp, sDown, sCw);
        __syncthreads();
        fmlp_taps(cfg, sCw, sTap);
    }
    __syncthreads();
    const FmlpKeep none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float* vin = sVec + wv * tD;
    float* tile = sY + wv * fTile * fXLd;
    float* ut = sU + wv * fTile * fULd;
    const float* mrow = sIn + d * fLds;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long j = ((long)blockIdx.x * walks + it_w) * fEnvsPerWg + wv;
        // ---- which rows are live: every refusal leaves the env and its row of state_out untouched ----
        bool ok = j < n;
        const long jj = ok ? j : 0;
        const int e = env_ids ? env_ids[jj] : (int)jj;
        ok = ok && e >= 0 && e < B;
        if (skip) ok = ok && !skip[jj];
        int pos = 0, u = 0;
        long it = 0;
        if (is_init) {
            u = users[jj];
            ok = ok && u >= 0 && u < cfg.n_users;
        } else {
            it = items[jj];
            ok = ok && it >= 0 && it < cfg.n_items;         // act = -1: the env finished earlier in this rollout
            pos = ok ? st.len[e] : 0;
            ok = ok && pos >= 1 && pos < L;                 // never initialised / history full
            if (!ok) pos = 0;
        }
        const size_t hist = (size_t)(ok ? e : 0) * L * tD;
        // ---- 1. the stored rows of the tile (the W - 1 item slots before the new one; a row before the first item or beyond the window is the zero
        //         row and forms no address): all requested at once, ahead of the slot's arithmetic ----
        const float* xh = st.x_hist + hist + d;
        float wl[fTile / 2];
#pragma unroll
        for (int q = 0; q < fTile / 2; ++q) {
            const int t = 2 * q + half, k = pos - W + 1 + t;
            wl[q] = (t < W - 1 && k >= 1) ? xh[(size_t)k * tD] : 0.f;      // k < pos: t <= W - 2
        }
        // ---- 2. the new input slot (both halves of the wavefront hold it); it is row W - 1 of the tile (pos >= 1) ----
        float x;
        if (is_init) {
            vin[d] = ok ? w.emb_user[(size_t)u * tD + d] : 0.f;
            __builtin_amdgcn_wave_barrier();
            float acc = w.ffn_user_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mrow[k], vin[k], acc);
            x = acc;
        } else {
            const float r = ok ? (float)rew[jj] : 0.f;
            const float a = ok ? w.emb_item[(size_t)it * tD + d] : 0.f;
            vin[d] = a;
            __builtin_amdgcn_wave_barrier();
            float acc = __builtin_fmaf(mrow[0], r, w.gate_b[d]);      // input order [r, a_0..a_31]
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mrow[1 + k], vin[k], acc);
            x = cell_sigmoid(acc) * a;
        }
#pragma unroll
        for (int q = 0; q < fTile / 2; ++q) {
            const int t = 2 * q + half;
            tile[t * fXLd + d] = (pos >= 1 && t == W - 1) ? x : wl[q];
        }
        const float x0 = is_init ? x : (ok ? xh[0] : 0.f);
        if (ok && half == 0) st.x_hist[hist + (size_t)pos * tD + d] = x;
        __builtin_amdgcn_wave_barrier();
        // ---- 3. the layers; h = x_0 + row W - 1 of the top layer; h_0 = x_0 ----
        float h = x0;
        if (!is_init) {
            fmlp_layers<false>(cfg, w, sUp, sDown, sTap, tile, ut, lane, none, 0, 0, false);
            h += tile[(W - 1) * fXLd + d];
        }
        __builtin_amdgcn_wave_barrier();
        vin[d] = h;
        __builtin_amdgcn_wave_barrier();
        // ---- 4. decoder ----
        if (d < S && half == 0) {
            float acc = w.dec_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(sDec[k * fLds + d], vin[k], acc);
            if (ok) state_out[(size_t)j * state_stride + d] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (ok && lane == 0) st.len[e] = pos + 1;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// (F) the forward of every buffer row again, one row per wavefront.  A row at position 0 keeps the values of the zero tile: the backward multiplies them by
// a zero gradient.  ONES [R]: the column of ones of the tap gradient's problem.
__global__ __launch_bounds__(256) void fmlp_rows_fwd(cirs_fmlp_cfg cfg, cirs_fmlp_weights w, const float* __restrict__ x_hist,
                                                     const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t, int R, int walks,
                                                     float* __restrict__ H, float* __restrict__ ONES, FmlpKeep keep) {
    __shared__ __attribute__((aligned(16))) float sUp[fMaxL * fUpFloats];
    __shared__ __attribute__((aligned(16))) float sDown[fMaxL * fDownFloats];
    __shared__ float sTap[fMaxL * fTile * tD];
    __shared__ __attribute__((aligned(16))) float sY[fEnvsPerWg * fTile * fXLd];
    __shared__ __attribute__((aligned(16))) float sU[fEnvsPerWg * fTile * fULd];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    __shared__ float sCw[fMaxL * fCwFloats];
    const int L = cfg.max_len, W = cfg.window;
    fmlp_stage<false>(cfg, w, sUp, sDown, sCw);
    __syncthreads();
    fmlp_taps(cfg, sCw, sTap);
    __syncthreads();
    float* tile = sY + wv * fTile * fXLd;
    float* ut = sU + wv * fTile * fULd;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long r = ((long)blockIdx.x * walks + it_w) * fEnvsPerWg + wv;
        const bool live = r < R;
        const long rr = live ? r : 0;
        const int p = row_t[rr];
        const float* xh = x_hist + (size_t)row_env[rr] * L * tD + d;
        float wl[fTile / 2];
#pragma unroll
        for (int q = 0; q < fTile / 2; ++q) {      // all requested at once
            const int t = 2 * q + half, k = p - W + 1 + t;
            wl[q] = (t < W && k >= 1) ? xh[(size_t)k * tD] : 0.f;      // k <= p: t <= W - 1
        }
#pragma unroll
        for (int q = 0; q < fTile / 2; ++q) tile[(2 * q + half) * fXLd + d] = wl[q];
        __builtin_amdgcn_wave_barrier();
        fmlp_layers<true>(cfg, w, sUp, sDown, sTap, tile, ut, lane, keep, rr, R, live);
        if (live && half == 0) H[(size_t)r * tD + d] = xh[0] + (p >= 1 ? tile[(W - 1) * fXLd + d] : 0.f);
        if (live && lane == 0) ONES[r] = 1.0f;
        __builtin_amdgcn_wave_barrier();
    }
}

// (B) one row per wavefront, top layer down, in the layout of the forward's accumulators.  Every gradient of a tile row >= W is an exact zero: the upstream
// one is, LayerNorm's backward and the transposed products keep a zero row zero, and the filter's correlations are confined to rows < W.
struct FmlpBwdOut { float *DN2, *DM, *DU, *DN1, *DHP, *DWIN; };      // per layer [L][R 16 32] (DU: [L][R 16 128]); DWIN [R 16 32]
__global__ __launch_bounds__(256) void fmlp_rows_bwd(cirs_fmlp_cfg cfg, cirs_fmlp_weights w, int R, int walks, const int32_t* __restrict__ row_t,
                                                     const float* __restrict__ dH, FmlpKeep keep, FmlpBwdOut out) {
    __shared__ __attribute__((aligned(16))) float sUp[fMaxL * fUpFloats];        // dense_2 transposed: [hidden][36]
    __shared__ __attribute__((aligned(16))) float sDown[fMaxL * fDownFloats];    // dense_1 transposed: [in][132]
    __shared__ float sTap[fMaxL * fTile * tD];
    __shared__ __attribute__((aligned(16))) float sD[fEnvsPerWg * fTile * fXLd];      // per wave: DM, then dPre
    __shared__ __attribute__((aligned(16))) float sU[fEnvsPerWg * fTile * fULd];      // per wave: DU
    __shared__ float sYin[fEnvsPerWg * fTile * fXLd];                                // per wave: the layer's input tile
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ float sCw[fMaxL * fCwFloats];
    const int l = lane & 15, q = lane >> 4, W = cfg.window;
    fmlp_stage<true>(cfg, w, sUp, sDown, sCw);
    __syncthreads();
    fmlp_taps(cfg, sCw, sTap);
    __syncthreads();
    float* db = sD + wv * fTile * fXLd;
    float* ut = sU + wv * fTile * fULd;
    float* yin = sYin + wv * fTile * fXLd;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long r = ((long)blockIdx.x * walks + it_w) * fEnvsPerWg + wv;
        if (r >= R) continue;                              // wave-uniform; only wave barriers below
        const int p = row_t[r];
        float dy0[4], dy1[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {                   // row W - 1 is the position's own slot; position 0 has none
            const bool top = p >= 1 && 4 * q + rr == W - 1;
            dy0[rr] = top ? dH[(size_t)r * tD + l] : 0.f;
            dy1[rr] = top ? dH[(size_t)r * tD + 16 + l] : 0.f;
        }
        for (int lay = cfg.nlayers - 1; lay >= 0; --lay) {
            const float* tap = sTap + lay * fTile * tD;
            const size_t rows16 = ((size_t)lay * R + r) * fTile;
            // ---- ffn.ln backward: DN2 = dY, DM = the gradient at A + M ----
            f32x4 dm0, dm1;
            {
                const float g0 = w.ln_w[lay][l], g1 = w.ln_w[lay][16 + l];
                float h0[4], h1[4], rs[4];                 // every load of the phase ahead of its first store (the pointers may alias for all the compiler knows)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const size_t row = rows16 + 4 * q + rr;
                    h0[rr] = keep.XH2[row * tD + l]; h1[rr] = keep.XH2[row * tD + 16 + l]; rs[rr] = keep.RSTD2[row];
                }
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const size_t row = rows16 + 4 * q + rr;
                    float o0, o1;
                    fmlp_ln_bwd(dy0[rr], dy1[rr], h0[rr], h1[rr], g0, g1, rs[rr], o0, o1);
                    out.DN2[row * tD + l] = dy0[rr]; out.DN2[row * tD + 16 + l] = dy1[rr];
                    out.DM[row * tD + l] = o0; out.DM[row * tD + 16 + l] = o1;
                    db[(4 * q + rr) * fXLd + l] = o0; db[(4 * q + rr) * fXLd + 16 + l] = o1;
                    dm0[rr] = o0; dm1[rr] = o1;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // ---- dG = DM W2 (the forward's 32 -> 128 product on the transposed weights);  DU = dG gelu'(U), gelu'(u) = Phi(u) + u phi(u);  U <- gelu(U) ----
            {
                f32x4 acc[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
                f32x4 uu[8];                               // the 32 loads in flight while the product runs, ahead of the phase's first store
#pragma unroll
                for (int c = 0; c < 8; ++c) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) uu[c][rr] = keep.U[(rows16 + 4 * q + rr) * fHid + 16 * c + l];
                }
                fmlp_up(db, sUp + lay * fUpFloats, l, q, acc);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int i = 4 * q + rr;
                        const size_t at = (rows16 + i) * fHid + 16 * c + l;
                        const float u = uu[c][rr];
                        const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752f));
                        const float pdf = 0.39894228040143268f * expf(-0.5f * u * u);
                        const float du = acc[c][rr] * __builtin_fmaf(u, pdf, cdf);
                        keep.U[at] = u * cdf;
                        out.DU[at] = du;
                        ut[i * fULd + 16 * c + l] = du;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            // ---- dA = DM + DU W1 (the accumulators start from the residual path);  filter.ln backward: DN1 = dA, dPre = the gradient at Y + F ----
            fmlp_down(ut, sDown + lay * fDownFloats, l, q, dm0, dm1);
            float dp0[4], dp1[4];
            {
                const float g0 = w.fln_w[lay][l], g1 = w.fln_w[lay][16 + l];
                float h0[4], h1[4], rs[4], y0[4], y1[4];   // again every load ahead of the first store
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const size_t row = rows16 + 4 * q + rr;
                    h0[rr] = keep.XH1[row * tD + l]; h1[rr] = keep.XH1[row * tD + 16 + l]; rs[rr] = keep.RSTD1[row];
                    y0[rr] = keep.YIN[row * tD + l]; y1[rr] = keep.YIN[row * tD + 16 + l];
                }
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const size_t row = rows16 + 4 * q + rr;
                    fmlp_ln_bwd(dm0[rr], dm1[rr], h0[rr], h1[rr], g0, g1, rs[rr], dp0[rr], dp1[rr]);
                    out.DN1[row * tD + l] = dm0[rr]; out.DN1[row * tD + 16 + l] = dm1[rr];
                    db[(4 * q + rr) * fXLd + l] = dp0[rr]; db[(4 * q + rr) * fXLd + 16 + l] = dp1[rr];      // DM's reads ended two barriers ago
                    yin[(4 * q + rr) * fXLd + l] = y0[rr]; yin[(4 * q + rr) * fXLd + 16 + l] = y1[rr];
                }
            }
            __builtin_amdgcn_wave_barrier();
            // ---- the filter's two correlations, i ascending, rows < W only: dY^{l-1}[m] = dPre[m] + sum_i h[(i-m) mod W] dPre[i];
            //      DHP[n] = sum_i dPre[i] Y^{l-1}[(i-n) mod W] ----
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int t = 4 * q + rr;
                const bool valid = t < W;
                const int tv = valid ? t : 0;
                float s0 = 0.f, s1 = 0.f, k0 = 0.f, k1 = 0.f;
                for (int i = 0; i < W; ++i) {
                    int n = i - tv;
                    n += n < 0 ? W : 0;
                    const float g0 = db[i * fXLd + l], g1 = db[i * fXLd + 16 + l];
                    s0 = __builtin_fmaf(tap[n * tD + l], g0, s0); s1 = __builtin_fmaf(tap[n * tD + 16 + l], g1, s1);
                    k0 = __builtin_fmaf(g0, yin[n * fXLd + l], k0); k1 = __builtin_fmaf(g1, yin[n * fXLd + 16 + l], k1);
                }
                dy0[rr] = valid ? dp0[rr] + s0 : 0.f; dy1[rr] = valid ? dp1[rr] + s1 : 0.f;
                out.DHP[(rows16 + t) * tD + l] = valid ? k0 : 0.f; out.DHP[(rows16 + t) * tD + 16 + l] = valid ? k1 : 0.f;
            }
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            float* dw = out.DWIN + ((size_t)r * fTile + 4 * q + rr) * tD;
            dw[l] = dy0[rr]; dw[16 + l] = dy1[rr];
        }
    }
}

// (X) dX from the rows' tile gradients.  Row (b, 0) collects dH of every position of its env, row (b, k >= 1) tile row W - 1 - (p - k) of every position p
// whose tile holds slot k; p ascending.  No carry between rows: 32 lanes per row, 8 rows per workgroup.
__global__ __launch_bounds__(256) void fmlp_window_bwd(const float* __restrict__ dH, const float* __restrict__ DWIN, const int32_t* __restrict__ row_env,
                                                       const int32_t* __restrict__ row_t, const int32_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ lens, int R, int W, float* __restrict__ dX) {
    const long r = blockIdx.x * 8L + (threadIdx.x >> 5);
    if (r >= R) return;
    const int d = threadIdx.x & 31, b = row_env[r], k = row_t[r], len = lens[b];
    const size_t base = (size_t)offsets[b];
    float acc = 0.f;
    if (k == 0) {
#pragma unroll 4
        for (int p = 0; p < len; ++p) acc += dH[(base + p) * tD + d];
    } else {
        const int last = (int)std::min<long>(len - 1, (long)k + W - 1);
#pragma unroll 4
        for (int p = k; p <= last; ++p) acc += DWIN[((base + p) * fTile + (W - 1 - (p - k))) * tD + d];
    }
    dX[(size_t)r * tD + d] = acc;
}

// (T) the summed tap gradient DH [L][16 32] -> d complex_weight_l [W/2+1][32][2]:
//   d re[k,d] = (c_k / W) sum_n dh[n,d] cos(2 pi (k n mod W) / W),  d im[k,d] = -(c_k / W) sum_n dh[n,d] sin(2 pi (k n mod W) / W)   (n ascending)
// and an exact 0 for the imaginary parts of the DC and the Nyquist bin, which the forward does not read.
__global__ __launch_bounds__(256) void fmlp_filter_grad(cirs_fmlp_cfg cfg, cirs_fmlp_grads g, const float* __restrict__ DH) {
    const int W = cfg.window, bins = W / 2 + 1;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cfg.nlayers * bins * tD) return;
    const int lay = idx / (bins * tD), rem = idx - lay * bins * tD, k = rem >> 5, d = rem & 31;
    const float* dh = DH + lay * fTile * tD;
    float re = 0.f, im = 0.f;
    for (int n = 0; n < W; ++n) {
        const float x = (float)(2 * ((k * n) % W)) / (float)W;
        const float v = dh[n * tD + d];
        re = __builtin_fmaf(v, cospif(x), re);
        im = __builtin_fmaf(v, sinpif(x), im);
    }
    const bool real_bin = k == 0 || 2 * k == W;
    const float scale = (real_bin ? 1.0f : 2.0f) / (float)W;
    float* dst = g.cw[lay] + (size_t)(k * tD + d) * 2;
    dst[0] = scale * re;
    dst[1] = real_bin ? 0.f : -(scale * im);
}

struct FmlpScratch : SlotScratch {
    float *G, *H, *dH, *dX, *ONES, *YIN, *XH1, *A, *XH2, *RSTD1, *RSTD2, *U, *DN2, *DM, *DU, *DN1, *DHP, *DWIN, *DH;
};

// the pass's list: decoder (S <= 32), ffn_user, gate; per layer dense_2, dense_1, the two LayerNorms and the tap gradient -- 3 + 5 L problems
static size_t fmlp_partial_floats(const cirs_fmlp_cfg* cfg, long R) {
    return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1) +
           (size_t)cfg->nlayers * (dw_list_floats(R, tD, fHid) + dw_list_floats(R, fHid, tD) + 2 * dw_list_floats(R, tD, tD) + dw_list_floats(R, 1, fTile * tD));
}

static FmlpScratch carve_fmlp(void* ws, const cirs_fmlp_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    const size_t nl = (size_t)cfg->nlayers, t32 = nl * R * fTile * tD, t128 = nl * R * fTile * fHid;
    FmlpScratch s;
    s.G = c.take((size_t)R * 32); s.H = c.take((size_t)R * tD); s.dH = c.take((size_t)R * tD); s.dX = c.take((size_t)R * tD); s.ONES = c.take((size_t)R);
    s.YIN = c.take(t32); s.XH1 = c.take(t32); s.A = c.take(t32); s.XH2 = c.take(t32);
    s.RSTD1 = c.take(nl * R * fTile); s.RSTD2 = c.take(nl * R * fTile);
    s.U = c.take(t128);
    s.DN2 = c.take(t32); s.DM = c.take(t32); s.DU = c.take(t128); s.DN1 = c.take(t32); s.DHP = c.take(t32);
    s.DWIN = c.take((size_t)R * fTile * tD);
    s.DH = c.take((size_t)fMaxL * fTile * tD);
    carve_slots(c, s, R, cfg->n_env, fmlp_partial_floats(cfg, R));
    *total_floats = c.total();
    return s;
}

// the cfg first and on its own: a cfg outside the fixed sizes is refused before any pointer is read
static int validate_fmlp_cfg(const cirs_fmlp_cfg* cfg) {
    CIRS_REQUIRE(cfg, "fmlp tracker: cfg null");
    CIRS_REQUIRE(cfg->window >= 1 && cfg->window <= fTile, "fmlp tracker: window must be in 1..16");
    CIRS_REQUIRE(cfg->nlayers >= 1 && cfg->nlayers <= fMaxL, "fmlp tracker: nlayers must be 1 or 2");
    return validate_slot_cfg(cfg, "fmlp tracker");
}

static int validate_fmlp(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w) {
    if (int rc = validate_fmlp_cfg(cfg)) return rc;
    CIRS_REQUIRE(w, "fmlp tracker: weights null");
    if (int rc = validate_slot_weights(w, "fmlp tracker")) return rc;
    for (int l = 0; l < cfg->nlayers; ++l) {
        CIRS_REQUIRE(w->cw[l] && w->fln_w[l] && w->fln_b[l], "fmlp tracker: filter weight pointer null (cw / fln_w / fln_b)");
        CIRS_REQUIRE(w->d1_w[l] && w->d1_b[l] && w->d2_w[l] && w->d2_b[l] && w->ln_w[l] && w->ln_b[l],
                     "fmlp tracker: feed-forward weight pointer null (d1 / d2 / ln)");
    }
    return CIRS_OK;
}

static int launch_fmlp_step(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w, cirs_fmlp_state* st, const int32_t* users, const int64_t* items,
                            const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_REQUIRE(st && st->x_hist && st->len, "fmlp tracker: state pointer null");
    // 131 328 bytes of LDS (70 656 of it the two layers' dense weights, staged for both layers' slots whatever nlayers is; 43 008 the four wavefronts'
    // tiles): one workgroup per CU, one wavefront per SIMD.  Up to 4 x 1 x CUs envs every env has a wavefront of its own, beyond that a workgroup walks
    // several groups of four and what it staged serves them all.  Derived from the LDS footprint, not tuned.
    const int walks = slot_walks(n, fEnvsPerWg, fWgPerCu);
    hipLaunchKernelGGL(fmlp_step_kernel, dim3(cdiv(n, (long)fEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n,
                       state_out, state_stride, walks);
    CIRS_CHECK_LAUNCH("fmlp_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_fmlp_tracker_init(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w, cirs_fmlp_state* st, const int32_t* users,
                                      const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_fmlp, cirs::launch_fmlp_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_fmlp_tracker_step(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w, cirs_fmlp_state* st, const int64_t* items, const double* rew,
                                      const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_fmlp, cirs::launch_fmlp_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_fmlp_tracker_backward_workspace_bytes(const cirs_fmlp_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_fmlp_cfg, cirs::carve_fmlp, cfg, n_rows);
}

extern "C" int cirs_fmlp_tracker_backward(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w, const cirs_fmlp_state* st, const int32_t* users,
                                          const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                          const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_fmlp_grads* grads, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_fmlp(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_slot_grads(grads, "fmlp tracker")) return rc;
    for (int l = 0; l < cfg->nlayers; ++l)
        CIRS_REQUIRE(grads->cw[l] && grads->fln_w[l] && grads->fln_b[l] && grads->d1_w[l] && grads->d1_b[l] && grads->d2_w[l] && grads->d2_b[l] &&
                         grads->ln_w[l] && grads->ln_b[l],
                     "fmlp tracker: layer gradient pointer null");
    CIRS_REQUIRE((long)n_rows * fTile < (1L << 27), "fmlp tracker: n_rows * 16 out of range");
    CIRS_REQUIRE(workspace_bytes >= cirs_fmlp_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, W = cfg->window, nl = cfg->nlayers;
    size_t total = 0;
    FmlpScratch sc = carve_fmlp(workspace, cfg, R, &total);
    DwList dwl{};
    const FmlpKeep keep{sc.YIN, sc.XH1, sc.A, sc.XH2, sc.RSTD1, sc.RSTD2, sc.U};
    hipLaunchKernelGGL(gather_dstate, dim3(cdiv((long)R * S, 256)), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    const int walks = slot_walks(R, fEnvsPerWg, fWgPerCu);
    hipLaunchKernelGGL(fmlp_rows_fwd, dim3(cdiv(R, (long)fEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, (const float*)st->x_hist, row_env, row_t, R, walks,
                       sc.H, sc.ONES, keep);
    launch_rows_gemm_dw(dwl, sc.H, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0, sc.dH,
                        tD, s);
    hipLaunchKernelGGL(fmlp_rows_bwd, dim3(cdiv(R, (long)fEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, R, walks, row_t, (const float*)sc.dH, keep,
                       FmlpBwdOut{sc.DN2, sc.DM, sc.DU, sc.DN1, sc.DHP, sc.DWIN});
    CIRS_CHECK_LAUNCH("fmlp tracker backward rows");
    const size_t per32 = (size_t)R * fTile * tD, per128 = (size_t)R * fTile * fHid;
    for (int l = 0; l < nl; ++l) {   // over the R 16 (row, tile row) pairs, in the slab count of the pass; every operand row >= W of a dY is zero
        DwBatch bt{};
        dw_batch_add(bt, dwl, sc.DM + l * per32, tD, sc.U + l * per128, fHid, R, tD, fHid, grads->d2_w[l], grads->d2_b[l], 0, sc.partial);
        dw_batch_add(bt, dwl, sc.DU + l * per128, fHid, sc.A + l * per32, tD, R, fHid, tD, grads->d1_w[l], grads->d1_b[l], 0, sc.partial);
        dw_batch_add(bt, dwl, sc.DN2 + l * per32, tD, sc.XH2 + l * per32, tD, R, tD, tD, grads->ln_w[l], grads->ln_b[l], 1, sc.partial);
        dw_batch_add(bt, dwl, sc.DN1 + l * per32, tD, sc.XH1 + l * per32, tD, R, tD, tD, grads->fln_w[l], grads->fln_b[l], 1, sc.partial);
        dw_batch_launch(bt, R, s, R * fTile);
    }
    {   // per row: the tap gradient = the column sums of DHP's first W tile rows, as the product of a column of ones with them
        DwBatch bt{};
        for (int l = 0; l < nl; ++l)
            dw_batch_add(bt, dwl, sc.ONES, 1, sc.DHP + l * per32, fTile * tD, R, 1, W * tD, sc.DH + (size_t)l * fTile * tD, nullptr, 0, sc.partial);
        dw_batch_launch(bt, R, s);
    }
    hipLaunchKernelGGL(fmlp_window_bwd, dim3(cdiv(R, 8)), dim3(256), 0, s, (const float*)sc.dH, (const float*)sc.DWIN, row_env, row_t, offsets, lens, R, W,
                       sc.dX);
    CIRS_CHECK_LAUNCH("fmlp tracker backward window");
    if (int rc = slots_backward(cfg, w, grads, sc.dX, users, act, rew, row_env, row_t, lens, R, dwl, sc, s)) return rc;
    hipLaunchKernelGGL(fmlp_filter_grad, dim3(cdiv((long)nl * (W / 2 + 1) * tD, 256)), dim3(256), 0, s, *cfg, *grads, (const float*)sc.DH);
    CIRS_CHECK_LAUNCH("fmlp_filter_grad");
    return CIRS_OK;
}
