// nextitnet_tracker.hip -- StateTrackerNextItNet for gfx950: residual blocks of dilated causal 1-D convolutions (width 3) over the item slots.
//
// The reference has no counterpart; the model is defined here, in include/cirs_hip.h and in DESIGN.md 7.6:
//   inputs    the other trackers' slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k -- no sqrt(D) scale, no positional encoding
//   blocks    y^{-1}_t = x_t (t >= 1);  c^l_t = b_l + sum_{j<3} W_l[:,:,j] y^{l-1}_{t-(2-j) d_l}, y^{l-1}_s = 0 for s < 1 (zero padding at EVERY layer's input);
//             n^l_t = LayerNorm_l(c^l_t);  y^l_t = y^{l-1}_t + relu(n^l_t)
//   state     h_p = x_0 + y^{n-1}_p (p >= 1), h_0 = x_0;  s_p = decoder(h_p)
// The tile: position p is computed from a tile of 16 rows, row t = slot p - 15 + t (row 15 = the newest item), with 8 zero rows in front for the taps that
// reach before the tile.  Every block is computed on ALL 16 rows; the receptive field R = 1 + 2 sum d_l <= 15 keeps the cone of row 15 inside the tile, rows
// outside the cone hold values of a truncated history and reach nothing that is read.  A row whose slot is < 1 (before the first item) is written as the zero
// row after every block: zero padding at every layer's input, not LayerNorm(bias) carried upwards.
// Step (one launch appends one position for n envs): ONE env per wavefront, four per workgroup.  A workgroup stages every block's conv weights k-major
// ([out][32 tap + in], stride 100), the decoder [k][33] and the slot's matrix [d][33] in LDS once, a wavefront its tile [24][36].  A block is one
// [16 positions] x [32 out] x [96] product on v_mfma_f32_16x16x4_f32, the two 16-channel output tiles as independent accumulators that start from the bias.
// LayerNorm, the residual add and the decoder are plain FMAs.  Everything per env is predicated, not branched.
//
// Backward (rows = (env b, position p < len_b), env-major; no sequential pass):
//   F  nin_rows_fwd: the forward of every row again from the stored slots (the step kernel's device functions) -> per block the input tile with its zero front
//      rows (YIN), the normalised values (NH) and the inverse standard deviations (RSTD); h
//   C  G = gather(dstate); dH = G W_dec and the decoder's weight gradient in one launch (rows_gemm + dw_gemm, as the other trackers' stage C)
//   B  nin_rows_bwd, top block down, dy^{top} = dH at row 15: dn = dy [n > 0]; LayerNorm backward -> dc (DC, laid out like YIN) and dn (DN);
//      dy^{l-1}_s = dy^l_s + sum_j W_l[:,:,j]^T dc_{s+(2-j) d_l} -- the same MFMA product on the transposed weights and a tile with zero BACK rows;
//      rows before the first item are cleared at every level.  Ends in DWIN [R, 16, 32]: a gradient per tile row
//   W  weight gradients through the slab partials.  Tap j of block l is the plain product DC_l^T (YIN_l shifted by (2-j) d_l rows): the zero front rows make
//      the shift a base-pointer offset.  3 n_blocks problems in a list of their own (into a [block][tap][out][in] buffer, transposed to torch's [out][in][tap]
//      by nin_taps_to_torch); LayerNorm weight / bias = the diagonal / column sums of DN^T NH, in the pass's main list
//   X  nin_window_bwd: dX[b,0] = sum_p dH[b,p];  dX[b,k] = sum_{p=k}^{min(len_b-1, k+R-1)} DWIN_p[k - p + 15]  -- p ascending, every row on its own
//   E  the slot stage of the recurrent trackers (slot_tracker.h)
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include "slot_tracker.h"

namespace cirs {

constexpr int nMaxBlocks = CIRS_NEXTITNET_MAX_BLOCKS;      // 4
constexpr int nTile = 16;                                  // rows of a tile: row t = slot p - 15 + t
constexpr int nFront = 2 * CIRS_NEXTITNET_MAX_DILATION;    // 8 zero rows: the farthest tap of the widest dilation
constexpr int nRows = nFront + nTile;                      // 24
constexpr int nYLd = tD + 4;                               // LDS stride of a tile row: 36 (16-byte aligned rows, row starts spread over the banks)
constexpr int nK = 3 * tD;                                 // 96: the contraction of a block, k = 32 tap + in
constexpr int nWLd = nK + 4;                               // LDS stride of an output channel's weights: 100
constexpr int nWFloats = tD * nWLd;                        // one block: 3200 floats
constexpr int nLds = tD + 1;                               // LDS stride of a staged 32-row matrix, as in avg_tracker.hip
constexpr int nEnvsPerWg = 4;                              // one env (or buffer row) per wavefront
constexpr int nWgPerCu = 2;                                // 73 KB of LDS per workgroup: two fit in a CU's 160 KB
constexpr float nEps = 1e-5f;

// every block's conv weights, once per workgroup: coalesced dword reads of torch's [out][in][tap] (the tensors are views of one flat buffer: no alignment
// beyond a float's), written k-major [out][32 tap + in] for the forward (kT: [in][32 tap + out] for the backward's transposed product).  Fixed trip counts,
// predicated: a thread's 48 loads are all issued before its first LDS store, one round trip to the L2 instead of one per block.
template <bool kT>
__device__ __forceinline__ void nin_stage(const cirs_nextitnet_cfg& cfg, const cirs_nextitnet_weights& w, float* sW) {
    float v[nMaxBlocks][12];
#pragma unroll
    for (int b = 0; b < nMaxBlocks; ++b) {
        const float* src = w.conv_w[b];
#pragma unroll
        for (int u = 0; u < 12; ++u) v[b][u] = b < cfg.n_blocks ? src[threadIdx.x + 256 * u] : 0.f;
    }
#pragma unroll
    for (int b = 0; b < nMaxBlocks; ++b) {
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            const int q = threadIdx.x + 256 * u, o = q / nK, rem = q - o * nK, i = rem / 3, j = rem - 3 * i;      // q = (o 32 + i) 3 + j
            if (b < cfg.n_blocks) sW[b * nWFloats + (kT ? i * nWLd + tD * j + o : o * nWLd + tD * j + i)] = v[b][u];
        }
    }
}

// acc[t][o] += sum_{j<3} sum_{c<32} buf[row0 + t + (2 - j) step][c] * sWl[o][32 j + c] for the 16 rows t and the 32 columns o, on v_mfma_f32_16x16x4_f32:
// lane (l = lane & 15, q = lane >> 4) supplies row t = l of A and columns o = l (acc0) and o = 16 + l (acc1) of B; of a block of 16 contraction indices it
// holds 4 q .. 4 q + 3 (one ds_read_b128 each), MFMA i of the block contracts {i, 4 + i, 8 + i, 12 + i}: a fixed order.  It receives acc[4 q + r][o], r = 0..3.
// The forward reads the tile behind its zero front rows (row0 = nFront, step = -d), the backward the gradient tile before its zero back rows (row0 = 0, step = d).
__device__ __forceinline__ void nin_product(const float* buf, int row0, int step, const float* sWl, int l, int q, f32x4& acc0, f32x4& acc1) {
    const float* w0 = sWl + l * nWLd + 4 * q;
    const float* w1 = w0 + 16 * nWLd;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* ar = buf + (row0 + l + (2 - j) * step) * nYLd + 4 * q;
#pragma unroll
        for (int kk = 0; kk < tD; kk += 16) {
            const float4 a = *reinterpret_cast<const float4*>(ar + kk);
            const float4 b0 = *reinterpret_cast<const float4*>(w0 + j * tD + kk);
            const float4 b1 = *reinterpret_cast<const float4*>(w1 + j * tD + kk);
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
}

// the sum over the 32 channels of a position: the lane's two tiles, then the 16 lanes of its quarter (xor 1, 2, 4, 8): the same order in every lane
__device__ __forceinline__ float nin_channel_sum(float a, float b) {
    float s = a + b;
#pragma unroll
    for (int sft = 1; sft <= 8; sft <<= 1) s += __shfl_xor(s, sft, CIRS_WAVE);
    return s;
}

// what the backward keeps of a row's forward, per block: YIN [n_blocks][256 + R 24 32] (256 zero floats in front of every block: the shifted reads of row 0),
// NH [n_blocks][R 16 32], RSTD [n_blocks][R 16]
struct NinKeep { float *YIN, *NH, *RSTD; };

// the blocks over a wavefront's tile ybuf [24][36] (rows 0 .. 7 zero, row 8 + t = slot pos - 15 + t), in place.  kKeep: the backward's copy of row r (of R).
template <bool kKeep>
__device__ __forceinline__ void nin_blocks(const cirs_nextitnet_cfg& cfg, const cirs_nextitnet_weights& w, const float* sW, float* ybuf, int pos, int lane,
                                           const NinKeep& keep, long r, long R, bool live) {
    const int l = lane & 15, q = lane >> 4;
    for (int b = 0; b < cfg.n_blocks; ++b) {
        const int dil = cfg.dilations[b];
        if (kKeep) {
            float* dst = keep.YIN + (size_t)b * (256 + (size_t)R * nRows * tD) + 256 + (size_t)r * nRows * tD;
#pragma unroll
            for (int u = 0; u < nRows * tD / 64; ++u) {
                const int idx = lane + 64 * u;
                if (live) dst[idx] = ybuf[(idx >> 5) * nYLd + (idx & 31)];
            }
        }
        const float b0 = w.conv_b[b][l], b1 = w.conv_b[b][16 + l];
        const float g0 = w.ln_w[b][l], g1 = w.ln_w[b][16 + l], e0 = w.ln_b[b][l], e1 = w.ln_b[b][16 + l];
        f32x4 acc0 = f32x4{b0, b0, b0, b0}, acc1 = f32x4{b1, b1, b1, b1};
        nin_product(ybuf, nFront, -dil, sW + b * nWFloats, l, q, acc0, acc1);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int t = 4 * q + rr;
            const float mean = nin_channel_sum(acc0[rr], acc1[rr]) * (1.0f / tD);
            const float c0 = acc0[rr] - mean, c1 = acc1[rr] - mean;
            const float var = nin_channel_sum(c0 * c0, c1 * c1) * (1.0f / tD);
            const float rstd = 1.0f / sqrtf(var + nEps);
            const float h0 = c0 * rstd, h1 = c1 * rstd;
            const float n0 = __builtin_fmaf(h0, g0, e0), n1 = __builtin_fmaf(h1, g1, e1);
            float* yr = ybuf + (nFront + t) * nYLd;
            const bool item = pos - (nTile - 1) + t >= 1;       // a row before the first item stays the zero row
            yr[l] = item ? yr[l] + fmaxf(n0, 0.f) : 0.f;
            yr[16 + l] = item ? yr[16 + l] + fmaxf(n1, 0.f) : 0.f;
            if (kKeep && live) {
                float* nh = keep.NH + ((size_t)b * R * nTile + (size_t)r * nTile + t) * tD;
                nh[l] = h0; nh[16 + l] = h1;
                if (l == 0) keep.RSTD[(size_t)b * R * nTile + (size_t)r * nTile + t] = rstd;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(256) void nin_step_kernel(cirs_nextitnet_cfg cfg, cirs_nextitnet_weights w, cirs_nextitnet_state st,
                                                       const int32_t* __restrict__ users, const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                       const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                       float* __restrict__ state_out, long state_stride, int walks, int rf) {
    __shared__ __attribute__((aligned(16))) float sW[nMaxBlocks * nWFloats];
    __shared__ float sDec[tD * nLds];                      // [k][s]: decoder, transposed
    __shared__ float sIn[tD * nLds];                       // [d][c]: fnn_gate [32][33] (step) or ffn_user [32][32] (init), row-major
    __shared__ __attribute__((aligned(16))) float sY[nEnvsPerWg * nRows * nYLd];
    __shared__ float sVec[nEnvsPerWg * tD];                // per wave: the slot's input vector
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state;
    const bool is_init = users != nullptr;
    nin_stage<false>(cfg, w, sW);
    for (int q = threadIdx.x; q < nEnvsPerWg * nRows * nYLd; q += 256) sY[q] = 0.f;      // the front rows stay zero: nothing below writes them
    for (int q = threadIdx.x; q < S * tD; q += 256) sDec[(q & 31) * nLds + (q >> 5)] = w.dec_w[q];
    if (is_init) {
        for (int q = threadIdx.x; q < tD * tD; q += 256) sIn[(q >> 5) * nLds + (q & 31)] = w.ffn_user_w[q];
    } else {
        for (int q = threadIdx.x; q < tD * (tD + 1); q += 256) sIn[q] = w.gate_w[q];
    }
    __syncthreads();
    float* vin = sVec + wv * tD;
    float* ybuf = sY + wv * nRows * nYLd;
    const float* mrow = sIn + d * nLds;
    const NinKeep none{nullptr, nullptr, nullptr};
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long j = ((long)blockIdx.x * walks + it_w) * nEnvsPerWg + wv;
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
        // ---- 1. the stored rows of the tile (the last R - 1 item slots before the new one, zero rows in front): all requested at once, ahead of the slot's
        //         arithmetic ----
        const float* xh = st.x_hist + hist + d;
        float wl[nTile / 2];
#pragma unroll
        for (int q = 0; q < nTile / 2; ++q) {
            const int t = 2 * q + half, k = pos - (nTile - 1) + t;
            wl[q] = (t >= nTile - rf && k >= 1 && k < pos) ? xh[(size_t)k * tD] : 0.f;
        }
        // ---- 2. the new input slot (both halves of the wavefront hold it); it is the tile's last row (pos >= 1) ----
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
        for (int q = 0; q < nTile / 2; ++q) {
            const int t = 2 * q + half;
            ybuf[(nFront + t) * nYLd + d] = (pos >= 1 && t == nTile - 1) ? x : wl[q];
        }
        const float x0 = is_init ? x : (ok ? xh[0] : 0.f);
        if (ok && half == 0) st.x_hist[hist + (size_t)pos * tD + d] = x;
        __builtin_amdgcn_wave_barrier();
        // ---- 3. the blocks; h = x_0 + the top block's last row (the zero row at position 0) ----
        nin_blocks<false>(cfg, w, sW, ybuf, pos, lane, none, 0, 0, false);
        const float h = x0 + ybuf[(nFront + nTile - 1) * nYLd + d];
        __builtin_amdgcn_wave_barrier();
        vin[d] = h;
        __builtin_amdgcn_wave_barrier();
        // ---- 4. decoder ----
        if (d < S && half == 0) {
            float acc = w.dec_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(sDec[k * nLds + d], vin[k], acc);
            if (ok) state_out[(size_t)j * state_stride + d] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (ok && lane == 0) st.len[e] = pos + 1;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// (F) the forward of every buffer row again, one row per wavefront
__global__ __launch_bounds__(256) void nin_rows_fwd(cirs_nextitnet_cfg cfg, cirs_nextitnet_weights w, const float* __restrict__ x_hist,
                                                    const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t, int R, int walks, int rf,
                                                    float* __restrict__ H, NinKeep keep) {
    __shared__ __attribute__((aligned(16))) float sW[nMaxBlocks * nWFloats];
    __shared__ __attribute__((aligned(16))) float sY[nEnvsPerWg * nRows * nYLd];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int L = cfg.max_len;
    nin_stage<false>(cfg, w, sW);
    for (int q = threadIdx.x; q < nEnvsPerWg * nRows * nYLd; q += 256) sY[q] = 0.f;
    if (blockIdx.x == 0)
        for (int b = 0; b < cfg.n_blocks; ++b) keep.YIN[(size_t)b * (256 + (size_t)R * nRows * tD) + threadIdx.x] = 0.f;
    __syncthreads();
    float* ybuf = sY + wv * nRows * nYLd;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long r = ((long)blockIdx.x * walks + it_w) * nEnvsPerWg + wv;
        const bool live = r < R;
        const long rr = live ? r : 0;
        const int p = row_t[rr];
        const float* xh = x_hist + (size_t)row_env[rr] * L * tD + d;
        float wl[nTile / 2];
#pragma unroll
        for (int q = 0; q < nTile / 2; ++q) {      // all requested at once
            const int t = 2 * q + half, k = p - (nTile - 1) + t;
            wl[q] = (t >= nTile - rf && k >= 1) ? xh[(size_t)k * tD] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < nTile / 2; ++q) ybuf[(nFront + 2 * q + half) * nYLd + d] = wl[q];
        __builtin_amdgcn_wave_barrier();
        nin_blocks<true>(cfg, w, sW, ybuf, p, lane, keep, rr, R, live);
        if (live && half == 0) H[(size_t)r * tD + d] = xh[0] + ybuf[(nFront + nTile - 1) * nYLd + d];
        __builtin_amdgcn_wave_barrier();
    }
}

// (B) one row per wavefront, top block down, in the layout of the forward's accumulators (lane (l, q): rows 4 q .. 4 q + 3, channels l and 16 + l).
// DC [n_blocks][R 24 32]: row (r, 8 + t) = dc of tile row t, the 8 front rows zero (they face YIN's front rows in the tap products).
__global__ __launch_bounds__(256) void nin_rows_bwd(cirs_nextitnet_cfg cfg, cirs_nextitnet_weights w, int R, const int32_t* __restrict__ row_t,
                                                    const float* __restrict__ dH, const float* __restrict__ NH, const float* __restrict__ RSTD,
                                                    float* __restrict__ DN, float* __restrict__ DC, float* __restrict__ DWIN) {
    __shared__ __attribute__((aligned(16))) float sWT[nMaxBlocks * nWFloats];
    __shared__ __attribute__((aligned(16))) float sDc[nEnvsPerWg * nRows * nYLd];      // per wave: rows 0 .. 15 dc, rows 16 .. 23 zero
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int l = lane & 15, q = lane >> 4;
    nin_stage<true>(cfg, w, sWT);
    for (int i = threadIdx.x; i < nEnvsPerWg * nRows * nYLd; i += 256) sDc[i] = 0.f;
    __syncthreads();
    const long r = blockIdx.x * (long)nEnvsPerWg + wv;
    if (r >= R) return;
    float* dcb = sDc + wv * nRows * nYLd;
    const int p = row_t[r];
    const bool top = q == 3 && p >= 1;      // row 15 is the position's own slot; position 0 has none
    f32x4 dy0 = f32x4{0.f, 0.f, 0.f, top ? dH[(size_t)r * tD + l] : 0.f};
    f32x4 dy1 = f32x4{0.f, 0.f, 0.f, top ? dH[(size_t)r * tD + 16 + l] : 0.f};
    for (int b = cfg.n_blocks - 1; b >= 0; --b) {
        const int dil = cfg.dilations[b];
        const float g0 = w.ln_w[b][l], g1 = w.ln_w[b][16 + l], e0 = w.ln_b[b][l], e1 = w.ln_b[b][16 + l];
        const size_t rows16 = (size_t)b * R * nTile + (size_t)r * nTile;
        float* dcg = DC + ((size_t)b * R * nRows + (size_t)r * nRows) * tD;
#pragma unroll
        for (int u = 0; u < nFront * tD / 64; ++u) dcg[lane + 64 * u] = 0.f;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int t = 4 * q + rr;
            const float* nh = NH + (rows16 + t) * tD;
            const float h0 = nh[l], h1 = nh[16 + l], rstd = RSTD[rows16 + t];
            const float dn0 = __builtin_fmaf(h0, g0, e0) > 0.f ? dy0[rr] : 0.f, dn1 = __builtin_fmaf(h1, g1, e1) > 0.f ? dy1[rr] : 0.f;
            float* dn = DN + (rows16 + t) * tD;
            dn[l] = dn0; dn[16 + l] = dn1;
            const float a0 = dn0 * g0, a1 = dn1 * g1;
            const float m1 = nin_channel_sum(a0, a1) * (1.0f / tD), m2 = nin_channel_sum(a0 * h0, a1 * h1) * (1.0f / tD);
            const float dc0 = rstd * (a0 - m1 - h0 * m2), dc1 = rstd * (a1 - m1 - h1 * m2);
            dcg[(nFront + t) * tD + l] = dc0; dcg[(nFront + t) * tD + 16 + l] = dc1;
            dcb[t * nYLd + l] = dc0; dcb[t * nYLd + 16 + l] = dc1;
        }
        __builtin_amdgcn_wave_barrier();
        nin_product(dcb, 0, dil, sWT + b * nWFloats, l, q, dy0, dy1);      // the accumulators start from dy: the residual path
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            if (p - (nTile - 1) + 4 * q + rr < 1) { dy0[rr] = 0.f; dy1[rr] = 0.f; }      // a zero row of the forward is a constant
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        float* dw = DWIN + ((size_t)r * nTile + 4 * q + rr) * tD;
        dw[l] = dy0[rr]; dw[16 + l] = dy1[rr];
    }
}

// the tap products' [block][tap][out][in] -> torch's [out][in][tap]
__global__ __launch_bounds__(256) void nin_taps_to_torch(cirs_nextitnet_grads g, const float* __restrict__ TAPS) {
    const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;      // q = (o 32 + i) 3 + j
    const int oi = q / 3, j = q - 3 * oi;
    g.conv_w[b][q] = TAPS[((size_t)b * 3 + j) * tD * tD + oi];
}

// (X) dX from the rows' tile gradients.  Row (b, 0) collects dH of every position of its env, row (b, k >= 1) tile row k - p + 15 of every position p whose
// receptive field holds slot k; p ascending.  No carry between rows: 32 lanes per row, 8 rows per workgroup.
__global__ __launch_bounds__(256) void nin_window_bwd(const float* __restrict__ dH, const float* __restrict__ DWIN, const int32_t* __restrict__ row_env,
                                                      const int32_t* __restrict__ row_t, const int32_t* __restrict__ offsets,
                                                      const int32_t* __restrict__ lens, int R, int rf, float* __restrict__ dX) {
    const long r = blockIdx.x * 8L + (threadIdx.x >> 5);
    if (r >= R) return;
    const int d = threadIdx.x & 31, b = row_env[r], k = row_t[r], len = lens[b];
    const size_t base = (size_t)offsets[b];
    float acc = 0.f;
    if (k == 0) {
#pragma unroll 4
        for (int p = 0; p < len; ++p) acc += dH[(base + p) * tD + d];
    } else {
        const int last = (int)std::min<long>(len - 1, (long)k + rf - 1);
#pragma unroll 4
        for (int p = k; p <= last; ++p) acc += DWIN[((base + p) * nTile + (k - p + nTile - 1)) * tD + d];
    }
    dX[(size_t)r * tD + d] = acc;
}

struct NinScratch : SlotScratch {
    float *G, *H, *dH, *dX, *YIN, *NH, *RSTD, *DN, *DC, *DWIN, *TAPS, *tap_partial;
};

static size_t nin_partial_floats(const cirs_nextitnet_cfg* cfg, long R) {      // the main list: decoder (S <= 32), ffn_user, gate, LayerNorm per block
    return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1) + (size_t)cfg->n_blocks * dw_list_floats(R, tD, tD);
}

static NinScratch carve_nin(void* ws, const cirs_nextitnet_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    const long nb = cfg->n_blocks;
    NinScratch s;
    s.G = c.take((size_t)R * 32); s.H = c.take((size_t)R * tD); s.dH = c.take((size_t)R * tD); s.dX = c.take((size_t)R * tD);
    s.YIN = c.take((size_t)nb * (256 + (size_t)R * nRows * tD));
    s.NH = c.take((size_t)nb * R * nTile * tD); s.RSTD = c.take((size_t)nb * R * nTile); s.DN = c.take((size_t)nb * R * nTile * tD);
    s.DC = c.take((size_t)nb * R * nRows * tD);
    s.DWIN = c.take((size_t)R * nTile * tD);
    s.TAPS = c.take((size_t)nb * 3 * tD * tD);
    s.tap_partial = c.take((size_t)nb * 3 * dw_list_floats(R, tD, tD) + 4096);
    carve_slots(c, s, R, cfg->n_env, nin_partial_floats(cfg, R));
    *total_floats = c.total();
    return s;
}

static int nin_receptive_field(const cirs_nextitnet_cfg* cfg) {
    int sum = 0;
    for (int l = 0; l < cfg->n_blocks; ++l) sum += cfg->dilations[l];
    return 1 + 2 * sum;
}

// the cfg first and on its own: a cfg outside the fixed sizes is refused before any pointer is read
static int validate_nin_cfg(const cirs_nextitnet_cfg* cfg) {
    CIRS_REQUIRE(cfg, "nextitnet tracker: cfg null");
    CIRS_REQUIRE(cfg->n_blocks >= 1 && cfg->n_blocks <= nMaxBlocks, "nextitnet tracker: n_blocks must be in 1..4");
    for (int l = 0; l < cfg->n_blocks; ++l)
        CIRS_REQUIRE(cfg->dilations[l] >= 1 && cfg->dilations[l] <= CIRS_NEXTITNET_MAX_DILATION, "nextitnet tracker: dilations must be in 1..4");
    CIRS_REQUIRE(nin_receptive_field(cfg) <= nTile - 1, "nextitnet tracker: the dilations must sum to at most 7");
    return validate_slot_cfg(cfg, "nextitnet tracker");
}

static int validate_nin(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w) {
    if (int rc = validate_nin_cfg(cfg)) return rc;
    CIRS_REQUIRE(w, "nextitnet tracker: weights null");
    if (int rc = validate_slot_weights(w, "nextitnet tracker")) return rc;
    for (int l = 0; l < cfg->n_blocks; ++l)
        CIRS_REQUIRE(w->conv_w[l] && w->conv_b[l] && w->ln_w[l] && w->ln_b[l], "nextitnet tracker: block weight pointer null");
    return CIRS_OK;
}

static int launch_nin_step(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w, cirs_nextitnet_state* st, const int32_t* users,
                           const int64_t* items, const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride,
                           hipStream_t s) {
    CIRS_REQUIRE(st && st->x_hist && st->len, "nextitnet tracker: state pointer null");
    // 73 KB of LDS (50 KB of it the four blocks' weights, staged whatever n_blocks is): two workgroups per CU.  Up to 4 x 2 x CUs envs every env has a
    // wavefront of its own, beyond that a workgroup walks several groups of four and what it staged serves them all.  Chosen from the structure, not tuned.
    const int walks = slot_walks(n, nEnvsPerWg, nWgPerCu);
    hipLaunchKernelGGL(nin_step_kernel, dim3(cdiv(n, (long)nEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n,
                       state_out, state_stride, walks, nin_receptive_field(cfg));
    CIRS_CHECK_LAUNCH("nin_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_nextitnet_tracker_init(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w, cirs_nextitnet_state* st, const int32_t* users,
                                           const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_nin, cirs::launch_nin_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_nextitnet_tracker_step(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w, cirs_nextitnet_state* st, const int64_t* items,
                                           const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride,
                                           void* stream) {
    return cirs::slot_tracker_step(cirs::validate_nin, cirs::launch_nin_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_nextitnet_tracker_backward_workspace_bytes(const cirs_nextitnet_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_nin_cfg, cirs::carve_nin, cfg, n_rows);
}

extern "C" int cirs_nextitnet_tracker_backward(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w, const cirs_nextitnet_state* st,
                                               const int32_t* users, const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                                               const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                                               const cirs_nextitnet_grads* grads, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_nin(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_slot_grads(grads, "nextitnet tracker")) return rc;
    for (int l = 0; l < cfg->n_blocks; ++l)
        CIRS_REQUIRE(grads->conv_w[l] && grads->conv_b[l] && grads->ln_w[l] && grads->ln_b[l], "nextitnet tracker: block gradient pointer null");
    CIRS_REQUIRE((long)n_rows * nRows < (1L << 27), "nextitnet tracker: n_rows * 24 out of range");
    CIRS_REQUIRE(workspace_bytes >= cirs_nextitnet_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, nb = cfg->n_blocks, rf = nin_receptive_field(cfg);
    size_t total = 0;
    NinScratch sc = carve_nin(workspace, cfg, R, &total);
    DwList dwl{};
    hipLaunchKernelGGL(gather_dstate, dim3(cdiv((long)R * S, 256)), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    const int walks = slot_walks(R, nEnvsPerWg, nWgPerCu);
    hipLaunchKernelGGL(nin_rows_fwd, dim3(cdiv(R, (long)nEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, (const float*)st->x_hist, row_env, row_t, R, walks, rf,
                       sc.H, NinKeep{sc.YIN, sc.NH, sc.RSTD});
    launch_rows_gemm_dw(dwl, sc.H, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0, sc.dH,
                        tD, s);
    hipLaunchKernelGGL(nin_rows_bwd, dim3(cdiv(R, nEnvsPerWg)), dim3(256), 0, s, *cfg, *w, R, row_t, (const float*)sc.dH, (const float*)sc.NH,
                       (const float*)sc.RSTD, sc.DN, sc.DC, sc.DWIN);
    CIRS_CHECK_LAUNCH("nextitnet tracker backward rows");
    {   // the taps over the R 24 (row, tile row) pairs, in the slab count of the pass: a list of their own (3 n_blocks problems), two blocks per launch
        DwList taps{};
        for (int b0 = 0; b0 < nb; b0 += 2) {
            DwBatch bt{};
            for (int b = b0; b < std::min(nb, b0 + 2); ++b) {
                const float* dc = sc.DC + (size_t)b * R * nRows * tD;
                const float* yin = sc.YIN + (size_t)b * (256 + (size_t)R * nRows * tD) + 256;
                for (int j = 0; j < 3; ++j)
                    dw_batch_add(bt, taps, dc, tD, yin - (size_t)(2 - j) * cfg->dilations[b] * tD, tD, R, tD, tD, sc.TAPS + ((size_t)b * 3 + j) * tD * tD,
                                 j == 2 ? grads->conv_b[b] : nullptr, 0, sc.tap_partial);
            }
            dw_batch_launch(bt, R, s, R * nRows);
        }
        launch_dw_list_final(taps, R, sc.tap_partial, s);
        hipLaunchKernelGGL(nin_taps_to_torch, dim3(3 * tD * tD / 256, nb), dim3(256), 0, s, *grads, (const float*)sc.TAPS);
    }
    {   // LayerNorm over the R 16 (row, tile row) pairs: weight = the diagonal of DN^T NH, bias = the column sums of DN
        DwBatch bt{};
        for (int b = 0; b < nb; ++b)
            dw_batch_add(bt, dwl, sc.DN + (size_t)b * R * nTile * tD, tD, sc.NH + (size_t)b * R * nTile * tD, tD, R, tD, tD, grads->ln_w[b], grads->ln_b[b], 1,
                         sc.partial);
        dw_batch_launch(bt, R, s, R * nTile);
    }
    hipLaunchKernelGGL(nin_window_bwd, dim3(cdiv(R, 8)), dim3(256), 0, s, (const float*)sc.dH, (const float*)sc.DWIN, row_env, row_t, offsets, lens, R, rf,
                       sc.dX);
    CIRS_CHECK_LAUNCH("nextitnet tracker backward window");
    return slots_backward(cfg, w, grads, sc.dX, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
