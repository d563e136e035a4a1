// stamp_tracker.hip -- StateTrackerSTAMP for gfx950: an attention pool over the window of the last item slots (STAMP, Liu et al., KDD 2018).
//
// The reference has no counterpart; the model is defined here, in include/cirs_hip.h and in DESIGN.md 7.7:
//   inputs     the other trackers' slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k -- no sqrt(D) scale, no positional encoding
//   window     n_p = min(W, p), slots k = p - n_p + 1 .. p;  m_s = (sum_k x_k) / n_p (k ascending, one division: the Avg tracker's m_p),  m_t = x_p
//   attention  c = W2 m_t + W3 m_s + b_a;  e_k = w0 . sigmoid(W1 x_k + c) (no softmax);  m_a = sum_k e_k x_k (k ascending)
//   read-out   h_s = tanh(A m_a + b_A),  h_t = tanh(B m_t + b_B);  h_p = x_0 + h_s * h_t (p >= 1), h_0 = x_0;  s_p = decoder(h_p)
// The tile: position p is computed from a tile of 16 rows, row t = slot p - 15 + t (row 15 = the newest item).  Only the rows of the window (t >= 16 - n_p)
// are ever loaded: a row outside it is the zero row whether its slot is a live older one (p > W) or lies before the first item (p < W), and its e is set
// to zero besides, so it reaches neither m_s nor m_a nor, in the backward, any gradient.
// Step (one launch appends one position for n envs): ONE env per wavefront, four per workgroup.  A workgroup stages W1 ([out][36], the MFMA's B operand),
// W2, W3, A, B, the decoder ([k][33]) and the slot's matrix ([d][33]) in LDS once, a wavefront its tile [16][36].  U = X_win W1^T is one 16 x 32 x 32 product
// on v_mfma_f32_16x16x4_f32: the two 16-column output tiles are independent accumulator chains of eight MFMAs each.  The mat-vecs are plain FMAs over the
// staged rows (lane = output row, stride 33: conflict-free); two of them run at a time, one per half of the wavefront (W2 m_t | W3 m_s, A m_a | B m_t).
// Everything per env is predicated, not branched.
//
// Backward (rows = (env b, position p < len_b), env-major; no sequential pass):
//   F  stamp_rows_fwd: the forward of every row again from the stored slots (the step kernel's device function) -> the tile (XWIN), the sigmoids (SIG), e (E),
//      m_s, m_a, h_s, h_t; h
//   C  G = gather(dstate); dH = G W_dec and the decoder's weight gradient in one launch (rows_gemm + dw_gemm, as the other trackers' stage C)
//   B  stamp_rows_bwd, one row per wavefront: the product and the two tanh (DPA, DPB); dm_a = A^T dpa, dm_t = B^T dpb; de_k = x_k . dm_a and e_k dm_a into
//      slot k; dG = (de_k w0) * s (1 - s); dX_win += dG W1 -- the same MFMA product on W1 staged transposed; dc = sum_k dG_k, W2^T dc (+ dm_t) into slot p,
//      W3^T dc / n_p into every window slot.  Ends in DWIN [R, 16, 32]: a gradient per tile row
//   W  weight gradients through the slab partials: attn.w1 = DG^T XWIN and attn.w0 = DE^T SIG over the R 16 (row, tile row) pairs; attn.w2 (+ attn.bias),
//      attn.w3, mlp_a, mlp_b per row
//   X  stamp_window_bwd: dX[b,0] = sum_p dH[b,p];  dX[b,k] = sum_{p=k}^{min(len_b-1, k+W-1)} DWIN_p[k - p + 15]  -- p ascending, every row on its own
//   E  the slot stage of the recurrent trackers (slot_tracker.h)
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include "slot_tracker.h"

namespace cirs {

constexpr int sTile = CIRS_STAMP_MAX_WINDOW;               // 16 rows of a tile: row t = slot p - 15 + t
constexpr int sXLd = tD + 4;                               // LDS stride of a tile row and of a row of the MFMA's staged operand: 36 (16-byte aligned rows)
constexpr int sLds = tD + 1;                               // LDS stride of a staged 32-row matrix, as in avg_tracker.hip
constexpr int sEnvsPerWg = 4;                              // one env (or buffer row) per wavefront
constexpr int sWgPerCu = 4;                                // 40 448 bytes of LDS per workgroup of the step kernel: four fit in a CU's 160 KB

// a row-major [32][32] matrix, once per workgroup: [row][33]
__device__ __forceinline__ void stamp_stage33(const float* __restrict__ src, float* dst) {
    for (int q = threadIdx.x; q < tD * tD; q += 256) dst[(q >> 5) * sLds + (q & 31)] = src[q];
}

// W1 [out][in] as the MFMA's B operand: [out][36] for the forward's X W1^T, kT: [in][36] for the backward's dG W1
template <bool kT>
__device__ __forceinline__ void stamp_stage_w1(const float* __restrict__ src, float* dst) {
    for (int q = threadIdx.x; q < tD * tD; q += 256) {
        const int o = q >> 5, c = q & 31;
        dst[kT ? c * sXLd + o : o * sXLd + c] = src[q];
    }
}

// acc[t][o] += sum_{c<32} tile[t][c] * sW[o][c] for the 16 rows t and the 32 columns o, on v_mfma_f32_16x16x4_f32: lane (l = lane & 15, q = lane >> 4)
// supplies row t = l of A and columns o = l (acc0) and o = 16 + l (acc1) of B; of a block of 16 contraction indices it holds 4 q .. 4 q + 3 (one
// ds_read_b128 each), MFMA i of the block contracts {i, 4 + i, 8 + i, 12 + i}: a fixed order.  It receives acc[4 q + r][o], r = 0..3.
__device__ __forceinline__ void stamp_product(const float* tile, const float* sW, int l, int q, f32x4& acc0, f32x4& acc1) {
    const float* ar = tile + l * sXLd + 4 * q;
    const float* w0 = sW + l * sXLd + 4 * q;
    const float* w1 = w0 + 16 * sXLd;
#pragma unroll
    for (int kk = 0; kk < tD; kk += 16) {
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

// the sum over the 32 columns of a tile row: the lane's two tiles, then the 16 lanes of its quarter (xor 1, 2, 4, 8): the same order in every lane
__device__ __forceinline__ float stamp_row_sum(float a, float b) {
    float s = a + b;
#pragma unroll
    for (int sft = 1; sft <= 8; sft <<= 1) s += __shfl_xor(s, sft, CIRS_WAVE);
    return s;
}

// the staged matrices of the attention and the read-out
struct StampLds { const float *W1, *W2, *W3, *A, *B; };

// what the backward keeps of a row's forward: XWIN, SIG [R][16][32], E [R][16], MS, MA, HS, HT [R][32]
struct StampKeep { float *XWIN, *SIG, *E, *MS, *MA, *HS, *HT; };

// h_s * h_t of the position whose tile (rows outside the window zero) a wavefront holds in LDS, for lane d = lane & 31 (both halves hold it).
// vec: the wavefront's 80 floats -- [0, 32) m_s, then m_a; [32, 64) c; [64, 80) e.  kKeep: the backward's copy of row r.
template <bool kKeep>
__device__ __forceinline__ float stamp_forward(const cirs_stamp_weights& w, const StampLds& m, const float* tile, float* vec, int nw, int lane,
                                               const StampKeep& keep, long r, bool live) {
    const int d = lane & (tD - 1), half = lane >> 5, l = lane & 15, q = lane >> 4;
    float* vA = vec;
    float* vC = vec + tD;
    float* vE = vec + 2 * tD;
    const int first = sTile - nw;                          // the window's first tile row
    const float* mt = tile + (sTile - 1) * sXLd;           // m_t = x_p: the tile's last row
    // ---- m_s: the window's rows in ascending order, then one division (rows outside the window add an exact zero) ----
    float ms = 0.f;
#pragma unroll
    for (int t = 0; t < sTile; ++t) ms += t >= first ? tile[t * sXLd + d] : 0.f;
    ms = ms / (float)nw;
    vA[d] = ms;
    __builtin_amdgcn_wave_barrier();
    // ---- c = W2 m_t + W3 m_s + b_a: half 0 takes W2 m_t, half 1 W3 m_s ----
    {
        const float* mat = (half ? m.W3 : m.W2) + d * sLds;
        const float* v = half ? vA : mt;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mat[k], v[k], acc);
        acc += __shfl_xor(acc, 32, CIRS_WAVE);             // a + b == b + a: both halves hold the same bits
        vC[d] = acc + w.attn_b[d];
    }
    __builtin_amdgcn_wave_barrier();
    // ---- U = X_win W1^T, e_t = w0 . sigmoid(U_t + c) ----
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    stamp_product(tile, m.W1, l, q, acc0, acc1);
    const float c0 = vC[l], c1 = vC[16 + l], u0 = w.w0[l], u1 = w.w0[16 + l];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int t = 4 * q + rr;
        const float s0 = cell_sigmoid(acc0[rr] + c0), s1 = cell_sigmoid(acc1[rr] + c1);
        float e = stamp_row_sum(u0 * s0, u1 * s1);
        e = t >= first ? e : 0.f;                          // a row outside the window has no attention term
        if (l == 0) vE[t] = e;
        if (kKeep && live) {
            float* sg = keep.SIG + ((size_t)r * sTile + t) * tD;
            sg[l] = s0; sg[16 + l] = s1;
            if (l == 0) keep.E[(size_t)r * sTile + t] = e;
        }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- m_a = sum_t e_t x_t, t ascending ----
    float ma = 0.f;
#pragma unroll
    for (int t = 0; t < sTile; ++t) ma = __builtin_fmaf(vE[t], tile[t * sXLd + d], ma);
    vA[d] = ma;
    __builtin_amdgcn_wave_barrier();
    // ---- h_s = tanh(A m_a + b_A) in half 0, h_t = tanh(B m_t + b_B) in half 1 ----
    const float* mat = (half ? m.B : m.A) + d * sLds;
    const float* v = half ? mt : vA;
    float acc = half ? w.mlp_b_b[d] : w.mlp_a_b[d];
#pragma unroll
    for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mat[k], v[k], acc);
    const float th = tanhf(acc);
    if (kKeep && live) {
        (half ? keep.HT : keep.HS)[(size_t)r * tD + d] = th;
        (half ? keep.MA : keep.MS)[(size_t)r * tD + d] = half ? ma : ms;
    }
    __builtin_amdgcn_wave_barrier();
    return th * __shfl_xor(th, 32, CIRS_WAVE);
}

// (256, 4): four wavefronts per SIMD, what the LDS admits.  Left to itself the compiler takes 144 VGPRs (three per SIMD); capped it takes 125, still without
// scratch, and the step measured 12.2 us against 13.1 at C3
__global__ __launch_bounds__(256, 4) void stamp_step_kernel(cirs_stamp_cfg cfg, cirs_stamp_weights w, cirs_stamp_state st, const int32_t* __restrict__ users,
                                                         const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                         const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                         float* __restrict__ state_out, long state_stride, int walks) {
    __shared__ __attribute__((aligned(16))) float sW1[tD * sXLd];
    __shared__ __attribute__((aligned(16))) float sX[sEnvsPerWg * sTile * sXLd];
    __shared__ float sMat[4 * tD * sLds];                  // W2, W3, A, B: [row][33]
    __shared__ float sDec[tD * sLds];                      // [k][s]: decoder, transposed
    __shared__ float sIn[tD * sLds];                       // [d][c]: fnn_gate [32][33] (step) or ffn_user [32][32] (init), row-major
    __shared__ float sVec[sEnvsPerWg * 80];                // per wave: see stamp_forward; [0, 32) is the slot's input vector first, [32, 64) h last
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state, W = cfg.window;
    const bool is_init = users != nullptr;
    for (int q = threadIdx.x; q < S * tD; q += 256) sDec[(q & 31) * sLds + (q >> 5)] = w.dec_w[q];
    if (is_init) {                                         // position 0 is h_0 = x_0: no attention, nothing of it staged
        for (int q = threadIdx.x; q < tD * tD; q += 256) sIn[(q >> 5) * sLds + (q & 31)] = w.ffn_user_w[q];
    } else {
        for (int q = threadIdx.x; q < tD * (tD + 1); q += 256) sIn[q] = w.gate_w[q];
        stamp_stage_w1<false>(w.w1, sW1);
        stamp_stage33(w.w2, sMat);
        stamp_stage33(w.w3, sMat + tD * sLds);
        stamp_stage33(w.mlp_a_w, sMat + 2 * tD * sLds);
        stamp_stage33(w.mlp_b_w, sMat + 3 * tD * sLds);
    }
    __syncthreads();
    const StampLds mats{sW1, sMat, sMat + tD * sLds, sMat + 2 * tD * sLds, sMat + 3 * tD * sLds};
    const StampKeep none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float* vec = sVec + wv * 80;
    float* vin = vec;
    float* vh = vec + tD;
    float* tile = sX + wv * sTile * sXLd;
    const float* mrow = sIn + d * sLds;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long j = ((long)blockIdx.x * walks + it_w) * sEnvsPerWg + wv;
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
        const int nw = pos >= 1 ? std::min(W, pos) : 1;
        // ---- 1. the stored rows of the window (the n_p - 1 item slots before the new one): all requested at once, ahead of the slot's arithmetic.  A tile
        //         row in front of the window is NOT read, whether its slot is a live older one or lies before the first item: it is the zero row ----
        const float* xh = st.x_hist + hist + d;
        float wl[sTile / 2];
#pragma unroll
        for (int q = 0; q < sTile / 2; ++q) {
            const int t = 2 * q + half, k = pos - (sTile - 1) + t;
            wl[q] = (t >= sTile - nw && t < sTile - 1) ? xh[(size_t)k * tD] : 0.f;      // k >= pos - n_p + 1 >= 1
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
        for (int q = 0; q < sTile / 2; ++q) {
            const int t = 2 * q + half;
            tile[t * sXLd + d] = (pos >= 1 && t == sTile - 1) ? x : wl[q];
        }
        const float x0 = is_init ? x : (ok ? xh[0] : 0.f);
        if (ok && half == 0) st.x_hist[hist + (size_t)pos * tD + d] = x;
        __builtin_amdgcn_wave_barrier();
        // ---- 3. the attention pool and the read-out; h_0 = x_0 ----
        float h = x0;
        if (!is_init) h += stamp_forward<false>(w, mats, tile, vec, nw, lane, none, 0, false);
        vh[d] = h;
        __builtin_amdgcn_wave_barrier();
        // ---- 4. decoder ----
        if (d < S && half == 0) {
            float acc = w.dec_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(sDec[k * sLds + d], vh[k], acc);
            if (ok) state_out[(size_t)j * state_stride + d] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (ok && lane == 0) st.len[e] = pos + 1;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// (F) the forward of every buffer row again, one row per wavefront.  A row at position 0 keeps the values of the zero tile: the backward multiplies them by
// a zero gradient.
__global__ __launch_bounds__(256) void stamp_rows_fwd(cirs_stamp_cfg cfg, cirs_stamp_weights w, const float* __restrict__ x_hist,
                                                      const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t, int R, int walks,
                                                      float* __restrict__ H, StampKeep keep) {
    __shared__ __attribute__((aligned(16))) float sW1[tD * sXLd];
    __shared__ __attribute__((aligned(16))) float sX[sEnvsPerWg * sTile * sXLd];
    __shared__ float sMat[4 * tD * sLds];
    __shared__ float sVec[sEnvsPerWg * 80];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int L = cfg.max_len, W = cfg.window;
    stamp_stage_w1<false>(w.w1, sW1);
    stamp_stage33(w.w2, sMat);
    stamp_stage33(w.w3, sMat + tD * sLds);
    stamp_stage33(w.mlp_a_w, sMat + 2 * tD * sLds);
    stamp_stage33(w.mlp_b_w, sMat + 3 * tD * sLds);
    __syncthreads();
    const StampLds mats{sW1, sMat, sMat + tD * sLds, sMat + 2 * tD * sLds, sMat + 3 * tD * sLds};
    float* tile = sX + wv * sTile * sXLd;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long r = ((long)blockIdx.x * walks + it_w) * sEnvsPerWg + wv;
        const bool live = r < R;
        const long rr = live ? r : 0;
        const int p = row_t[rr];
        const int nw = p >= 1 ? std::min(W, p) : 1;
        const float* xh = x_hist + (size_t)row_env[rr] * L * tD + d;
        float wl[sTile / 2];
#pragma unroll
        for (int q = 0; q < sTile / 2; ++q) {      // all requested at once; the window's rows only
            const int t = 2 * q + half, k = p - (sTile - 1) + t;
            wl[q] = (p >= 1 && t >= sTile - nw) ? xh[(size_t)k * tD] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < sTile / 2; ++q) {
            const int t = 2 * q + half;
            tile[t * sXLd + d] = wl[q];
            if (live) keep.XWIN[((size_t)r * sTile + t) * tD + d] = wl[q];
        }
        __builtin_amdgcn_wave_barrier();
        const float prod = stamp_forward<true>(w, mats, tile, sVec + wv * 80, nw, lane, keep, rr, live);
        if (live && half == 0) H[(size_t)r * tD + d] = xh[0] + (p >= 1 ? prod : 0.f);
        __builtin_amdgcn_wave_barrier();
    }
}

// (B) one row per wavefront.  Vectors live in the lane = dimension layout (d = lane & 31, a job per half), tiles in the layout of the forward's accumulators
// (lane (l, q): rows 4 q .. 4 q + 3, columns l and 16 + l).
struct StampBwdOut { float *DPA, *DPB, *DC, *DE, *DG, *DWIN; };
__global__ __launch_bounds__(256) void stamp_rows_bwd(cirs_stamp_cfg cfg, cirs_stamp_weights w, int R, int walks, const int32_t* __restrict__ row_t,
                                                      const float* __restrict__ dH, StampKeep keep, StampBwdOut out) {
    __shared__ __attribute__((aligned(16))) float sW1T[tD * sXLd];
    __shared__ __attribute__((aligned(16))) float sDg[sEnvsPerWg * sTile * sXLd];
    __shared__ float sMat[4 * tD * sLds];                  // W2, W3, A, B: [row][33], read down their columns here
    __shared__ float sVec[sEnvsPerWg * 224];               // per wave: [0, 64) dpa | dpb; [64, 128) dm_a | dm_t; [128, 160) dc; [160, 224) slot p's | every slot's
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5, l = lane & 15, q = lane >> 4;
    const int W = cfg.window;
    stamp_stage_w1<true>(w.w1, sW1T);
    stamp_stage33(w.w2, sMat);
    stamp_stage33(w.w3, sMat + tD * sLds);
    stamp_stage33(w.mlp_a_w, sMat + 2 * tD * sLds);
    stamp_stage33(w.mlp_b_w, sMat + 3 * tD * sLds);
    __syncthreads();
    float* dgb = sDg + wv * sTile * sXLd;
    float* vG = sVec + wv * 224;
    float* vM = vG + 64;
    float* vC = vG + 128;
    float* vL = vG + 160;
    const float u0 = w.w0[l], u1 = w.w0[16 + l];
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long r = ((long)blockIdx.x * walks + it_w) * sEnvsPerWg + wv;
        if (r >= R) continue;                              // wave-uniform; only wave barriers below
        const int p = row_t[r];
        const int nw = p >= 1 ? std::min(W, p) : 1;
        const int first = p >= 1 ? sTile - nw : sTile;     // position 0 has no window: every gradient below is zero
        // ---- the product and the two tanh: half 0 -> dpa = dh h_t (1 - h_s^2), half 1 -> dpb = dh h_s (1 - h_t^2) ----
        const float dh = p >= 1 ? dH[(size_t)r * tD + d] : 0.f;
        const float hs = keep.HS[(size_t)r * tD + d], ht = keep.HT[(size_t)r * tD + d];
        const float mine = half ? ht : hs, other = half ? hs : ht;
        const float g = dh * other * (1.0f - mine * mine);
        (half ? out.DPB : out.DPA)[(size_t)r * tD + d] = g;
        vG[half * tD + d] = g;
        __builtin_amdgcn_wave_barrier();
        // ---- dm_a = A^T dpa (half 0), dm_t = B^T dpb (half 1) ----
        {
            const float* mat = sMat + (2 + half) * tD * sLds + d;
            const float* v = vG + half * tD;
            float acc = 0.f;
#pragma unroll
            for (int o = 0; o < tD; ++o) acc = __builtin_fmaf(mat[o * sLds], v[o], acc);
            vM[half * tD + d] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- de_t = x_t . dm_a;  dG_t = de_t w0 * s_t (1 - s_t), rows of the window only ----
        const float a0 = vM[l], a1 = vM[16 + l];
        float ev[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int t = 4 * q + rr;
            const size_t row = (size_t)r * sTile + t;
            const bool in = t >= first;
            const float x0 = keep.XWIN[row * tD + l], x1 = keep.XWIN[row * tD + 16 + l];
            const float s0 = keep.SIG[row * tD + l], s1 = keep.SIG[row * tD + 16 + l];
            ev[rr] = keep.E[row];
            float de = stamp_row_sum(x0 * a0, x1 * a1);
            de = in ? de : 0.f;
            const float g0 = de * u0 * s0 * (1.0f - s0), g1 = de * u1 * s1 * (1.0f - s1);
            dgb[t * sXLd + l] = g0; dgb[t * sXLd + 16 + l] = g1;
            out.DG[row * tD + l] = g0; out.DG[row * tD + 16 + l] = g1;
            if (l == 0) out.DE[row] = de;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- dX_win = dG W1 (the forward's product on the transposed weights);  dc = sum_t dG_t, t ascending ----
        f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
        stamp_product(dgb, sW1T, l, q, acc0, acc1);
        float dc = 0.f;
#pragma unroll
        for (int t = 0; t < sTile; ++t) dc += dgb[t * sXLd + d];
        if (half == 0) out.DC[(size_t)r * tD + d] = dc;
        vC[d] = dc;
        __builtin_amdgcn_wave_barrier();
        // ---- c's inputs: W2^T dc + dm_t into slot p (half 0), W3^T dc / n_p into every window slot (half 1) ----
        {
            const float* mat = sMat + half * tD * sLds + d;
            float acc = 0.f;
#pragma unroll
            for (int o = 0; o < tD; ++o) acc = __builtin_fmaf(mat[o * sLds], vC[o], acc);
            vL[half * tD + d] = half ? acc / (float)nw : acc + vM[tD + d];
        }
        __builtin_amdgcn_wave_barrier();
        // ---- the gradient per tile row: e_t dm_a + (dG W1)_t + W3^T dc / n_p, and slot p's own terms in row 15 ----
        const float p0 = vL[l], p1 = vL[16 + l], w30 = vL[tD + l], w31 = vL[tD + 16 + l];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int t = 4 * q + rr;
            const bool in = t >= first, own = t == sTile - 1;
            const float o0 = __builtin_fmaf(ev[rr], a0, acc0[rr]) + w30 + (own ? p0 : 0.f);
            const float o1 = __builtin_fmaf(ev[rr], a1, acc1[rr]) + w31 + (own ? p1 : 0.f);
            float* dw = out.DWIN + ((size_t)r * sTile + t) * tD;
            dw[l] = in ? o0 : 0.f; dw[16 + l] = in ? o1 : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// (X) dX from the rows' tile gradients.  Row (b, 0) collects dH of every position of its env, row (b, k >= 1) tile row k - p + 15 of every position p whose
// window holds slot k; p ascending.  No carry between rows: 32 lanes per row, 8 rows per workgroup.
__global__ __launch_bounds__(256) void stamp_window_bwd(const float* __restrict__ dH, const float* __restrict__ DWIN, const int32_t* __restrict__ row_env,
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
        for (int p = k; p <= last; ++p) acc += DWIN[((base + p) * sTile + (k - p + sTile - 1)) * tD + d];
    }
    dX[(size_t)r * tD + d] = acc;
}

struct StampScratch : SlotScratch {
    float *G, *H, *dH, *dX, *XWIN, *SIG, *DG, *DWIN, *E, *DE, *MS, *MA, *HS, *HT, *DPA, *DPB, *DC;
};

// the pass's list: decoder (S <= 32), ffn_user, gate, attn.w1, attn.w2 (+ attn.bias), attn.w3, mlp_a, mlp_b, attn.w0 -- nine problems
static size_t stamp_partial_floats(long R) {
    return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1) + 5 * dw_list_floats(R, tD, tD) + dw_list_floats(R, 1, tD);
}

static StampScratch carve_stamp(void* ws, const cirs_stamp_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    StampScratch s;
    s.G = c.take((size_t)R * 32); s.H = c.take((size_t)R * tD); s.dH = c.take((size_t)R * tD); s.dX = c.take((size_t)R * tD);
    s.XWIN = c.take((size_t)R * sTile * tD); s.SIG = c.take((size_t)R * sTile * tD); s.DG = c.take((size_t)R * sTile * tD); s.DWIN = c.take((size_t)R * sTile * tD);
    s.E = c.take((size_t)R * sTile); s.DE = c.take((size_t)R * sTile);
    s.MS = c.take((size_t)R * tD); s.MA = c.take((size_t)R * tD); s.HS = c.take((size_t)R * tD); s.HT = c.take((size_t)R * tD);
    s.DPA = c.take((size_t)R * tD); s.DPB = c.take((size_t)R * tD); s.DC = c.take((size_t)R * tD);
    carve_slots(c, s, R, cfg->n_env, stamp_partial_floats(R));
    *total_floats = c.total();
    return s;
}

// the cfg first and on its own: a cfg outside the fixed sizes is refused before any pointer is read
static int validate_stamp_cfg(const cirs_stamp_cfg* cfg) {
    CIRS_REQUIRE(cfg, "stamp tracker: cfg null");
    CIRS_REQUIRE(cfg->window >= 1 && cfg->window <= sTile, "stamp tracker: window must be in 1..16");
    return validate_slot_cfg(cfg, "stamp tracker");
}

static int validate_stamp(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w) {
    if (int rc = validate_stamp_cfg(cfg)) return rc;
    CIRS_REQUIRE(w, "stamp tracker: weights null");
    if (int rc = validate_slot_weights(w, "stamp tracker")) return rc;
    CIRS_REQUIRE(w->w1 && w->w2 && w->w3 && w->attn_b && w->w0, "stamp tracker: attention weight pointer null (w1 / w2 / w3 / attn_b / w0)");
    CIRS_REQUIRE(w->mlp_a_w && w->mlp_a_b && w->mlp_b_w && w->mlp_b_b, "stamp tracker: read-out weight pointer null (mlp_a / mlp_b)");
    return CIRS_OK;
}

static int launch_stamp_step(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w, cirs_stamp_state* st, const int32_t* users, const int64_t* items,
                             const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_REQUIRE(st && st->x_hist && st->len, "stamp tracker: state pointer null");
    // 40 448 bytes of LDS (30 KB of it the seven staged matrices): four workgroups per CU, four wavefronts per SIMD.  Up to 4 x 4 x CUs envs every env has a
    // wavefront of its own, beyond that a workgroup walks several groups of four and what it staged serves them all.  Chosen from the structure, not tuned.
    const int walks = slot_walks(n, sEnvsPerWg, sWgPerCu);
    hipLaunchKernelGGL(stamp_step_kernel, dim3(cdiv(n, (long)sEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n,
                       state_out, state_stride, walks);
    CIRS_CHECK_LAUNCH("stamp_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_stamp_tracker_init(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w, cirs_stamp_state* st, const int32_t* users,
                                       const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_stamp, cirs::launch_stamp_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_stamp_tracker_step(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w, cirs_stamp_state* st, const int64_t* items,
                                       const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                                       int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_stamp, cirs::launch_stamp_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_stamp_tracker_backward_workspace_bytes(const cirs_stamp_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_stamp_cfg, cirs::carve_stamp, cfg, n_rows);
}

extern "C" int cirs_stamp_tracker_backward(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w, const cirs_stamp_state* st, const int32_t* users,
                                           const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                           const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_stamp_grads* grads, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_stamp(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_slot_grads(grads, "stamp tracker")) return rc;
    CIRS_REQUIRE(grads->w1 && grads->w2 && grads->w3 && grads->attn_b && grads->w0 && grads->mlp_a_w && grads->mlp_a_b && grads->mlp_b_w && grads->mlp_b_b,
                 "stamp tracker: attention / read-out gradient pointer null");
    CIRS_REQUIRE((long)n_rows * sTile < (1L << 27), "stamp tracker: n_rows * 16 out of range");
    CIRS_REQUIRE(workspace_bytes >= cirs_stamp_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, W = cfg->window;
    size_t total = 0;
    StampScratch sc = carve_stamp(workspace, cfg, R, &total);
    DwList dwl{};
    const StampKeep keep{sc.XWIN, sc.SIG, sc.E, sc.MS, sc.MA, sc.HS, sc.HT};
    hipLaunchKernelGGL(gather_dstate, dim3(cdiv((long)R * S, 256)), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    const int walks = slot_walks(R, sEnvsPerWg, sWgPerCu);
    hipLaunchKernelGGL(stamp_rows_fwd, dim3(cdiv(R, (long)sEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, (const float*)st->x_hist, row_env, row_t, R, walks,
                       sc.H, keep);
    launch_rows_gemm_dw(dwl, sc.H, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0, sc.dH,
                        tD, s);
    hipLaunchKernelGGL(stamp_rows_bwd, dim3(cdiv(R, (long)sEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, R, walks, row_t, (const float*)sc.dH, keep,
                       StampBwdOut{sc.DPA, sc.DPB, sc.DC, sc.DE, sc.DG, sc.DWIN});
    CIRS_CHECK_LAUNCH("stamp tracker backward rows");
    {   // over the R 16 (row, tile row) pairs, in the slab count of the pass: attn.w1 = DG^T XWIN, attn.w0 = DE^T SIG (DE is zero outside the window)
        DwBatch bt{};
        dw_batch_add(bt, dwl, sc.DG, tD, sc.XWIN, tD, R, tD, tD, grads->w1, nullptr, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.DE, 1, sc.SIG, tD, R, 1, tD, grads->w0, nullptr, 0, sc.partial);
        dw_batch_launch(bt, R, s, R * sTile);
    }
    {   // per row: m_t is the tile's last row; attn.bias = the column sums of DC
        const float* MT = sc.XWIN + (size_t)(sTile - 1) * tD;
        DwBatch bt{};
        dw_batch_add(bt, dwl, sc.DC, tD, MT, sTile * tD, R, tD, tD, grads->w2, grads->attn_b, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.DC, tD, sc.MS, tD, R, tD, tD, grads->w3, nullptr, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.DPA, tD, sc.MA, tD, R, tD, tD, grads->mlp_a_w, grads->mlp_a_b, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.DPB, tD, MT, sTile * tD, R, tD, tD, grads->mlp_b_w, grads->mlp_b_b, 0, sc.partial);
        dw_batch_launch(bt, R, s);
    }
    hipLaunchKernelGGL(stamp_window_bwd, dim3(cdiv(R, 8)), dim3(256), 0, s, (const float*)sc.dH, (const float*)sc.DWIN, row_env, row_t, offsets, lens, R, W,
                       sc.dX);
    CIRS_CHECK_LAUNCH("stamp tracker backward window");
    return slots_backward(cfg, w, grads, sc.dX, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
