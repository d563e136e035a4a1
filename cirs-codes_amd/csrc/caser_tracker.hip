// caser_tracker.hip -- StateTrackerCaser for gfx950: the convolutional window tracker (horizontal filters max-pooled over time + one vertical filter).
//
// The reference has no counterpart; the model is defined here, in include/cirs_hip.h and in DESIGN.md 7.5:
//   inputs    the other trackers' slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k -- no sqrt(D) scale, no positional encoding
//   window    win_p[j] = x_{p-W+1+j} if p-W+1+j >= 1, else the zero row (j = 0..W-1); x_0 is never in it, position 0 has an all-zero window
//   banks     c_{i,f,t} = bh_i[f] + sum_{j<h_i} sum_d Wh_i[f,j,d] win_p[t+j,d] (t = 0..W-h_i);  o_{i,f} = relu(max_t c_{i,f,t}), arg-max = the first maximal t
//   vertical  v_d = relu(bv + sum_j wv[j] win_p[j,d])
//   fc        z = relu(fc([o_0 | o_1 | ... | v]));  h_p = x_0 + z;  s_p = decoder(h_p)
// Step (one launch appends one position for n envs): ONE env per wavefront, four per workgroup.  A workgroup stages the banks [f][32 h + 4], fc [d][KC + 1],
// the decoder [k][33] and the slot's matrix [d][33] in LDS once, a wavefront its window [W][36].  A bank over a window is one 16 x 16 tile of
// v_mfma_f32_16x16x4_f32 (positions x filters, K = 32 h): measured against plain FMAs at C3, 16.6 against 20.0 us per step.  The vertical
// filter, fc and the decoder are plain FMAs.  Everything per env is predicated, not branched.
//
// Backward (rows = (env b, position p < len_b), env-major; no sequential pass):
//   F  caser_rows_fwd: the forward of every row again from the stored slots -> the window WIN, the concatenation CAT, the arg-max ARG, z, h
//   C  G = gather(dstate); dH = G W_dec and the decoder's weight gradient in one launch (rows_gemm + dw_gemm, as the other trackers' stage C)
//   B  caser_rows_bwd: dZ = dH [z > 0]; dCAT = dZ fc_w; dO = dCAT [o > 0] routed to its arg-max position (DC, zero elsewhere); dV = dCAT [v > 0];
//      per row the vertical filter's terms sum_d dV[d] win[j,d] and sum_d dV[d] (d ascending)
//   W  weight gradients through the slab partials: fc (dZ, CAT), the vertical filter (column sums of the per-row terms), bank i as the product of
//      DC_i [R W, 16] and the patches of WIN [R W, 32 h_i] (patch t = rows t .. t + h_i - 1 of a window, contiguous)
//   X  caser_window_bwd: dX[b,0] = sum_p dH[b,p];  dX[b,k] = sum_{p=k}^{min(len_b-1, k+W-1)} dWin_p[k-p+W-1]  -- p ascending, every row on its own, with
//      dWin_p[j] = wv[j] dV_p + sum_i sum_f [0 <= j - arg < h_i] dO_p[i,f] Wh_i[f, j - arg]  (i, f ascending)
//   E  the slot stage of the recurrent trackers (slot_tracker.h)
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include "slot_tracker.h"

namespace cirs {

constexpr int cF = CIRS_CASER_FILTERS;                     // filters per bank: 16
constexpr int cMaxW = CIRS_CASER_MAX_WINDOW;               // 16
constexpr int cMaxNh = CIRS_CASER_MAX_HEIGHTS;             // 4 banks, heights <= 4
constexpr int cWinRows = cMaxW + 4;                        // rows t + j of a lane whose t lies past the last position are read and discarded
constexpr int cWinLd = tD + 4;                             // LDS stride of a window row: 36 (16-byte aligned rows, row starts spread over the banks)
constexpr int cMaxCat = cF * cMaxNh + tD;                  // 96
constexpr int cConvFloats = cF * (36 + 68 + 100 + 132);    // the four banks at stride 32 h + 4
constexpr int cFcFloats = tD * (cMaxCat + 1);
constexpr int cLds = tD + 1;                               // LDS stride of a staged 32-row matrix, as in avg_tracker.hip
constexpr int cEnvsPerWg = 4;                              // one env (or buffer row) per wavefront
constexpr int cWgPerCu = 2;                                // 54 KB of LDS per workgroup: two fit in a CU's 160 KB

// x / m for the small run-time divisors of the staging (heights 1..4, fc rows of 3..6 sixteenths): constant divisions, no division routine
__device__ __forceinline__ int caser_div(int x, int m) {
    switch (m) {
        case 1: return x;
        case 2: return x >> 1;
        case 3: return x / 3;
        case 4: return x >> 2;
        case 5: return x / 5;
        default: return x / 6;
    }
}

// the banks [f][32 h + 4] one after the other (rows 16-byte aligned for the ds_read_b128 of the MFMA operands) and fc [d][KC + 1], once per workgroup:
// coalesced dword reads of the row-major tensors (the tensors are views of one flat buffer: no alignment beyond a float's).  Fixed trip counts, predicated:
// a thread's loads (up to 44) are all issued before its first LDS store, one round trip to the L2 instead of one per pass.
__device__ __forceinline__ void caser_stage(const cirs_caser_cfg& cfg, const cirs_caser_weights& w, float* sConv, float* sFc) {
    const int KC = cF * cfg.n_heights + tD;
    float vc[cMaxNh][8], vf[12];
#pragma unroll
    for (int i = 0; i < cMaxNh; ++i) {
        const int n = i < cfg.n_heights ? cF * cfg.heights[i] * tD : 0;
        const float* src = w.conv_w[i];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = threadIdx.x + 256 * u;
            vc[i][u] = q < n ? src[q] : 0.f;
        }
    }
#pragma unroll
    for (int u = 0; u < 12; ++u) {
        const int q = threadIdx.x + 256 * u;
        vf[u] = q < tD * KC ? w.fc_w[q] : 0.f;
    }
    int off = 0;
#pragma unroll
    for (int i = 0; i < cMaxNh; ++i) {
        if (i < cfg.n_heights) {
            const int h = cfg.heights[i], K = h * tD;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = threadIdx.x + 256 * u, f = caser_div(q >> 5, h);      // q = (f h + j) 32 + c
                if (q < cF * K) sConv[off + f * (K + 4) + (q - f * K)] = vc[i][u];
            }
            off += cF * (K + 4);
        }
    }
#pragma unroll
    for (int u = 0; u < 12; ++u) {
        const int q = threadIdx.x + 256 * u, dd = caser_div(q >> 4, KC >> 4);      // q = d KC + k, KC a multiple of 16
        if (q < tD * KC) sFc[dd * (KC + 1) + (q - dd * KC)] = vf[u];
    }
}

// window -> concatenation, one wavefront.  win: [cWinRows][cWinLd], rows 0 .. W-1 set; cat: [KC]; arg (kArg): [16 n_heights] the first maximal t of every filter.
// A bank is D[t][f] = bias[f] + sum_k A[t][k] B[k][f] on v_mfma_f32_16x16x4_f32 with A[t][32 j + d] = win[t + j][d] and B[k][f] = Wh[f][k]: lane (l = lane & 15,
// q = lane >> 4) supplies row t = l of A and column f = l of B; of a block of 16 contraction indices it holds 4 q .. 4 q + 3 (one ds_read_b128 each), MFMA i of
// the block contracts {i, 4 + i, 8 + i, 12 + i}: a fixed order.  It receives D[4 q + r][l], r = 0..3.  Rows t > W - h of A are rows of other patches or stale:
// they reach only their own rows of D, which the pooling leaves out.
template <bool kArg>
__device__ __forceinline__ void caser_features(const cirs_caser_cfg& cfg, const cirs_caser_weights& w, const float* sConv, const float* win, float* cat,
                                               int* arg, int lane) {
    const int W = cfg.window, l = lane & (cF - 1), q = lane >> 4;
    int off = 0;
    for (int i = 0; i < cfg.n_heights; ++i) {
        const int h = cfg.heights[i], K = h * tD, nT = W - h + 1;
        const float* wr = sConv + off + l * (K + 4) + 4 * q;
        const float b = w.conv_b[i][l];
        f32x4 acc = f32x4{b, b, b, b};
        for (int j = 0; j < h; ++j) {
            const float* ar = win + (l + j) * cWinLd + 4 * q;
#pragma unroll
            for (int kk = 0; kk < tD; kk += 16) {
                const float4 a = *reinterpret_cast<const float4*>(ar + kk);
                const float4 bw = *reinterpret_cast<const float4*>(wr + j * tD + kk);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bw.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bw.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bw.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bw.w, acc, 0, 0, 0);
            }
        }
        // the lane's positions 4 q .. 4 q + 3 in ascending t (a later one wins only if larger), then the filter's four lanes: larger value, ties to the smaller t
        float m = -INFINITY;
        int at = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (4 * q + r < nT && acc[r] > m) { m = acc[r]; at = 4 * q + r; }
        }
#pragma unroll
        for (int sft = 16; sft <= 32; sft <<= 1) {
            const float om = __shfl_xor(m, sft, CIRS_WAVE);
            const int ot = __shfl_xor(at, sft, CIRS_WAVE);
            if (om > m || (om == m && ot < at)) { m = om; at = ot; }
        }
        if (q == 0) {
            cat[i * cF + l] = fmaxf(m, 0.f);
            if (kArg) arg[i * cF + l] = at;
        }
        off += cF * (K + 4);
    }
    if (lane < tD) {
        float v = w.vert_b[0];
        for (int j = 0; j < W; ++j) v = __builtin_fmaf(w.vert_w[j], win[j * cWinLd + lane], v);
        cat[cF * cfg.n_heights + lane] = fmaxf(v, 0.f);
    }
    __builtin_amdgcn_wave_barrier();
}

// z_d = relu(fc_b[d] + sum_k fc[d,k] cat[k]): the two halves of the wavefront take one half of k each (ascending), lower half + upper half; every lane returns z_d
__device__ __forceinline__ float caser_fc(const cirs_caser_cfg& cfg, const cirs_caser_weights& w, const float* sFc, const float* cat, int lane) {
    const int KC = cF * cfg.n_heights + tD, d = lane & (tD - 1), half = lane >> 5, k0 = half * (KC >> 1);
    const float* fr = sFc + d * (KC + 1) + k0;
    float acc = half ? 0.f : w.fc_b[d];
#pragma unroll 8
    for (int k = 0; k < (KC >> 1); ++k) acc = __builtin_fmaf(fr[k], cat[k0 + k], acc);
    const float other = __shfl_xor(acc, 32, CIRS_WAVE);
    return fmaxf(half ? other + acc : acc + other, 0.f);
}

__global__ __launch_bounds__(256) void caser_step_kernel(cirs_caser_cfg cfg, cirs_caser_weights w, cirs_caser_state st, const int32_t* __restrict__ users,
                                                         const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                         const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                         float* __restrict__ state_out, long state_stride, int walks) {
    __shared__ __attribute__((aligned(16))) float sConv[cConvFloats];
    __shared__ float sFc[cFcFloats];
    __shared__ float sDec[tD * cLds];                      // [k][s]: decoder, transposed
    __shared__ float sIn[tD * cLds];                       // [d][c]: fnn_gate [32][33] (step) or ffn_user [32][32] (init), row-major
    __shared__ __attribute__((aligned(16))) float sWin[cEnvsPerWg * cWinRows * cWinLd];
    __shared__ float sCat[cEnvsPerWg * cMaxCat];
    __shared__ float sVec[cEnvsPerWg * 2 * tD];            // per wave: [0, 32) the slot's input vector, [32, 64) h
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state, W = cfg.window;
    const bool is_init = users != nullptr;
    caser_stage(cfg, w, sConv, sFc);
    for (int q = threadIdx.x; q < cEnvsPerWg * cWinRows * cWinLd; q += 256) sWin[q] = 0.f;      // rows past W are read (and left out): keep them finite
    for (int q = threadIdx.x; q < S * tD; q += 256) sDec[(q & 31) * cLds + (q >> 5)] = w.dec_w[q];
    if (is_init) {
        for (int q = threadIdx.x; q < tD * tD; q += 256) sIn[(q >> 5) * cLds + (q & 31)] = w.ffn_user_w[q];
    } else {
        for (int q = threadIdx.x; q < tD * (tD + 1); q += 256) sIn[q] = w.gate_w[q];
    }
    __syncthreads();
    float* vin = sVec + wv * 2 * tD;
    float* vh = vin + tD;
    float* win = sWin + wv * cWinRows * cWinLd;
    float* cat = sCat + wv * cMaxCat;
    const float* mrow = sIn + d * cLds;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long j = ((long)blockIdx.x * walks + it_w) * cEnvsPerWg + wv;
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
        // ---- 1. the stored rows of the window (the last W item slots, zero rows in front): all requested at once, ahead of the slot's arithmetic ----
        const float* xh = st.x_hist + hist + d;
        float wl[cMaxW / 2];
#pragma unroll
        for (int q = 0; q < cMaxW / 2; ++q) {
            const int k = pos - W + 1 + 2 * q + half;
            wl[q] = (2 * q + half < W && k >= 1 && k < pos) ? xh[(size_t)k * tD] : 0.f;
        }
        // ---- 2. the new input slot (both halves of the wavefront hold it); it is the window's last row (pos >= 1) ----
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
        for (int q = 0; q < cMaxW / 2; ++q) {
            const int jw = 2 * q + half;
            if (jw < W) win[jw * cWinLd + d] = (pos >= 1 && jw == W - 1) ? x : wl[q];
        }
        const float x0 = is_init ? x : (ok ? xh[0] : 0.f);
        if (ok && half == 0) st.x_hist[hist + (size_t)pos * tD + d] = x;
        __builtin_amdgcn_wave_barrier();
        // ---- 3. banks, vertical filter, fc ----
        caser_features<false>(cfg, w, sConv, win, cat, nullptr, lane);
        vh[d] = x0 + caser_fc(cfg, w, sFc, cat, lane);
        __builtin_amdgcn_wave_barrier();
        // ---- 4. decoder ----
        if (d < S && half == 0) {
            float acc = w.dec_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(sDec[k * cLds + d], vh[k], acc);
            if (ok) state_out[(size_t)j * state_stride + d] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (ok && lane == 0) st.len[e] = pos + 1;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// (F) the forward of every buffer row again, one row per wavefront.  WIN is followed by three zero rows: the last patches of the bank problems read past
// the last window (their DC rows are zero, the product needs finite values there).
__global__ __launch_bounds__(256) void caser_rows_fwd(cirs_caser_cfg cfg, cirs_caser_weights w, const float* __restrict__ x_hist,
                                                      const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t, int R, int walks,
                                                      float* __restrict__ H, float* __restrict__ Z, float* __restrict__ CAT, int32_t* __restrict__ ARG,
                                                      float* __restrict__ WIN, float* __restrict__ ONES) {
    __shared__ __attribute__((aligned(16))) float sConv[cConvFloats];
    __shared__ float sFc[cFcFloats];
    __shared__ __attribute__((aligned(16))) float sWin[cEnvsPerWg * cWinRows * cWinLd];
    __shared__ float sCat[cEnvsPerWg * cMaxCat];
    __shared__ int sArg[cEnvsPerWg * cF * cMaxNh];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int L = cfg.max_len, W = cfg.window, nF = cF * cfg.n_heights, KC = nF + tD;
    caser_stage(cfg, w, sConv, sFc);
    for (int q = threadIdx.x; q < cEnvsPerWg * cWinRows * cWinLd; q += 256) sWin[q] = 0.f;
    if (blockIdx.x == 0 && threadIdx.x < 3 * tD) WIN[(size_t)R * W * tD + threadIdx.x] = 0.f;
    __syncthreads();
    float* win = sWin + wv * cWinRows * cWinLd;
    float* cat = sCat + wv * cMaxCat;
    int* arg = sArg + wv * cF * cMaxNh;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long r = ((long)blockIdx.x * walks + it_w) * cEnvsPerWg + wv;
        const bool live = r < R;
        const long rr = live ? r : 0;
        const int p = row_t[rr];
        const float* xh = x_hist + (size_t)row_env[rr] * L * tD + d;
        float wl[cMaxW / 2];
#pragma unroll
        for (int q = 0; q < cMaxW / 2; ++q) {      // all requested at once
            const int k = p - W + 1 + 2 * q + half;
            wl[q] = (2 * q + half < W && k >= 1) ? xh[(size_t)k * tD] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < cMaxW / 2; ++q) {
            const int jw = 2 * q + half;
            if (jw < W) {
                win[jw * cWinLd + d] = wl[q];
                if (live) WIN[((size_t)r * W + jw) * tD + d] = wl[q];
            }
        }
        __builtin_amdgcn_wave_barrier();
        caser_features<true>(cfg, w, sConv, win, cat, arg, lane);
        const float z = caser_fc(cfg, w, sFc, cat, lane);
        if (live) {
            for (int k = lane; k < KC; k += 64) CAT[(size_t)r * KC + k] = cat[k];
            if (lane < nF) ARG[(size_t)r * nF + lane] = arg[lane];
            if (half == 0) {
                Z[(size_t)r * tD + d] = z;
                H[(size_t)r * tD + d] = xh[0] + z;
            }
            if (lane == 0) ONES[r] = 1.f;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// (B) one row per wavefront: through fc, the ReLUs and the pooling.  DC holds bank i at DC + i * R * W * 16 as [R W, 16].  VW [R, W + 1]: the vertical filter's
// per-row terms, column W the bias'.
__global__ __launch_bounds__(256) void caser_rows_bwd(cirs_caser_cfg cfg, cirs_caser_weights w, int R, const float* __restrict__ dH,
                                                      const float* __restrict__ Z, const float* __restrict__ CAT, const int32_t* __restrict__ ARG,
                                                      const float* __restrict__ WIN, float* __restrict__ DZ, float* __restrict__ DO, float* __restrict__ DVP,
                                                      float* __restrict__ DC, float* __restrict__ VW) {
    __shared__ float sDv[cEnvsPerWg * tD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long r = blockIdx.x * (long)cEnvsPerWg + wv;
    if (r >= R) return;
    const int d = lane & (tD - 1);
    const int W = cfg.window, nF = cF * cfg.n_heights, KC = nF + tD;
    const float dz = Z[(size_t)r * tD + d] > 0.f ? dH[(size_t)r * tD + d] : 0.f;
    if (lane < tD) DZ[(size_t)r * tD + d] = dz;
    float* dv = sDv + wv * tD;
    for (int k = lane; k < KC; k += 64) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < tD; ++o) acc = __builtin_fmaf(lane_bcast(dz, o), w.fc_w[(size_t)o * KC + k], acc);
        const float dc = CAT[(size_t)r * KC + k] > 0.f ? acc : 0.f;
        if (k < nF) {
            DO[(size_t)r * nF + k] = dc;
            const int a = ARG[(size_t)r * nF + k];
            float* dcb = DC + ((size_t)(k >> 4) * R * W + (size_t)r * W) * cF + (k & (cF - 1));
            for (int t = 0; t < W; ++t) dcb[(size_t)t * cF] = t == a ? dc : 0.f;
        } else {
            DVP[(size_t)r * tD + k - nF] = dc;
            dv[k - nF] = dc;
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane <= W) {
        float acc = 0.f;
        if (lane < W) {
            const float* wr = WIN + ((size_t)r * W + lane) * tD;
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(dv[k], wr[k], acc);
        } else {
            for (int k = 0; k < tD; ++k) acc += dv[k];
        }
        VW[(size_t)r * (W + 1) + lane] = acc;
    }
}

// (X) dX from the rows' window gradients.  Row (b, 0) collects dH of every position of its env, row (b, k >= 1) row k - p + W - 1 of the window gradient of every
// position p whose window holds slot k; p ascending.  No carry between rows: 32 lanes per row, 8 rows per workgroup.
__global__ __launch_bounds__(256) void caser_window_bwd(cirs_caser_cfg cfg, cirs_caser_weights w, const float* __restrict__ dH, const float* __restrict__ DO,
                                                        const float* __restrict__ DVP, const int32_t* __restrict__ ARG, const int32_t* __restrict__ row_env,
                                                        const int32_t* __restrict__ row_t, const int32_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ lens, int R, float* __restrict__ dX) {
    const long r = blockIdx.x * 8L + (threadIdx.x >> 5);
    if (r >= R) return;
    const int d = threadIdx.x & 31, b = row_env[r], k = row_t[r], len = lens[b];
    const int W = cfg.window, nF = cF * cfg.n_heights;
    const size_t base = (size_t)offsets[b];
    float acc = 0.f;
    if (k == 0) {
#pragma unroll 4
        for (int p = 0; p < len; ++p) acc += dH[(base + p) * tD + d];
    } else {
        const int last = (int)std::min<long>(len - 1, (long)k + W - 1);
        for (int p = k; p <= last; ++p) {
            const size_t rp = base + p;
            const int j = k - p + W - 1;
            float t = w.vert_w[j] * DVP[rp * tD + d];
            for (int i = 0; i < cfg.n_heights; ++i) {
                const int h = cfg.heights[i];
                const float* wi = w.conv_w[i] + d;
                const int32_t* ar = ARG + rp * nF + i * cF;
                const float* go = DO + rp * nF + i * cF;
                for (int f = 0; f < cF; ++f) {
                    const int jj = j - ar[f];
                    if (jj >= 0 && jj < h) t = __builtin_fmaf(go[f], wi[(size_t)(f * h + jj) * tD], t);
                }
            }
            acc += t;
        }
    }
    dX[(size_t)r * tD + d] = acc;
}

struct CaserScratch : SlotScratch {
    float *G, *H, *Z, *dH, *dX, *DZ, *CAT, *DO, *DVP, *VW, *ONES, *WIN, *DC;
    int32_t* ARG;
};

static size_t caser_partial_floats(const cirs_caser_cfg* cfg, long R) {
    size_t f = dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1);       // decoder (S <= 32), ffn_user, gate
    f += dw_list_floats(R, tD, cF * cfg->n_heights + tD) + dw_list_floats(R, cfg->window, 1) + dw_list_floats(R, 1, 1);   // fc, vertical weight and bias
    for (int i = 0; i < cfg->n_heights; ++i) f += dw_list_floats(R, cF, cfg->heights[i] * tD);
    return f;
}

static CaserScratch carve_caser(void* ws, const cirs_caser_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    const long W = cfg->window, nF = cF * cfg->n_heights;
    CaserScratch s;
    s.G = c.take((size_t)R * 32); s.H = c.take((size_t)R * tD); s.Z = c.take((size_t)R * tD); s.dH = c.take((size_t)R * tD); s.dX = c.take((size_t)R * tD);
    s.DZ = c.take((size_t)R * tD); s.CAT = c.take((size_t)R * (nF + tD)); s.DO = c.take((size_t)R * nF); s.DVP = c.take((size_t)R * tD);
    s.ARG = (int32_t*)c.take((size_t)R * nF);
    s.VW = c.take((size_t)R * (W + 1)); s.ONES = c.take(R);
    s.WIN = c.take((size_t)R * W * tD + 3 * tD);
    s.DC = c.take((size_t)cfg->n_heights * R * W * cF);
    carve_slots(c, s, R, cfg->n_env, caser_partial_floats(cfg, R));
    *total_floats = c.total();
    return s;
}

// the cfg first and on its own: a cfg outside the fixed sizes is refused before any pointer is read
static int validate_caser_cfg(const cirs_caser_cfg* cfg) {
    CIRS_REQUIRE(cfg, "caser tracker: cfg null");
    CIRS_REQUIRE(cfg->window >= 1 && cfg->window <= cMaxW, "caser tracker: window must be in 1..16");
    CIRS_REQUIRE(cfg->n_heights >= 1 && cfg->n_heights <= cMaxNh, "caser tracker: n_heights must be in 1..4");
    for (int i = 0; i < cfg->n_heights; ++i) {
        CIRS_REQUIRE(cfg->heights[i] >= 1 && cfg->heights[i] <= 4, "caser tracker: heights must be in 1..4");
        CIRS_REQUIRE(i == 0 || cfg->heights[i] > cfg->heights[i - 1], "caser tracker: heights must be strictly ascending");
    }
    CIRS_REQUIRE(cfg->heights[cfg->n_heights - 1] <= cfg->window, "caser tracker: heights must not exceed window");
    return validate_slot_cfg(cfg, "caser tracker");
}

static int validate_caser(const cirs_caser_cfg* cfg, const cirs_caser_weights* w) {
    if (int rc = validate_caser_cfg(cfg)) return rc;
    CIRS_REQUIRE(w, "caser tracker: weights null");
    if (int rc = validate_slot_weights(w, "caser tracker")) return rc;
    CIRS_REQUIRE(w->vert_w && w->vert_b && w->fc_w && w->fc_b, "caser tracker: weight pointer null");
    for (int i = 0; i < cfg->n_heights; ++i) CIRS_REQUIRE(w->conv_w[i] && w->conv_b[i], "caser tracker: bank weight pointer null");
    return CIRS_OK;
}

static int launch_caser_step(const cirs_caser_cfg* cfg, const cirs_caser_weights* w, cirs_caser_state* st, const int32_t* users, const int64_t* items,
                             const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_REQUIRE(st && st->x_hist && st->len, "caser tracker: state pointer null");
    // 54 KB of LDS: two workgroups per CU.  Up to 4 x 2 x CUs envs every env has a wavefront of its own, beyond that a workgroup walks several groups of
    // four and what it staged (35 KB of weights at the default shape) serves them all.  Chosen from the structure, not tuned.
    const int walks = slot_walks(n, cEnvsPerWg, cWgPerCu);
    hipLaunchKernelGGL(caser_step_kernel, dim3(cdiv(n, (long)cEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n,
                       state_out, state_stride, walks);
    CIRS_CHECK_LAUNCH("caser_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_caser_tracker_init(const cirs_caser_cfg* cfg, const cirs_caser_weights* w, cirs_caser_state* st, const int32_t* users,
                                       const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_caser, cirs::launch_caser_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_caser_tracker_step(const cirs_caser_cfg* cfg, const cirs_caser_weights* w, cirs_caser_state* st, const int64_t* items, const double* rew,
                                       const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_caser, cirs::launch_caser_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_caser_tracker_backward_workspace_bytes(const cirs_caser_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_caser_cfg, cirs::carve_caser, cfg, n_rows);
}

extern "C" int cirs_caser_tracker_backward(const cirs_caser_cfg* cfg, const cirs_caser_weights* w, const cirs_caser_state* st, const int32_t* users,
                                           const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                           const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_caser_grads* grads, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_caser(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_slot_grads(grads, "caser tracker")) return rc;
    CIRS_REQUIRE(grads->vert_w && grads->vert_b && grads->fc_w && grads->fc_b, "caser tracker: gradient pointer null");
    for (int i = 0; i < cfg->n_heights; ++i) CIRS_REQUIRE(grads->conv_w[i] && grads->conv_b[i], "caser tracker: bank gradient pointer null");
    CIRS_REQUIRE((long)n_rows * cfg->window < (1L << 27), "caser tracker: n_rows * window out of range");
    CIRS_REQUIRE(workspace_bytes >= cirs_caser_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, W = cfg->window, nF = cF * cfg->n_heights, KC = nF + tD;
    size_t total = 0;
    CaserScratch sc = carve_caser(workspace, cfg, R, &total);
    DwList dwl{};
    hipLaunchKernelGGL(gather_dstate, dim3(cdiv((long)R * S, 256)), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    const int walks = slot_walks(R, cEnvsPerWg, cWgPerCu);
    hipLaunchKernelGGL(caser_rows_fwd, dim3(cdiv(R, (long)cEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, (const float*)st->x_hist, row_env, row_t, R, walks,
                       sc.H, sc.Z, sc.CAT, sc.ARG, sc.WIN, sc.ONES);
    launch_rows_gemm_dw(dwl, sc.H, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0, sc.dH,
                        tD, s);
    hipLaunchKernelGGL(caser_rows_bwd, dim3(cdiv(R, cEnvsPerWg)), dim3(256), 0, s, *cfg, *w, R, (const float*)sc.dH, (const float*)sc.Z,
                       (const float*)sc.CAT, (const int32_t*)sc.ARG, (const float*)sc.WIN, sc.DZ, sc.DO, sc.DVP, sc.DC, sc.VW);
    {   // fc and the vertical filter over the R rows
        DwBatch bt{};
        dw_batch_add(bt, dwl, sc.DZ, tD, sc.CAT, KC, R, tD, KC, grads->fc_w, grads->fc_b, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.VW, W + 1, sc.ONES, 1, R, W, 1, grads->vert_w, nullptr, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.VW + W, W + 1, sc.ONES, 1, R, 1, 1, grads->vert_b, nullptr, 0, sc.partial);
        dw_batch_launch(bt, R, s);
    }
    {   // the banks over the R W (row, position) pairs, in the slab count of the pass
        DwBatch bt{};
        for (int i = 0; i < cfg->n_heights; ++i)
            dw_batch_add(bt, dwl, sc.DC + (size_t)i * R * W * cF, cF, sc.WIN, tD, R, cF, cfg->heights[i] * tD, grads->conv_w[i], grads->conv_b[i], 0, sc.partial);
        dw_batch_launch(bt, R, s, R * W);
    }
    hipLaunchKernelGGL(caser_window_bwd, dim3(cdiv(R, 8)), dim3(256), 0, s, *cfg, *w, (const float*)sc.dH, (const float*)sc.DO, (const float*)sc.DVP,
                       (const int32_t*)sc.ARG, row_env, row_t, offsets, lens, R, sc.dX);
    CIRS_CHECK_LAUNCH("caser tracker backward window");
    return slots_backward(cfg, w, grads, sc.dX, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
