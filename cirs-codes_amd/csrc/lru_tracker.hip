// lru_tracker.hip -- StateTrackerLRU for gfx950: a linear recurrent unit (the diagonal complex recurrence of LRU / S4-style sequence models; LRURec, Yue et
// al., 2023) followed by a LayerNorm / GELU feed-forward block.
//
// The reference has no counterpart; the model is defined here, in include/cirs_hip.h and in DESIGN.md 7.11.  All arithmetic is real, a complex number is a
// (re, im) pair:
//   inputs     the GRU tracker's slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
//   lambda     = exp(-exp(nu_log)) (cos phi, sin phi), phi = exp(theta_log);  gamma = exp(gamma_log)           (|lambda| < 1 by construction)
//   v_p        = W_in x_p + b_in            (W_in [64, 32]: rows 0..31 the real part, 32..63 the imaginary part);  u_p = gamma * v_p (both parts of feature d)
//   h_p        = lambda * h_{p-1} + u_p, h_{-1} = 0:   h_re' = lr h_re - li h_im + u_re,   h_im' = lr h_im + li h_re + u_im
//   y_p        = W_out [h_re ; h_im] + b_out  (W_out [32, 64]);  z_p = LayerNorm(y_p + x_p)  (lru.ln)
//   m_p        = LayerNorm(z_p + W2 gelu(W1 z_p + b1) + b2)  (32 -> 128 -> 32, erf GELU, ffn.ln);  s_p = decoder(m_p)
//
// Step (one launch appends one position for n envs): ONE env per wavefront, four per workgroup, lane = (half, d) = (real | imaginary part, feature): the 64
// carried floats of an env are one per lane.  A workgroup stages W_in [64][33], W_out [32][65], W1 [128][33], W2 [32][129], the decoder [k][33] and the slot's
// matrix [d][33] in LDS once, and forms lambda and gamma from the three log vectors once (expf / cosf / sinf: phi is any positive float).  Per env: the slot
// and its write into x_hist; v (one 32-term dot per lane) and the recurrence on the carried h (the complex product needs the other half's value: one
// __shfl_xor(., 32)); the read-out (32 columns per half, joined by one shuffle); LayerNorm; the FFN (two of the 128 hidden units per lane, then 64 columns of
// W2 per half, joined by one shuffle); LayerNorm; the decoder.  fp32, fma chains in a fixed order, no atomics.  The cost of a step does not depend on the
// position.
//
// Backward (recompute-based over the buffer rows (env b, position p < len_b), env-major):
//   A  X = gather(x_hist);  V = X W_in^T + b_in                                        (rows_gemm, N = 64)
//   B  lru_scan_fwd: one env per wavefront, lanes (half, d), p ascending:  H[row] = lambda * H[row-1] + gamma * V[row]
//   C  Y = H W_out^T + b_out (Kd = 64);  Z = LN(Y + X), keeping xhat and rstd;  U = Z W1^T + b1 (N = 128);  GA = gelu(U);  F = GA W2^T + b2 (Kd = 128);
//      M = LN(Z + F), keeping xhat and rstd                                            (rows_gemm for the products, row kernels for LN / GELU)
//   D  G = gather(dstate);  dM = G W_dec and the decoder's gradients                   (rows_gemm + dw_gemm in one launch, as every tracker's stage C)
//   E  ffn.ln backward -> dP2;  dGA = dP2 W2 (+ dense_2's gradients);  dU = dGA gelu'(U);  dZ = dP2 + dU W1 (+ dense_1's gradients);
//      lru.ln backward -> dY, which is also the residual's share of dX
//   F  dHin = dY W_out  ([R, 64]) (+ out_proj's gradients)
//   G  lru_scan_bwd: one env per wavefront, p descending:  a_p = dHin_p + conj(lambda) * a_{p+1};  writes dV_p = gamma * a_p per row and, per env, the partial
//      sums of d lambda_re, d lambda_im and d gamma over its positions
//   H  lru_param_grad: the per-env partials summed over b in a fixed order, then the chain to nu_log, theta_log, gamma_log;
//      dW_in, db_in and the two LayerNorms' gradients (dw_batch);  dX += dV W_in;  the slot stage of the recurrent trackers (slot_tracker.h)
// The only sequential work is the complex multiply-add of B and G, one per position; the row loads of lScan positions are issued together, so a dependent
// memory round trip is paid once per lScan positions.  A workgroup-parallel (blocked) scan over the positions is not built.
// The workspace is O(rows) + O(n_env) and does not depend on max_len.  No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include "slot_tracker.h"

namespace cirs {

constexpr int lC = 2 * tD;                                 // 64: the complex state as floats, [re 0..31 | im 0..31]
constexpr int lHid = CIRS_LRU_HIDDEN;                      // 128
constexpr int lLds = tD + 1;                               // LDS stride of a row of 32: 33
constexpr int lOutLds = lC + 1;                            // ... of a row of W_out: 65
constexpr int lDownLds = lHid + 1;                         // ... of a row of W2: 129
constexpr int lEnvsPerWg = 4;                              // one env per wavefront
constexpr int lWgPerCu = 2;                                // 63 104 bytes of LDS per workgroup of the step kernel: two fit in a CU's 160 KB
constexpr int lVecFloats = 256;                            // per wave: x | z [0, 32), m [32, 64), h [64, 128), gelu(u) [128, 256)
constexpr int lScan = 8;                                   // positions of a scan whose row loads are issued together
constexpr float lEps = 1e-5f;

// lambda = exp(-exp(nu_log)) (cos phi, sin phi), phi = exp(theta_log);  gamma = exp(gamma_log) -- the accurate functions: phi is any positive float
__device__ __forceinline__ void lru_lambda(const float* nu_log, const float* theta_log, const float* gamma_log, int d, float& lr, float& li, float& ga) {
    const float mod = expf(-expf(nu_log[d])), phi = expf(theta_log[d]);
    lr = mod * cosf(phi); li = mod * sinf(phi); ga = expf(gamma_log[d]);
}

// the sum over the 32 lanes of a half-wavefront (xor 1 .. 16 stay inside the half): the same order, so the same bits, in every lane
__device__ __forceinline__ float lru_half_sum(float s) {
#pragma unroll
    for (int sft = 1; sft <= 16; sft <<= 1) s += __shfl_xor(s, sft, CIRS_WAVE);
    return s;
}

// LayerNorm of a row of 32 held one feature per lane of a half-wavefront: the normalised value and the inverse deviation
__device__ __forceinline__ void lru_ln(float x, float& xh, float& rstd) {
    const float mean = lru_half_sum(x) * (1.0f / tD);
    const float c = x - mean;
    const float var = lru_half_sum(c * c) * (1.0f / tD);
    rstd = 1.0f / sqrtf(var + lEps);
    xh = c * rstd;
}

__device__ __forceinline__ float lru_gelu(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752f)); }

// (256, 2): two wavefronts per SIMD, what the LDS admits
__global__ __launch_bounds__(256, 2) void lru_step_kernel(cirs_lru_cfg cfg, cirs_lru_weights w, cirs_lru_state st, const int32_t* __restrict__ users,
                                                          const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                          const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                          float* __restrict__ state_out, long state_stride, int walks) {
    __shared__ float sWin[lC * lLds];                      // [row 64][33]
    __shared__ float sWout[tD * lOutLds];                  // [row 32][65]
    __shared__ float sUp[lHid * lLds];                     // dense_1 [row 128][33]
    __shared__ float sDown[tD * lDownLds];                 // dense_2 [row 32][129]
    __shared__ float sDec[tD * lLds];                      // [k][s]: decoder, transposed
    __shared__ float sIn[tD * lLds];                       // [d][c]: fnn_gate [32][33] (step) or ffn_user [32][32] (init), row-major
    __shared__ float sLam[3 * tD];                         // lambda_re | lambda_im | gamma
    __shared__ float sVec[lEnvsPerWg * lVecFloats];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state;
    const bool is_init = users != nullptr;
    // ---- once per workgroup: coalesced reads of the row-major matrices ----
    for (int q = threadIdx.x; q < lC * tD; q += 256) sWin[(q >> 5) * lLds + (q & 31)] = w.in_w[q];
    for (int q = threadIdx.x; q < tD * lC; q += 256) sWout[(q >> 6) * lOutLds + (q & 63)] = w.out_w[q];
    for (int q = threadIdx.x; q < lHid * tD; q += 256) sUp[(q >> 5) * lLds + (q & 31)] = w.d1_w[q];
    for (int q = threadIdx.x; q < tD * lHid; q += 256) sDown[(q >> 7) * lDownLds + (q & 127)] = w.d2_w[q];
    for (int q = threadIdx.x; q < tD * lLds; q += 256) sDec[q] = 0.f;      // columns s >= S are read by no lane; cleared all the same
    __syncthreads();
    for (int q = threadIdx.x; q < S * tD; q += 256) sDec[(q & 31) * lLds + (q >> 5)] = w.dec_w[q];
    if (is_init) {
        for (int q = threadIdx.x; q < tD * tD; q += 256) sIn[(q >> 5) * lLds + (q & 31)] = w.ffn_user_w[q];
    } else {
        for (int q = threadIdx.x; q < tD * (tD + 1); q += 256) sIn[q] = w.gate_w[q];
    }
    if (threadIdx.x < tD) {
        float lr, li, ga;
        lru_lambda(w.nu_log, w.theta_log, w.gamma_log, threadIdx.x, lr, li, ga);
        sLam[threadIdx.x] = lr; sLam[tD + threadIdx.x] = li; sLam[2 * tD + threadIdx.x] = ga;
    }
    __syncthreads();
    float* vx = sVec + wv * lVecFloats;                    // x, later z
    float* vm = vx + tD;                                   // m
    float* vh = vx + 2 * tD;                               // h [64]
    float* vg = vx + 2 * tD + lC;                          // gelu(u) [128]
    const float* mrow = sIn + d * lLds;
    const float lr = sLam[d], ga = sLam[2 * tD + d];
    const float sl = half ? sLam[tD + d] : -sLam[tD + d];  // the other part's factor: re' takes -li h_im, im' takes +li h_re
    const float b_in = w.in_b[lane], b_out = w.out_b[d], b_up0 = w.d1_b[lane], b_up1 = w.d1_b[64 + lane], b_down = w.d2_b[d];
    const float g1 = w.lln_w[d], e1 = w.lln_b[d], g2 = w.ln_w[d], e2 = w.ln_b[d];
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long j = ((long)blockIdx.x * walks + it_w) * lEnvsPerWg + wv;
        if (j >= n) break;                                 // wave-uniform, as every refusal below: only wave barriers follow
        const int e = env_ids ? env_ids[j] : (int)j;
        if (e < 0 || e >= B) continue;
        if (skip && skip[j]) continue;
        // ---- 1. the new input slot (both halves of the wavefront hold it) and its write into x_hist ----
        int pos = 0;
        float x;
        if (is_init) {
            const int u = users[j];
            if (u < 0 || u >= cfg.n_users) continue;
            if (lane < tD) vx[lane] = w.emb_user[(size_t)u * tD + lane];
            __builtin_amdgcn_wave_barrier();
            float acc = w.ffn_user_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mrow[k], vx[k], acc);
            x = acc;
        } else {
            const long it = items[j];
            if (it < 0 || it >= cfg.n_items) continue;      // act = -1: the env finished earlier in this rollout
            pos = st.len[e];
            if (pos < 1 || pos >= L) continue;              // never initialised / history full
            const float r = (float)rew[j];
            const float a = w.emb_item[(size_t)it * tD + d];
            if (lane < tD) vx[lane] = a;
            __builtin_amdgcn_wave_barrier();
            float acc = __builtin_fmaf(mrow[0], r, w.gate_b[d]);      // input order [r, a_0..a_31]
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mrow[1 + k], vx[k], acc);
            x = cell_sigmoid(acc) * a;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < tD) { st.x_hist[((size_t)e * L + pos) * tD + d] = x; vx[lane] = x; }
        __builtin_amdgcn_wave_barrier();
        // ---- 2. v = W_in x + b_in (row `lane`), the recurrence on the carried h ----
        float hnew;
        {
            float* hp = (half ? st.h_im : st.h_re) + (size_t)e * tD + d;
            const float hprev = is_init ? 0.f : *hp;
            const float* wr = sWin + lane * lLds;
            float v = b_in;
#pragma unroll
            for (int k = 0; k < tD; ++k) v = __builtin_fmaf(wr[k], vx[k], v);
            const float other = __shfl_xor(hprev, 32, CIRS_WAVE);
            hnew = __builtin_fmaf(lr, hprev, __builtin_fmaf(sl, other, ga * v));
            *hp = hnew;
            vh[lane] = hnew;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- 3. y = W_out [h_re ; h_im] + b_out: the real part's columns in half 0, the imaginary part's in half 1;  z = LayerNorm(y + x) ----
        float z;
        {
            const float* wr = sWout + d * lOutLds + half * tD;
            const float* hv = vh + half * tD;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(wr[k], hv[k], acc);
            acc += __shfl_xor(acc, 32, CIRS_WAVE);         // a + b == b + a: both halves hold the same bits
            float xh, rstd;
            lru_ln((acc + b_out) + x, xh, rstd);
            z = __builtin_fmaf(xh, g1, e1);
        }
        __builtin_amdgcn_wave_barrier();                   // (vx was last read in 2.)
        if (lane < tD) vx[lane] = z;
        __builtin_amdgcn_wave_barrier();
        // ---- 4. the FFN: hidden units lane and 64 + lane;  then 64 columns of dense_2 per half;  m = LayerNorm(z + f) ----
        float m;
        {
            const float* w0 = sUp + lane * lLds;
            const float* w1 = sUp + (64 + lane) * lLds;
            float u0 = b_up0, u1 = b_up1;
#pragma unroll
            for (int k = 0; k < tD; ++k) {
                const float zk = vx[k];
                u0 = __builtin_fmaf(w0[k], zk, u0);
                u1 = __builtin_fmaf(w1[k], zk, u1);
            }
            vg[lane] = lru_gelu(u0); vg[64 + lane] = lru_gelu(u1);
            __builtin_amdgcn_wave_barrier();
            const float* wr = sDown + d * lDownLds + half * 64;
            const float* gv = vg + half * 64;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 64; ++k) acc = __builtin_fmaf(wr[k], gv[k], acc);
            acc += __shfl_xor(acc, 32, CIRS_WAVE);
            float xh, rstd;
            lru_ln(z + (acc + b_down), xh, rstd);
            m = __builtin_fmaf(xh, g2, e2);
        }
        if (lane < tD) vm[lane] = m;
        __builtin_amdgcn_wave_barrier();
        // ---- 5. decoder ----
        if (lane < S) {
            float acc = w.dec_b[lane];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(sDec[k * lLds + lane], vm[k], acc);
            state_out[(size_t)j * state_stride + lane] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) st.len[e] = pos + 1;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// (B) one env per wavefront, lane (half, d);  rows of an env are contiguous from offsets[b].  The loads of lScan rows of V are issued together; what is
// left per position is the shuffle and the two fmas of the step kernel, in its order.
__global__ __launch_bounds__(64) void lru_scan_fwd(const float* __restrict__ V, const float* __restrict__ nu_log, const float* __restrict__ theta_log,
                                                   const float* __restrict__ gamma_log, const int32_t* __restrict__ offsets,
                                                   const int32_t* __restrict__ lens, float* __restrict__ H) {
    const int lane = threadIdx.x, d = lane & (tD - 1), half = lane >> 5, b = blockIdx.x;
    const int len = lens[b];
    const size_t base = (size_t)offsets[b];
    float lr, li, ga;
    lru_lambda(nu_log, theta_log, gamma_log, d, lr, li, ga);
    const float sl = half ? li : -li;
    float h = 0.f;
    for (int p0 = 0; p0 < len; p0 += lScan) {
        float v[lScan];
#pragma unroll
        for (int u = 0; u < lScan; ++u) v[u] = V[(base + std::min(p0 + u, len - 1)) * lC + lane];
#pragma unroll
        for (int u = 0; u < lScan; ++u) {
            if (p0 + u >= len) break;                      // wave-uniform
            const float other = __shfl_xor(h, 32, CIRS_WAVE);
            h = __builtin_fmaf(lr, h, __builtin_fmaf(sl, other, ga * v[u]));
            H[(base + p0 + u) * lC + lane] = h;
        }
    }
}

// (G) the adjoint scan, p descending: a_p = g_p + conj(lambda) * a_{p+1}
//       a_re = g_re + lr a_re+ + li a_im+        a_im = g_im + lr a_im+ - li a_re+
// dV[row] = gamma * a_p;  per env, summed over its positions in descending p (h_{-1} = 0: position 0 adds nothing to the first two):
//   P[b][0][d] = sum_p a_re h_re,p-1 + a_im h_im,p-1      P[b][1][d] = sum_p -a_re h_im,p-1 + a_im h_re,p-1      P[b][2][d] = sum_p a_re v_re + a_im v_im
// (a lane sums its own part over p, the two parts are added once at the end).  An env without rows writes zeros.
__global__ __launch_bounds__(64) void lru_scan_bwd(const float* __restrict__ dHin, const float* __restrict__ H, const float* __restrict__ V,
                                                   const float* __restrict__ nu_log, const float* __restrict__ theta_log,
                                                   const float* __restrict__ gamma_log, const int32_t* __restrict__ offsets,
                                                   const int32_t* __restrict__ lens, float* __restrict__ dV, float* __restrict__ P) {
    const int lane = threadIdx.x, d = lane & (tD - 1), half = lane >> 5, b = blockIdx.x;
    const int len = lens[b];
    const size_t base = (size_t)offsets[b];
    float lr, li, ga;
    lru_lambda(nu_log, theta_log, gamma_log, d, lr, li, ga);
    const float sc = half ? -li : li;
    float a = 0.f, s_own = 0.f, s_cross = 0.f, s_v = 0.f;
    for (int p0 = len - 1; p0 >= 0; p0 -= lScan) {
        float g[lScan], vv[lScan], hm[lScan], ho[lScan];
#pragma unroll
        for (int u = 0; u < lScan; ++u) {
            const int p = std::max(p0 - u, 0);
            const size_t row = base + p;
            g[u] = dHin[row * lC + lane];
            vv[u] = V[row * lC + lane];
            hm[u] = p >= 1 ? H[(row - 1) * lC + lane] : 0.f;
            ho[u] = p >= 1 ? H[(row - 1) * lC + (lane ^ 32)] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < lScan; ++u) {
            if (p0 - u < 0) break;                         // wave-uniform
            const float other = __shfl_xor(a, 32, CIRS_WAVE);
            a = __builtin_fmaf(lr, a, __builtin_fmaf(sc, other, g[u]));
            dV[(base + p0 - u) * lC + lane] = ga * a;
            s_own = __builtin_fmaf(a, hm[u], s_own);
            s_cross = __builtin_fmaf(a, ho[u], s_cross);
            s_v = __builtin_fmaf(a, vv[u], s_v);
        }
    }
    s_cross = half ? s_cross : -s_cross;
    s_own += __shfl_xor(s_own, 32, CIRS_WAVE);             // a + b == b + a: both halves hold the same bits
    s_cross += __shfl_xor(s_cross, 32, CIRS_WAVE);
    s_v += __shfl_xor(s_v, 32, CIRS_WAVE);
    if (half == 0) {
        float* out = P + (size_t)b * 3 * tD;
        out[d] = s_own; out[tD + d] = s_cross; out[2 * tD + d] = s_v;
    }
}

// (H) the per-env partials summed over b in a fixed order (32 contiguous chunks of envs, each ascending, then the chunks ascending), then
//   d nu_log = -exp(nu_log) (lr dlr + li dli)      d theta_log = phi (-li dlr + lr dli)      d gamma_log = gamma dgamma
__global__ __launch_bounds__(1024) void lru_param_grad(const float* __restrict__ P, int B, const float* __restrict__ nu_log,
                                                       const float* __restrict__ theta_log, const float* __restrict__ gamma_log,
                                                       float* __restrict__ g_nu, float* __restrict__ g_theta, float* __restrict__ g_gamma) {
    __shared__ float sPart[32 * 3 * tD];
    const int d = threadIdx.x & 31, c = threadIdx.x >> 5;
    const int per = (B + 31) / 32, b_beg = c * per, b_end = std::min(B, b_beg + per);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int b = b_beg; b < b_end; ++b) {
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += P[((size_t)b * 3 + q) * tD + d];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) sPart[(c * 3 + q) * tD + d] = acc[q];
    __syncthreads();
    if (c != 0) return;
    float tot[3] = {0.f, 0.f, 0.f};
    for (int cc = 0; cc < 32; ++cc) {
#pragma unroll
        for (int q = 0; q < 3; ++q) tot[q] += sPart[(cc * 3 + q) * tD + d];
    }
    float lr, li, ga;
    lru_lambda(nu_log, theta_log, gamma_log, d, lr, li, ga);
    g_nu[d] = -expf(nu_log[d]) * (lr * tot[0] + li * tot[1]);
    g_theta[d] = expf(theta_log[d]) * (lr * tot[1] - li * tot[0]);
    g_gamma[d] = ga * tot[2];
}

// the row kernels of C and E: 32 lanes per row, 8 rows per workgroup
// OUT = LayerNorm(A + Bres) * g + e;  XH, RSTD: what the backward needs of it
__global__ __launch_bounds__(256) void lru_ln_rows(const float* __restrict__ A, const float* __restrict__ Bres, const float* __restrict__ g,
                                                   const float* __restrict__ e, int R, float* __restrict__ OUT, float* __restrict__ XH,
                                                   float* __restrict__ RSTD) {
    const long r = blockIdx.x * 8L + (threadIdx.x >> 5);
    const int d = threadIdx.x & 31;
    const bool live = r < R;                                // the half-wavefront's shuffles need all of its lanes: no early return
    const size_t o = (size_t)(live ? r : 0) * tD + d;
    float xh, rstd;
    lru_ln(A[o] + Bres[o], xh, rstd);
    if (!live) return;
    OUT[o] = __builtin_fmaf(xh, g[d], e[d]);
    XH[o] = xh;
    if (d == 0) RSTD[r] = rstd;
}

// dIN = the gradient at the input of a LayerNorm from dOUT at its output (the weight's and the bias's gradients are a diag problem over dOUT and XH);
// dIN2 (nullable): a second copy, the start of the sum along the residual path
__global__ __launch_bounds__(256) void lru_ln_rows_bwd(const float* __restrict__ dOUT, const float* __restrict__ XH, const float* __restrict__ RSTD,
                                                       const float* __restrict__ g, int R, float* __restrict__ dIN, float* __restrict__ dIN2) {
    const long r = blockIdx.x * 8L + (threadIdx.x >> 5);
    const int d = threadIdx.x & 31;
    const bool live = r < R;
    const size_t o = (size_t)(live ? r : 0) * tD + d;
    const float a = dOUT[o] * g[d], xh = XH[o];
    const float m1 = lru_half_sum(a) * (1.0f / tD), m2 = lru_half_sum(a * xh) * (1.0f / tD);
    if (!live) return;
    const float v = RSTD[r] * (a - m1 - xh * m2);
    dIN[o] = v;
    if (dIN2) dIN2[o] = v;
}

__global__ __launch_bounds__(256) void lru_gelu_rows(const float* __restrict__ U, long n, float* __restrict__ GA) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i < n) GA[i] = lru_gelu(U[i]);
}

// dU = dGA gelu'(U), gelu'(u) = Phi(u) + u phi(u); in place over dGA
__global__ __launch_bounds__(256) void lru_gelu_rows_bwd(const float* __restrict__ U, long n, float* __restrict__ dGA) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const float u = U[i];
    const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * expf(-0.5f * u * u);
    dGA[i] = dGA[i] * __builtin_fmaf(u, pdf, cdf);
}

struct LruScratch : SlotScratch {
    float *X, *V, *H, *Y, *Z, *XH1, *RSTD1, *U, *GA, *F, *M, *XH2, *RSTD2, *G, *dM, *dP2, *dGA, *dZ, *dY, *dHin, *dV, *P;
};

// the pass's list: decoder (S <= 32), dense_2, dense_1, out_proj, the two LayerNorms (diag), in_proj, ffn_user, gate -- nine problems
static size_t lru_partial_floats(long R) {
    return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, lHid) + dw_list_floats(R, lHid, tD) + dw_list_floats(R, tD, lC) + 2 * dw_list_floats(R, tD, tD) +
           dw_list_floats(R, lC, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1);
}

static LruScratch carve_lru(void* ws, const cirs_lru_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    LruScratch s;
    const size_t r32 = (size_t)R * tD, r64 = (size_t)R * lC, r128 = (size_t)R * lHid;
    s.X = c.take(r32); s.V = c.take(r64); s.H = c.take(r64); s.Y = c.take(r32); s.Z = c.take(r32); s.XH1 = c.take(r32); s.RSTD1 = c.take(R);
    s.U = c.take(r128); s.GA = c.take(r128); s.F = c.take(r32); s.M = c.take(r32); s.XH2 = c.take(r32); s.RSTD2 = c.take(R);
    s.G = c.take((size_t)R * 32); s.dM = c.take(r32); s.dP2 = c.take(r32); s.dGA = c.take(r128); s.dZ = c.take(r32); s.dY = c.take(r32);
    s.dHin = c.take(r64); s.dV = c.take(r64);
    s.P = c.take((size_t)cfg->n_env * 3 * tD);             // the per-env partials of the adjoint scan
    carve_slots(c, s, R, cfg->n_env, lru_partial_floats(R));
    *total_floats = c.total();
    return s;
}

// the cfg first and on its own: a cfg outside the fixed sizes is refused before any pointer is read
static int validate_lru_cfg(const cirs_lru_cfg* cfg) {
    CIRS_SLOT_REQUIRE(cfg, "lru tracker", "cfg/weights null");
    if (int rc = validate_slot_dim_model(cfg, "lru tracker")) return rc;
    if (cfg->nlayers != CIRS_LRU_MAX_LAYERS) return slot_fail(CIRS_E_UNSUPPORTED, "lru tracker", "nlayers must be 1 (one recurrence layer)");
    return validate_slot_sizes(cfg, "lru tracker");
}

template <class T>
static bool lru_cell_pointers(const T* w) {
    return w->nu_log && w->theta_log && w->gamma_log && w->in_w && w->in_b && w->out_w && w->out_b && w->lln_w && w->lln_b && w->d1_w && w->d1_b &&
           w->d2_w && w->d2_b && w->ln_w && w->ln_b;
}

static int validate_lru(const cirs_lru_cfg* cfg, const cirs_lru_weights* w) {
    if (int rc = validate_lru_cfg(cfg)) return rc;
    CIRS_SLOT_REQUIRE(w, "lru tracker", "cfg/weights null");
    if (int rc = validate_slot_weights(w, "lru tracker")) return rc;
    CIRS_SLOT_REQUIRE(lru_cell_pointers(w), "lru tracker", "recurrence / feed-forward weight pointer null (lru.* / ffn.*)");
    return CIRS_OK;
}

static int launch_lru_step(const cirs_lru_cfg* cfg, const cirs_lru_weights* w, cirs_lru_state* st, const int32_t* users, const int64_t* items,
                           const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_SLOT_REQUIRE(st && st->x_hist && st->h_re && st->h_im && st->len, "lru tracker", "state pointer null");
    // 63 104 bytes of LDS (58 624 of it the staged matrices, 4 096 the four wavefronts' vectors): two workgroups per CU, two wavefronts per SIMD.  Up to
    // 4 x 2 x CUs envs every env has a wavefront of its own, beyond that a workgroup walks several groups of four and what it staged serves them all.
    // From the structure (the LDS footprint), not tuned.
    const int walks = slot_walks(n, lEnvsPerWg, lWgPerCu);
    hipLaunchKernelGGL(lru_step_kernel, dim3(cdiv(n, (long)lEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n,
                       state_out, state_stride, walks);
    CIRS_CHECK_LAUNCH("lru_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_lru_tracker_init(const cirs_lru_cfg* cfg, const cirs_lru_weights* w, cirs_lru_state* st, const int32_t* users,
                                     const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_lru, cirs::launch_lru_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_lru_tracker_step(const cirs_lru_cfg* cfg, const cirs_lru_weights* w, cirs_lru_state* st, const int64_t* items, const double* rew,
                                     const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_lru, cirs::launch_lru_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_lru_tracker_backward_workspace_bytes(const cirs_lru_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_lru_cfg, cirs::carve_lru, cfg, n_rows);
}

extern "C" int cirs_lru_tracker_backward(const cirs_lru_cfg* cfg, const cirs_lru_weights* w, const cirs_lru_state* st, const int32_t* users,
                                         const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                         const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_lru_grads* grads, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_lru(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_slot_grads(grads, "lru tracker")) return rc;
    CIRS_SLOT_REQUIRE(lru_cell_pointers(grads), "lru tracker", "recurrence / feed-forward gradient pointer null (lru.* / ffn.*)");
    CIRS_REQUIRE(workspace_bytes >= cirs_lru_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, L = cfg->max_len;
    size_t total = 0;
    LruScratch sc = carve_lru(workspace, cfg, R, &total);
    const dim3 ln_grid(cdiv(R, 8)), hid_grid(cdiv((long)R * lHid, 256));
    // ---- forward recompute: the recurrence (A, B), the read-out and the feed-forward block (C) ----
    hipLaunchKernelGGL(gather_x, dim3(cdiv((long)R * tD, 256)), dim3(256), 0, s, (const float*)st->x_hist, row_env, row_t, R, L, sc.X);
    launch_rows_gemm(true, sc.X, tD, w->in_w, tD, w->in_b, R, tD, lC, 0, nullptr, 0, sc.V, lC, s);
    hipLaunchKernelGGL(lru_scan_fwd, dim3(B), dim3(64), 0, s, (const float*)sc.V, w->nu_log, w->theta_log, w->gamma_log, offsets, lens, sc.H);
    launch_rows_gemm(true, sc.H, lC, w->out_w, lC, w->out_b, R, lC, tD, 0, nullptr, 0, sc.Y, tD, s);
    hipLaunchKernelGGL(lru_ln_rows, ln_grid, dim3(256), 0, s, (const float*)sc.Y, (const float*)sc.X, w->lln_w, w->lln_b, R, sc.Z, sc.XH1, sc.RSTD1);
    launch_rows_gemm(true, sc.Z, tD, w->d1_w, tD, w->d1_b, R, tD, lHid, 0, nullptr, 0, sc.U, lHid, s);
    hipLaunchKernelGGL(lru_gelu_rows, hid_grid, dim3(256), 0, s, (const float*)sc.U, (long)R * lHid, sc.GA);
    launch_rows_gemm(true, sc.GA, lHid, w->d2_w, lHid, w->d2_b, R, lHid, tD, 0, nullptr, 0, sc.F, tD, s);
    hipLaunchKernelGGL(lru_ln_rows, ln_grid, dim3(256), 0, s, (const float*)sc.Z, (const float*)sc.F, w->ln_w, w->ln_b, R, sc.M, sc.XH2, sc.RSTD2);
    CIRS_CHECK_LAUNCH("lru tracker forward recompute");
    // ---- backward: the decoder (D), the feed-forward block and the two LayerNorms (E) ----
    DwList dwl{};
    hipLaunchKernelGGL(gather_dstate, dim3(cdiv((long)R * S, 256)), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    launch_rows_gemm_dw(dwl, sc.M, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0, sc.dM,
                        tD, s);
    hipLaunchKernelGGL(lru_ln_rows_bwd, ln_grid, dim3(256), 0, s, (const float*)sc.dM, (const float*)sc.XH2, (const float*)sc.RSTD2, w->ln_w, R, sc.dP2,
                       sc.dZ);      // dZ starts as the residual path's share; dense_1's is added to it
    launch_rows_gemm_dw(dwl, sc.GA, lHid, tD, lHid, grads->d2_w, grads->d2_b, sc.partial, false, sc.dP2, tD, w->d2_w, lHid, nullptr, R, tD, lHid, 0, nullptr, 0,
                        sc.dGA, lHid, s);
    hipLaunchKernelGGL(lru_gelu_rows_bwd, hid_grid, dim3(256), 0, s, (const float*)sc.U, (long)R * lHid, sc.dGA);
    launch_rows_gemm_dw(dwl, sc.Z, tD, lHid, tD, grads->d1_w, grads->d1_b, sc.partial, false, sc.dGA, lHid, w->d1_w, tD, nullptr, R, lHid, tD, 0, nullptr, 1,
                        sc.dZ, tD, s);
    hipLaunchKernelGGL(lru_ln_rows_bwd, ln_grid, dim3(256), 0, s, (const float*)sc.dZ, (const float*)sc.XH1, (const float*)sc.RSTD1, w->lln_w, R, sc.dY,
                       (float*)nullptr);
    CIRS_CHECK_LAUNCH("lru tracker backward feed-forward");
    // ---- the read-out (F), the adjoint scan (G), the recurrence's parameters and the input projection (H) ----
    launch_rows_gemm_dw(dwl, sc.H, lC, tD, lC, grads->out_w, grads->out_b, sc.partial, false, sc.dY, tD, w->out_w, lC, nullptr, R, tD, lC, 0, nullptr, 0,
                        sc.dHin, lC, s);
    hipLaunchKernelGGL(lru_scan_bwd, dim3(B), dim3(64), 0, s, (const float*)sc.dHin, (const float*)sc.H, (const float*)sc.V, w->nu_log, w->theta_log,
                       w->gamma_log, offsets, lens, sc.dV, sc.P);
    hipLaunchKernelGGL(lru_param_grad, dim3(1), dim3(1024), 0, s, (const float*)sc.P, B, w->nu_log, w->theta_log, w->gamma_log, grads->nu_log,
                       grads->theta_log, grads->gamma_log);
    DwBatch bt{};
    dw_batch_add(bt, dwl, sc.dM, tD, sc.XH2, tD, R, tD, tD, grads->ln_w, grads->ln_b, 1, sc.partial);
    dw_batch_add(bt, dwl, sc.dZ, tD, sc.XH1, tD, R, tD, tD, grads->lln_w, grads->lln_b, 1, sc.partial);
    dw_batch_add(bt, dwl, sc.dV, lC, sc.X, tD, R, lC, tD, grads->in_w, grads->in_b, 0, sc.partial);
    dw_batch_launch(bt, R, s);
    launch_rows_gemm(false, sc.dV, lC, w->in_w, tD, nullptr, R, lC, tD, 0, nullptr, 1, sc.dY, tD, s);      // dX = dY (the residual's share) + dV W_in
    CIRS_CHECK_LAUNCH("lru tracker backward recurrence");
    return slots_backward(cfg, w, grads, sc.dY, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
