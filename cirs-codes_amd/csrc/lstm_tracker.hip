// lstm_tracker.hip -- StateTrackerLSTM for gfx950: the second recurrent tracker, built in the form of gru_tracker.hip.
//
// The reference only announces the class (core/state_tracker.py:282-289, empty); the model is defined here and in DESIGN.md 7.3:
//   inputs   the GRU tracker's slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
//   cell     torch.nn.LSTM(D, D, num_layers = L), h_{-1} = c_{-1} = 0, gate order i, f, g, o:
//              i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)   f = sigmoid(W_if x + b_if + W_hf h + b_hf)
//              g = tanh(W_ig x + b_ig + W_hg h + b_hg)      o = sigmoid(W_io x + b_io + W_ho h + b_ho)
//              c' = f * c + i * g                           h' = o * tanh(c')
//   state    s_t = decoder(h_t of the top layer)
// Step (one launch appends one position for n envs): a workgroup stages the cell weights of every layer in LDS once (34 KB per layer, [k][129]) and each
// of its four wavefronts then walks several envs.  A wavefront is (half, feature d): half 0 forms the four input dots of feature d, half 1 the four hidden
// dots, cross-half shuffles join them.  fma chains with k ascending, fp32 throughout.  h and c are carried per (layer, env) in global memory.
//
// Backward (recompute-based BPTT over the buffer rows (env b, position p < len_b), env-major), the GRU's stages:
//   A  Gi = X W_ih^T + b_ih for all rows at once                                   (rows_gemm, N = 128)
//   B  lstm_seq_fwd: one wavefront per env over p = 0 .. len-1, W_hh in LDS; keeps i, f, g, o, c, h and the previous c, h per row
//   C  dH_top = gather(dstate) W_dec, the decoder's weight gradient                (rows_gemm + dw_gemm in one launch)
//   D  lstm_seq_bwd: one wavefront per env over p = len-1 .. 0: the pre-activation gradients dG [R, 128]; the input side and the hidden side share them
//   E  dW_ih, dW_hh and both bias gradients from dG (dw_batch); dX = dG W_ih = the lower layer's dH or the slot gradient; then the slot stage (slot_tracker.h)
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include <utility>
#include "slot_tracker.h"

namespace cirs {

constexpr int lG = 4 * tD;                                 // gate rows of a cell matrix
constexpr int kLstmLds = lG + 1;                           // LDS stride of one k of a staged [k][128] matrix: 129 (odd: conflict-free both ways)
constexpr int kLstmMat = tD * kLstmLds;                    // 4128 floats; = 32 mod 64: the two matrices of a layer start half the banks apart
constexpr int kLstmLayerFloats = 2 * kLstmMat + 2 * lG;    // W_ih^T | W_hh^T | b_ih | b_hh = 8512 floats = 34 048 B

static size_t lstm_step_lds_bytes(int nlayers) { return sizeof(float) * ((size_t)nlayers * kLstmLayerFloats + 4 * 64); }

__global__ __launch_bounds__(256) void lstm_step_kernel(cirs_lstm_cfg cfg, cirs_lstm_weights w, cirs_lstm_state st, const int32_t* __restrict__ users,
                                                        const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                        const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                        float* __restrict__ state_out, long state_stride, int envs_per_wave) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int nl = cfg.nlayers, B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state;
    // ---- the cell weights of every layer, once per workgroup; every thread reaches the barrier before any per-env exit ----
    // (coalesced reads of the row-major [128][32] matrices, transposed stores)
    for (int l = 0; l < nl; ++l) {
        float* Wl = smem + l * kLstmLayerFloats;
        for (int q = threadIdx.x; q < 2 * lG * tD; q += 256) {
            const int m = q >= lG * tD, i = q - m * lG * tD, o = i >> 5, k = i & 31;
            Wl[m * kLstmMat + k * kLstmLds + o] = (m ? w.layer[l].w_hh : w.layer[l].w_ih)[i];
        }
        for (int q = threadIdx.x; q < 2 * lG; q += 256) Wl[2 * kLstmMat + q] = q < lG ? w.layer[l].b_ih[q] : w.layer[l].b_hh[q - lG];
    }
    __syncthreads();
    float* vec = smem + nl * kLstmLayerFloats + wv * 64;      // per wave: [0, 32) the cell's input, [32, 64) its previous h
    const bool is_init = users != nullptr;
    for (int it_e = 0; it_e < envs_per_wave; ++it_e) {
        const int j = (blockIdx.x * envs_per_wave + it_e) * 4 + wv;
        if (j >= n) break;
        const int e = env_ids ? env_ids[j] : j;
        if (e < 0 || e >= B) continue;
        if (skip && skip[j]) continue;
        // ---- 1. the new input slot ----
        int pos = 0;
        float x;
        if (is_init) {
            const int u = users[j];
            if (u < 0 || u >= cfg.n_users) continue;
            if (lane < tD) vec[lane] = w.emb_user[(size_t)u * tD + lane];
            __builtin_amdgcn_wave_barrier();
            const float* fr = w.ffn_user_w + (size_t)d * tD;
            float acc = w.ffn_user_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(fr[k], vec[k], acc);
            x = acc;
        } else {
            const long it = items[j];
            if (it < 0 || it >= cfg.n_items) continue;      // act = -1: the env finished earlier in this rollout
            pos = st.len[e];
            if (pos < 1 || pos >= L) continue;              // never initialised / history full
            const float r = (float)rew[j];
            const float a = w.emb_item[(size_t)it * tD + d];
            if (lane < tD) vec[lane] = a;
            __builtin_amdgcn_wave_barrier();
            const float* gw = w.gate_w + (size_t)d * (tD + 1);      // input order [r, a_0..a_31]
            float acc = __builtin_fmaf(gw[0], r, w.gate_b[d]);
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(gw[1 + k], vec[k], acc);
            x = cell_sigmoid(acc) * a;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < tD) st.x_hist[((size_t)e * L + pos) * tD + d] = x;
        // ---- 2. the cells ----
        float hin = x;
        for (int l = 0; l < nl; ++l) {
            float* hp = st.h + ((size_t)l * B + e) * tD;
            float* cp = st.c + ((size_t)l * B + e) * tD;
            const float hprev = is_init ? 0.f : hp[d];
            const float cprev = is_init ? 0.f : cp[d];
            vec[lane] = half ? hprev : hin;
            __builtin_amdgcn_wave_barrier();
            const float* Wl = smem + l * kLstmLayerFloats + half * kLstmMat + d;
            const float* bl = smem + l * kLstmLayerFloats + 2 * kLstmMat + half * lG + d;
            const float* v = vec + half * tD;
            float g0 = bl[0], g1 = bl[tD], g2 = bl[2 * tD], g3 = bl[3 * tD];
#pragma unroll
            for (int k = 0; k < tD; ++k) {
                const float vk = v[k];
                g0 = __builtin_fmaf(Wl[k * kLstmLds], vk, g0);
                g1 = __builtin_fmaf(Wl[k * kLstmLds + tD], vk, g1);
                g2 = __builtin_fmaf(Wl[k * kLstmLds + 2 * tD], vk, g2);
                g3 = __builtin_fmaf(Wl[k * kLstmLds + 3 * tD], vk, g3);
            }
            // the other half's four dots: input side + hidden side in every lane (one rounding, the same in both halves)
            const float gi = cell_sigmoid(g0 + __shfl_xor(g0, 32, CIRS_WAVE)), gf = cell_sigmoid(g1 + __shfl_xor(g1, 32, CIRS_WAVE));
            const float gg = tanhf(g2 + __shfl_xor(g2, 32, CIRS_WAVE)), go = cell_sigmoid(g3 + __shfl_xor(g3, 32, CIRS_WAVE));
            const float cnew = gf * cprev + gi * gg;
            const float hnew = go * tanhf(cnew);
            __builtin_amdgcn_wave_barrier();
            if (lane < tD) { hp[d] = hnew; cp[d] = cnew; }
            hin = hnew;
        }
        // ---- 3. decoder ----
        if (lane < tD) vec[lane] = hin;
        __builtin_amdgcn_wave_barrier();
        if (lane < S) {
            const float* dr = w.dec_w + (size_t)lane * tD;
            float acc = w.dec_b[lane];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(dr[k], vec[k], acc);
            state_out[(size_t)j * state_stride + lane] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) st.len[e] = pos + 1;
    }
}

// ---- BPTT ---------------------------------------------------------------------------------------------------------------------------
struct LstmRows { float *i, *f, *g, *o, *c, *cp, *h, *hp; };      // [R, 32] each: the gates, the new and the previous c and h of every row

// (B) one wavefront per env.  Lane (half, d): half 0 forms rows d of W_hi h and W_hf h, half 1 rows d of W_hg h and W_ho h (full 32-term dots).
__global__ __launch_bounds__(64) void lstm_seq_fwd(const float* __restrict__ Gi, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
                                                   const int32_t* __restrict__ offsets, const int32_t* __restrict__ lens, LstmRows a) {
    __shared__ float sW[kLstmMat];
    __shared__ float sb[lG];
    __shared__ float sh[tD];
    const int lane = threadIdx.x, d = lane & (tD - 1), half = lane >> 5;
    for (int q = lane; q < lG * tD; q += 64) sW[(q & 31) * kLstmLds + (q >> 5)] = w_hh[q];
    for (int q = lane; q < lG; q += 64) sb[q] = b_hh[q];
    __syncthreads();
    const int b = blockIdx.x, len = lens[b], off = offsets[b];
    if (len <= 0) return;
    const int oa = 2 * tD * half + d;      // this lane's two rows: oa and oa + 32
    float h = 0.f, c = 0.f;
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = Gi[(size_t)off * lG + q * tD + d];
    for (int t = 0; t < len; ++t) {
        const size_t row = (size_t)off + t;
        const float x_i = p[0], x_f = p[1], x_g = p[2], x_o = p[3];
        if (t + 1 < len) {
#pragma unroll
            for (int q = 0; q < 4; ++q) p[q] = Gi[(row + 1) * lG + q * tD + d];
        }
        if (lane < tD) sh[lane] = h;
        __builtin_amdgcn_wave_barrier();
        float a0 = sb[oa], a1 = sb[oa + tD];
#pragma unroll
        for (int k = 0; k < tD; ++k) {
            const float hk = sh[k];
            a0 = __builtin_fmaf(sW[k * kLstmLds + oa], hk, a0);
            a1 = __builtin_fmaf(sW[k * kLstmLds + oa + tD], hk, a1);
        }
        const float o0 = __shfl_xor(a0, 32, CIRS_WAVE), o1 = __shfl_xor(a1, 32, CIRS_WAVE);
        const float h_i = half ? o0 : a0, h_f = half ? o1 : a1, h_g = half ? a0 : o0, h_o = half ? a1 : o1;
        const float gi = cell_sigmoid(x_i + h_i), gf = cell_sigmoid(x_f + h_f), gg = tanhf(x_g + h_g), go = cell_sigmoid(x_o + h_o);
        const float cnew = gf * c + gi * gg;
        const float hnew = go * tanhf(cnew);
        __builtin_amdgcn_wave_barrier();
        if (lane < tD) {
            const size_t o = row * tD + d;
            a.i[o] = gi; a.f[o] = gf; a.g[o] = gg; a.o[o] = go; a.cp[o] = c; a.c[o] = cnew; a.hp[o] = h; a.h[o] = hnew;
        }
        h = hnew; c = cnew;
    }
}

// (D) one wavefront per env, positions in reverse.  carry_h[k] = sum_o dG[o] W_hh[o][k]: lane (half, k) adds the 64 rows o of its half in ascending order.
__global__ __launch_bounds__(64) void lstm_seq_bwd(const float* __restrict__ dH, LstmRows a, const float* __restrict__ w_hh, const int32_t* __restrict__ offsets,
                                                   const int32_t* __restrict__ lens, float* __restrict__ dG) {
    __shared__ float sW[lG * tD];
    __shared__ float sg[lG];
    const int lane = threadIdx.x, d = lane & (tD - 1), half = lane >> 5;
    for (int q = lane; q < lG * tD; q += 64) sW[q] = w_hh[q];
    __syncthreads();
    const int b = blockIdx.x, len = lens[b], off = offsets[b];
    float carry_h = 0.f, carry_c = 0.f;
    for (int t = len - 1; t >= 0; --t) {
        const size_t row = (size_t)off + t, o = row * tD + d;
        const float gi = a.i[o], gf = a.f[o], gg = a.g[o], go = a.o[o], c = a.c[o], cprev = a.cp[o];
        const float dh = dH[o] + carry_h;
        const float tc = tanhf(c);
        const float dc = dh * go * (1.0f - tc * tc) + carry_c;
        const float da_i = dc * gg * gi * (1.0f - gi);
        const float da_f = dc * cprev * gf * (1.0f - gf);
        const float da_g = dc * gi * (1.0f - gg * gg);
        const float da_o = dh * tc * go * (1.0f - go);
        if (lane < tD) {
            dG[row * lG + d] = da_i; dG[row * lG + tD + d] = da_f; dG[row * lG + 2 * tD + d] = da_g; dG[row * lG + 3 * tD + d] = da_o;
            sg[d] = da_i; sg[tD + d] = da_f; sg[2 * tD + d] = da_g; sg[3 * tD + d] = da_o;
        }
        __builtin_amdgcn_wave_barrier();
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < lG / 2; ++q) {
            const int oo = q + (lG / 2) * half;
            acc = __builtin_fmaf(sg[oo], sW[oo * tD + d], acc);
        }
        const float other = __shfl_xor(acc, 32, CIRS_WAVE);
        carry_h = (half ? other : acc) + (half ? acc : other);
        carry_c = dc * gf;
        __builtin_amdgcn_wave_barrier();
    }
}

struct LstmScratch : SlotScratch {
    float *X, *G, *dHa, *dHb, *dG, *Gi;
    LstmRows rows[CIRS_LSTM_MAX_LAYERS];
};

static size_t lstm_partial_floats(const cirs_lstm_cfg* cfg, long R) {
    return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1) + (size_t)cfg->nlayers * 2 * dw_list_floats(R, lG, tD);
}

static LstmScratch carve_lstm(void* ws, const cirs_lstm_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    LstmScratch s;
    s.X = c.take((size_t)R * tD); s.G = c.take((size_t)R * 32); s.dHa = c.take((size_t)R * tD); s.dHb = c.take((size_t)R * tD);
    s.dG = c.take((size_t)R * lG); s.Gi = c.take((size_t)R * lG);
    for (int l = 0; l < CIRS_LSTM_MAX_LAYERS; ++l)
        for (float** q : {&s.rows[l].i, &s.rows[l].f, &s.rows[l].g, &s.rows[l].o, &s.rows[l].c, &s.rows[l].cp, &s.rows[l].h, &s.rows[l].hp}) *q = c.take((size_t)R * tD);
    carve_slots(c, s, R, cfg->n_env, lstm_partial_floats(cfg, R));
    *total_floats = c.total();
    return s;
}

static int validate_lstm_cfg(const cirs_lstm_cfg* cfg) { return validate_recurrent_cfg(cfg, CIRS_LSTM_MAX_LAYERS, "lstm tracker"); }
static int validate_lstm(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w) { return validate_recurrent(cfg, w, CIRS_LSTM_MAX_LAYERS, "lstm tracker"); }

static int launch_lstm_step(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w, cirs_lstm_state* st, const int32_t* users, const int64_t* items,
                            const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_REQUIRE(st && st->x_hist && st->h && st->c && st->len, "lstm tracker: state pointer null");
    // As for the GRU, more workgroups beat longer walks until the CUs are full, and a CU holds fewer of these: 3 with one layer (148 VGPRs: three
    // wavefronts per SIMD; a fourth workgroup waits for a whole round), 2 with two (69 KB of LDS each).  Only beyond that a wavefront walks several
    // envs (DESIGN.md 7.3 has the numbers)
    const int wgs_per_cu = cfg->nlayers == 1 ? 3 : 2;
    const int epw = std::max(1, cdiv(n, 4L * wgs_per_cu * device_cu_count()));
    const size_t shmem = lstm_step_lds_bytes(cfg->nlayers);
    if (shmem > 48 * 1024) {
        static bool optin = false;
        if (!optin) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&lstm_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lstm_step_lds_bytes(CIRS_LSTM_MAX_LAYERS)) != hipSuccess)
                return fail(CIRS_E_LAUNCH, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
            optin = true;
        }
    }
    hipLaunchKernelGGL(lstm_step_kernel, dim3(cdiv(n, 4L * epw)), dim3(256), shmem, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n, state_out,
                       state_stride, epw);
    CIRS_CHECK_LAUNCH("lstm_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_lstm_tracker_init(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w, cirs_lstm_state* st, const int32_t* users,
                                      const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_lstm, cirs::launch_lstm_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_lstm_tracker_step(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w, cirs_lstm_state* st, const int64_t* items, const double* rew,
                                      const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_lstm, cirs::launch_lstm_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_lstm_tracker_backward_workspace_bytes(const cirs_lstm_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_lstm_cfg, cirs::carve_lstm, cfg, n_rows);
}

extern "C" int cirs_lstm_tracker_backward(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w, const cirs_lstm_state* st, const int32_t* users,
                                          const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                          const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_lstm_grads* grads, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_lstm(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_recurrent_grads(cfg, grads, "lstm tracker")) return rc;
    CIRS_REQUIRE(workspace_bytes >= cirs_lstm_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, L = cfg->max_len, nl = cfg->nlayers;
    size_t total = 0;
    LstmScratch sc = carve_lstm(workspace, cfg, R, &total);
    auto g1 = [&](long n) { return dim3(cdiv(n, 256)); };
    // ---- forward recompute ----
    hipLaunchKernelGGL(gather_x, g1((long)R * tD), dim3(256), 0, s, (const float*)st->x_hist, row_env, row_t, R, L, sc.X);
    for (int l = 0; l < nl; ++l) {
        const float* in = l == 0 ? sc.X : sc.rows[l - 1].h;
        launch_rows_gemm(true, in, tD, w->layer[l].w_ih, tD, w->layer[l].b_ih, R, tD, lG, 0, nullptr, 0, sc.Gi, lG, s);
        hipLaunchKernelGGL(lstm_seq_fwd, dim3(B), dim3(64), 0, s, (const float*)sc.Gi, w->layer[l].w_hh, w->layer[l].b_hh, offsets, lens, sc.rows[l]);
    }
    CIRS_CHECK_LAUNCH("lstm tracker forward recompute");
    // ---- backward ----
    DwList dwl{};
    hipLaunchKernelGGL(gather_dstate, g1((long)R * S), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    float *dH = sc.dHa, *dX = sc.dHb;
    launch_rows_gemm_dw(dwl, sc.rows[nl - 1].h, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0,
                        dH, tD, s);
    for (int l = nl - 1; l >= 0; --l) {
        const float* in = l == 0 ? sc.X : sc.rows[l - 1].h;
        hipLaunchKernelGGL(lstm_seq_bwd, dim3(B), dim3(64), 0, s, (const float*)dH, sc.rows[l], w->layer[l].w_hh, offsets, lens, sc.dG);
        DwBatch bt{};      // one dG serves both matrices and both bias vectors (b_ih and b_hh receive the same gradient)
        dw_batch_add(bt, dwl, sc.dG, lG, in, tD, R, lG, tD, grads->layer[l].w_ih, grads->layer[l].b_ih, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.dG, lG, sc.rows[l].hp, tD, R, lG, tD, grads->layer[l].w_hh, grads->layer[l].b_hh, 0, sc.partial);
        dw_batch_launch(bt, R, s);
        launch_rows_gemm(false, sc.dG, lG, w->layer[l].w_ih, tD, nullptr, R, lG, tD, 0, nullptr, 0, dX, tD, s);
        std::swap(dH, dX);
    }
    CIRS_CHECK_LAUNCH("lstm tracker backward layers");
    return slots_backward(cfg, w, grads, dH, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
