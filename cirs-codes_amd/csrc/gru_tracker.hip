// gru_tracker.hip -- StateTrackerGRU for gfx950: the recurrent counterpart of tracker.hip / tracker_bwd.hip.
//
// The reference only announces the class (core/state_tracker.py:282-289, empty); the model is defined here and in DESIGN.md:
//   inputs   the Transformer tracker's slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k   (state_tracker.py:205-215,225-242)
//            -- no sqrt(D) scale, no positional encoding
//   cell     torch.nn.GRU(D, D, num_layers = L), h_{-1} = 0, gate order r, z, n:
//              r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)     z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//              n = tanh(W_in x + b_in + r * (W_hn h + b_hn))  h' = (1 - z) * n + z * h
//   state    s_t = decoder(h_t of the top layer)
// Step (one launch appends one position for n envs): a workgroup stages the cell weights of every layer in LDS once (25.6 KB per layer, [k][97] so that
// the stores and the lane = output reads are both conflict-free) and each of its four wavefronts then walks several envs -- per env the kernel reads an id,
// a reward, one embedding row and L x 32 carried floats, so the staging is what a workgroup has to amortise.  A wavefront is (half, feature d): half 0
// forms the three input dots of feature d, half 1 the three hidden dots, one cross-half shuffle joins them.  fma chains with k ascending, fp32 throughout.
//
// Backward (recompute-based BPTT over the buffer rows (env b, position p < len_b), env-major):
//   A  Gi = X W_ih^T + b_ih for all rows at once                                   (rows_gemm, MFMA)
//   B  gru_seq_fwd (gru_seq.h): one wavefront per env over p = 0 .. len-1, W_hh in LDS; keeps r, z, n, W_hn h + b_hn, h and the previous h per row
//   C  dH_top = gather(dstate) W_dec, the decoder's weight gradient                (rows_gemm + dw_gemm in one launch)
//   D  gru_seq_bwd: one wavefront per env over p = len-1 .. 0: dh = dH[p] + carry -> rows dGi, dGh; carry = dh * z + W_hh^T dGh
//   E  dW_ih, db_ih, dW_hh, db_hh (dw_batch, slab partials in slab order); dX = dGi W_ih = the lower layer's dH or the slot gradient;
//      then the Transformer tracker's slot backward (input scale 1) and ordered embedding scatter (tracker_rows.h)
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include <utility>
#include "gru_seq.h"

namespace cirs {

constexpr int kGruLayerFloats = 2 * kGruMat + 2 * gG;      // W_ih^T | W_hh^T | b_ih | b_hh = 6400 floats = 25.6 KB

__global__ __launch_bounds__(256) void gru_step_kernel(cirs_gru_cfg cfg, cirs_gru_weights w, cirs_gru_state st, const int32_t* __restrict__ users,
                                                       const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                       const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                       float* __restrict__ state_out, long state_stride, int envs_per_wave) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int nl = cfg.nlayers, B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state;
    // ---- the cell weights of every layer, once per workgroup: coalesced reads of the row-major [96][32] matrices, transposed stores ----
    for (int l = 0; l < nl; ++l) {
        float* Wl = smem + l * kGruLayerFloats;
        for (int q = threadIdx.x; q < 2 * gG * tD; q += 256) {
            const int m = q >= gG * tD, i = q - m * gG * tD, o = i >> 5, k = i & 31;
            Wl[m * kGruMat + k * kGruLds + o] = (m ? w.layer[l].w_hh : w.layer[l].w_ih)[i];
        }
        for (int q = threadIdx.x; q < 2 * gG; q += 256) Wl[2 * kGruMat + q] = q < gG ? w.layer[l].b_ih[q] : w.layer[l].b_hh[q - gG];
    }
    __syncthreads();
    float* vec = smem + nl * kGruLayerFloats + wv * 64;      // per wave: [0, 32) the cell's input, [32, 64) its previous h
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
            const float hprev = is_init ? 0.f : hp[d];
            vec[lane] = half ? hprev : hin;
            __builtin_amdgcn_wave_barrier();
            const float* Wl = smem + l * kGruLayerFloats + half * kGruMat + d;
            const float* bl = smem + l * kGruLayerFloats + 2 * kGruMat + half * gG + d;
            const float* v = vec + half * tD;
            float g0 = bl[0], g1 = bl[tD], g2 = bl[2 * tD];
#pragma unroll
            for (int k = 0; k < tD; ++k) {
                const float vk = v[k];
                g0 = __builtin_fmaf(Wl[k * kGruLds], vk, g0);
                g1 = __builtin_fmaf(Wl[k * kGruLds + tD], vk, g1);
                g2 = __builtin_fmaf(Wl[k * kGruLds + 2 * tD], vk, g2);
            }
            const float o0 = __shfl_xor(g0, 32, CIRS_WAVE), o1 = __shfl_xor(g1, 32, CIRS_WAVE), o2 = __shfl_xor(g2, 32, CIRS_WAVE);
            const float gi_r = half ? o0 : g0, gh_r = half ? g0 : o0, gi_z = half ? o1 : g1, gh_z = half ? g1 : o1;
            const float gi_n = half ? o2 : g2, gh_n = half ? g2 : o2;
            const float r = cell_sigmoid(gi_r + gh_r), z = cell_sigmoid(gi_z + gh_z);
            const float nn = tanhf(gi_n + r * gh_n);
            const float hnew = (1.0f - z) * nn + z * hprev;
            __builtin_amdgcn_wave_barrier();
            if (lane < tD) hp[d] = hnew;
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

// ---- BPTT (GruRows, gru_seq_fwd (B) and gru_seq_bwd (D): gru_seq.h) -----------------------------------------------------------------------------------
struct GruScratch : SlotScratch {
    float *X, *G, *dHa, *dHb, *dGi, *dGh, *Gi;
    GruRows rows[CIRS_GRU_MAX_LAYERS];
};

static size_t gru_partial_floats(const cirs_gru_cfg* cfg, long R) {
    return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1) + (size_t)cfg->nlayers * 2 * dw_list_floats(R, gG, tD);
}

static GruScratch carve_gru(void* ws, const cirs_gru_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    GruScratch s;
    s.X = c.take((size_t)R * tD); s.G = c.take((size_t)R * 32); s.dHa = c.take((size_t)R * tD); s.dHb = c.take((size_t)R * tD);
    s.dGi = c.take((size_t)R * gG); s.dGh = c.take((size_t)R * gG); s.Gi = c.take((size_t)R * gG);
    for (int l = 0; l < CIRS_GRU_MAX_LAYERS; ++l) {
        GruRows& g = s.rows[l];
        g.r = c.take((size_t)R * tD); g.z = c.take((size_t)R * tD); g.n = c.take((size_t)R * tD); g.hn = c.take((size_t)R * tD);
        g.h = c.take((size_t)R * tD); g.hp = c.take((size_t)R * tD);
    }
    carve_slots(c, s, R, cfg->n_env, gru_partial_floats(cfg, R));
    *total_floats = c.total();
    return s;
}

static int validate_gru_cfg(const cirs_gru_cfg* cfg) { return validate_recurrent_cfg(cfg, CIRS_GRU_MAX_LAYERS, "gru tracker"); }
static int validate_gru(const cirs_gru_cfg* cfg, const cirs_gru_weights* w) { return validate_recurrent(cfg, w, CIRS_GRU_MAX_LAYERS, "gru tracker"); }

static int launch_gru_step(const cirs_gru_cfg* cfg, const cirs_gru_weights* w, cirs_gru_state* st, const int32_t* users, const int64_t* items,
                           const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_REQUIRE(st && st->x_hist && st->h && st->len, "gru tracker state pointer null");
    // An env costs a wavefront ~3 us of dependent latency (4 us with two layers), the launch + staging ~10 us: more workgroups beat longer walks until the
    // CUs are full -- measured best at 4 workgroups per CU with one layer (26.6 KB of LDS each), 2 with two (52 KB); only beyond that a wavefront walks
    // several envs (DESIGN.md 7.2 has the numbers)
    const int wgs_per_cu = cfg->nlayers == 1 ? 4 : 2;
    const int epw = std::max(1, cdiv(n, 4L * wgs_per_cu * device_cu_count()));
    const size_t shmem = sizeof(float) * ((size_t)cfg->nlayers * kGruLayerFloats + 4 * 64);
    if (shmem > 48 * 1024) {
        static bool optin = false;
        if (!optin) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gru_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess)
                return fail(CIRS_E_LAUNCH, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
            optin = true;
        }
    }
    hipLaunchKernelGGL(gru_step_kernel, dim3(cdiv(n, 4L * epw)), dim3(256), shmem, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n, state_out,
                       state_stride, epw);
    CIRS_CHECK_LAUNCH("gru_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_gru_tracker_init(const cirs_gru_cfg* cfg, const cirs_gru_weights* w, cirs_gru_state* st, const int32_t* users,
                                     const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_gru, cirs::launch_gru_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_gru_tracker_step(const cirs_gru_cfg* cfg, const cirs_gru_weights* w, cirs_gru_state* st, const int64_t* items, const double* rew,
                                     const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_gru, cirs::launch_gru_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_gru_tracker_backward_workspace_bytes(const cirs_gru_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_gru_cfg, cirs::carve_gru, cfg, n_rows);
}

extern "C" int cirs_gru_tracker_backward(const cirs_gru_cfg* cfg, const cirs_gru_weights* w, const cirs_gru_state* st, const int32_t* users,
                                         const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                         const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_gru_grads* grads, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_gru(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_recurrent_grads(cfg, grads, "gru tracker")) return rc;
    CIRS_REQUIRE(workspace_bytes >= cirs_gru_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, L = cfg->max_len, nl = cfg->nlayers;
    size_t total = 0;
    GruScratch sc = carve_gru(workspace, cfg, R, &total);
    auto g1 = [&](long n) { return dim3(cdiv(n, 256)); };
    // ---- forward recompute ----
    hipLaunchKernelGGL(gather_x, g1((long)R * tD), dim3(256), 0, s, (const float*)st->x_hist, row_env, row_t, R, L, sc.X);
    for (int l = 0; l < nl; ++l) {
        const float* in = l == 0 ? sc.X : sc.rows[l - 1].h;
        launch_rows_gemm(true, in, tD, w->layer[l].w_ih, tD, w->layer[l].b_ih, R, tD, gG, 0, nullptr, 0, sc.Gi, gG, s);
        hipLaunchKernelGGL(gru_seq_fwd, dim3(B), dim3(64), 0, s, (const float*)sc.Gi, w->layer[l].w_hh, w->layer[l].b_hh, offsets, lens, sc.rows[l]);
    }
    CIRS_CHECK_LAUNCH("gru tracker forward recompute");
    // ---- backward ----
    DwList dwl{};
    hipLaunchKernelGGL(gather_dstate, g1((long)R * S), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    float *dH = sc.dHa, *dX = sc.dHb;
    launch_rows_gemm_dw(dwl, sc.rows[nl - 1].h, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0,
                        dH, tD, s);
    for (int l = nl - 1; l >= 0; --l) {
        const float* in = l == 0 ? sc.X : sc.rows[l - 1].h;
        hipLaunchKernelGGL(gru_seq_bwd, dim3(B), dim3(64), 0, s, (const float*)dH, sc.rows[l], w->layer[l].w_hh, offsets, lens, sc.dGi, sc.dGh);
        DwBatch bt{};
        dw_batch_add(bt, dwl, sc.dGi, gG, in, tD, R, gG, tD, grads->layer[l].w_ih, grads->layer[l].b_ih, 0, sc.partial);
        dw_batch_add(bt, dwl, sc.dGh, gG, sc.rows[l].hp, tD, R, gG, tD, grads->layer[l].w_hh, grads->layer[l].b_hh, 0, sc.partial);
        dw_batch_launch(bt, R, s);
        launch_rows_gemm(false, sc.dGi, gG, w->layer[l].w_ih, tD, nullptr, R, gG, tD, 0, nullptr, 0, dX, tD, s);
        std::swap(dH, dX);
    }
    CIRS_CHECK_LAUNCH("gru tracker backward layers");
    return slots_backward(cfg, w, grads, dH, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
