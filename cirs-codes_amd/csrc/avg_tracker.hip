// avg_tracker.hip -- StateTrackerAvg for gfx950: the pooled-window tracker, the floor under the sequence models (tracker.hip, gru_tracker.hip, lstm_tracker.hip).
//
// The reference has no counterpart; the model is defined here, in include/cirs_hip.h and in DESIGN.md 7.4:
//   inputs   the other trackers' slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k -- no sqrt(D) scale, no positional encoding
//   pooling  n_p = min(W, p);  m_0 = 0,  m_p = (x_{p-n_p+1} + ... + x_p) / n_p  (fp32, k ascending, then ONE division by float(n_p));  h_p = x_0 + m_p
//            the sum is formed anew from the stored slots at every step: no running sum, so position p depends on its window only
//   state    s_p = decoder(h_p)
// Step (one launch appends one position for n envs): lanes = the 32 model dimensions, so a slot row is one coalesced 128-byte access and a wavefront holds
// two envs; a workgroup (4 wavefronts = 8 envs per walk) stages the decoder [k][33] and the slot's matrix (fnn_gate, or ffn_user at init) [d][33] in LDS once
// -- both strides odd, so the transposed stores and the lane = row reads are conflict-free.  Everything per env is predicated, not branched: the two envs of a
// wavefront may differ in whether they are live and in how long their window is.
//
// Backward (the pooling is linear, rows = (env b, position p < len_b), env-major):
//   C  G = gather(dstate);  H = the pooled rows again from the stored slots (avg_rows_h: the decoder's weight gradient needs its input);
//      dH = G W_dec and the decoder's weight gradient in one launch (rows_gemm + dw_gemm, as the GRU's stage C)
//   W  avg_window_bwd: dX[b,0] = sum_p dH[b,p];  dX[b,k] = sum_{p=k}^{min(len_b-1, k+W-1)} dH[b,p] / float(n_p)   -- p ascending, every row on its own
//   E  the slot stage of the recurrent trackers (slot_tracker.h: slot_bwd with input scale 1, ordered embedding scatter, slab partials in slab order)
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include "slot_tracker.h"

namespace cirs {

constexpr int kAvgLds = tD + 1;                            // LDS stride of a staged 32-row matrix: 33 (odd: conflict-free both ways)
constexpr int kAvgEnvsPerWg = 8;                           // 4 wavefronts x 2 envs

__global__ __launch_bounds__(256) void avg_step_kernel(cirs_avg_cfg cfg, cirs_avg_weights w, cirs_avg_state st, const int32_t* __restrict__ users,
                                                       const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                       const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                       float* __restrict__ state_out, long state_stride, int walks) {
    __shared__ float sDec[tD * kAvgLds];                   // [k][s]: decoder, transposed
    __shared__ float sIn[tD * kAvgLds];                    // [d][c]: fnn_gate [32][33] (step) or ffn_user [32][32] (init), row-major
    __shared__ float sVec[4 * 128];                        // per wave and env: [0, 32) the slot's input vector, [32, 64) h
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state, W = cfg.window;
    const bool is_init = users != nullptr;
    // ---- the decoder and the slot's matrix, once per workgroup: coalesced reads of the row-major matrices ----
    for (int q = threadIdx.x; q < S * tD; q += 256) sDec[(q & 31) * kAvgLds + (q >> 5)] = w.dec_w[q];
    if (is_init) {
        for (int q = threadIdx.x; q < tD * tD; q += 256) sIn[(q >> 5) * kAvgLds + (q & 31)] = w.ffn_user_w[q];
    } else {
        for (int q = threadIdx.x; q < tD * (tD + 1); q += 256) sIn[q] = w.gate_w[q];
    }
    __syncthreads();
    float* vin = sVec + wv * 128 + half * 64;
    float* vh = vin + tD;
    const float* mrow = sIn + d * kAvgLds;
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long j = ((long)blockIdx.x * walks + it_w) * kAvgEnvsPerWg + wv * 2 + half;
        // ---- which rows are live: every refusal leaves the env and its row of state_out untouched ----
        bool ok = j < n;
        const long jj = ok ? j : 0;
        const int e = env_ids ? env_ids[jj] : (int)jj;
        ok = ok && e >= 0 && e < B;
        if (skip) ok = ok && !skip[jj];
        const size_t hist = (size_t)(ok ? e : 0) * L * tD;
        // ---- 1. the new input slot ----
        int pos = 0;
        float x, h;
        if (is_init) {
            const int u = users[jj];
            ok = ok && u >= 0 && u < cfg.n_users;
            vin[d] = ok ? w.emb_user[(size_t)u * tD + d] : 0.f;
            __builtin_amdgcn_wave_barrier();
            float acc = w.ffn_user_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mrow[k], vin[k], acc);
            x = acc;
            h = x;                                          // m_0 = 0
        } else {
            const long it = items[jj];
            ok = ok && it >= 0 && it < cfg.n_items;         // act = -1: the env finished earlier in this rollout
            pos = ok ? st.len[e] : 0;
            ok = ok && pos >= 1 && pos < L;                 // never initialised / history full
            const float r = ok ? (float)rew[jj] : 0.f;
            const float a = ok ? w.emb_item[(size_t)it * tD + d] : 0.f;
            vin[d] = a;
            __builtin_amdgcn_wave_barrier();
            float acc = __builtin_fmaf(mrow[0], r, w.gate_b[d]);      // input order [r, a_0..a_31]
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mrow[1 + k], vin[k], acc);
            x = cell_sigmoid(acc) * a;
            // ---- 2. the window: the stored slots first .. pos - 1 in ascending order, then the new one, then one division ----
            const int nw = ok ? std::min(W, pos) : 1;
            const int first = pos - nw + 1;
            const float* xh = st.x_hist + hist + d;
            float sum = nw > 1 ? xh[(size_t)first * tD] : x;
#pragma unroll 4
            for (int k = first + 1; k < pos; ++k) sum += xh[(size_t)k * tD];
            if (nw > 1) sum += x;
            h = (ok ? xh[0] : 0.f) + sum / (float)nw;
        }
        if (ok) st.x_hist[hist + (size_t)pos * tD + d] = x;
        // ---- 3. decoder ----
        vh[d] = h;
        __builtin_amdgcn_wave_barrier();
        if (d < S) {
            float acc = w.dec_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(sDec[k * kAvgLds + d], vh[k], acc);
            if (ok) state_out[(size_t)j * state_stride + d] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (ok && d == 0) st.len[e] = pos + 1;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// H[r] = h of buffer row r, from the stored slots in the step kernel's order.  32 lanes per row, 8 rows per workgroup.
__global__ __launch_bounds__(256) void avg_rows_h(const float* __restrict__ x_hist, const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t,
                                                  int R, int L, int W, float* __restrict__ H) {
    const long r = blockIdx.x * 8L + (threadIdx.x >> 5);
    if (r >= R) return;
    const int d = threadIdx.x & 31, p = row_t[r];
    const float* xh = x_hist + (size_t)row_env[r] * L * tD + d;
    float h = xh[0];
    if (p > 0) {
        const int nw = std::min(W, p);
        float sum = xh[(size_t)(p - nw + 1) * tD];
#pragma unroll 4
        for (int k = p - nw + 2; k <= p; ++k) sum += xh[(size_t)k * tD];
        h += sum / (float)nw;
    }
    H[(size_t)r * tD + d] = h;
}

// dX from dH: the transpose of the pooling.  Row (b, 0) collects every position of its env, row (b, k >= 1) the positions whose window holds slot k; p ascending,
// every term divided by its own float(n_p) before it is added.  No carry between rows: 32 lanes per row, 8 rows per workgroup.
__global__ __launch_bounds__(256) void avg_window_bwd(const float* __restrict__ dH, const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t,
                                                      const int32_t* __restrict__ offsets, const int32_t* __restrict__ lens, int R, int W,
                                                      float* __restrict__ dX) {
    const long r = blockIdx.x * 8L + (threadIdx.x >> 5);
    if (r >= R) return;
    const int d = threadIdx.x & 31, b = row_env[r], k = row_t[r], len = lens[b];
    const float* g = dH + (size_t)offsets[b] * tD + d;
    float acc = 0.f;
    if (k == 0) {
#pragma unroll 4
        for (int p = 0; p < len; ++p) acc += g[(size_t)p * tD];
    } else {
        const int last = (int)std::min<long>(len - 1, (long)k + W - 1);
#pragma unroll 4
        for (int p = k; p <= last; ++p) acc += g[(size_t)p * tD] / (float)std::min(W, p);
    }
    dX[(size_t)r * tD + d] = acc;
}

struct AvgScratch : SlotScratch {
    float *G, *H, *dH, *dX;
};

static size_t avg_partial_floats(long R) { return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1); }

static AvgScratch carve_avg(void* ws, const cirs_avg_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    AvgScratch s;
    s.G = c.take((size_t)R * 32); s.H = c.take((size_t)R * tD); s.dH = c.take((size_t)R * tD); s.dX = c.take((size_t)R * tD);
    carve_slots(c, s, R, cfg->n_env, avg_partial_floats(R));
    *total_floats = c.total();
    return s;
}

// the cfg first and on its own: a cfg outside the fixed sizes is refused before any pointer is read
static int validate_avg_cfg(const cirs_avg_cfg* cfg) {
    CIRS_REQUIRE(cfg, "avg tracker: cfg null");
    CIRS_REQUIRE(cfg->window >= 1, "avg tracker: window must be at least 1");
    return validate_slot_cfg(cfg, "avg tracker");
}

static int validate_avg(const cirs_avg_cfg* cfg, const cirs_avg_weights* w) {
    if (int rc = validate_avg_cfg(cfg)) return rc;
    CIRS_REQUIRE(w, "avg tracker: weights null");
    return validate_slot_weights(w, "avg tracker");
}

static int launch_avg_step(const cirs_avg_cfg* cfg, const cirs_avg_weights* w, cirs_avg_state* st, const int32_t* users, const int64_t* items,
                           const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_REQUIRE(st && st->x_hist && st->len, "avg tracker: state pointer null");
    // 10.5 KB of LDS and few registers: a CU could hold eight of these workgroups, and what a workgroup stages is 7 KB, so there is little to amortise.  Four
    // per CU (four wavefronts per SIMD, what the LDS reads need to reach their rate) is the cap: up to 8 x 4 x CUs envs every pair of envs has a wavefront of
    // its own, beyond that a workgroup walks several groups of eight.  Chosen from the structure, not tuned.
    const int walks = slot_walks(n, kAvgEnvsPerWg, 4);
    hipLaunchKernelGGL(avg_step_kernel, dim3(cdiv(n, (long)kAvgEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n,
                       state_out, state_stride, walks);
    CIRS_CHECK_LAUNCH("avg_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_avg_tracker_init(const cirs_avg_cfg* cfg, const cirs_avg_weights* w, cirs_avg_state* st, const int32_t* users,
                                     const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_avg, cirs::launch_avg_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_avg_tracker_step(const cirs_avg_cfg* cfg, const cirs_avg_weights* w, cirs_avg_state* st, const int64_t* items, const double* rew,
                                     const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_avg, cirs::launch_avg_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_avg_tracker_backward_workspace_bytes(const cirs_avg_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_avg_cfg, cirs::carve_avg, cfg, n_rows);
}

extern "C" int cirs_avg_tracker_backward(const cirs_avg_cfg* cfg, const cirs_avg_weights* w, const cirs_avg_state* st, const int32_t* users,
                                         const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                         const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_avg_grads* grads, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_avg(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_slot_grads(grads, "avg tracker")) return rc;
    CIRS_REQUIRE(workspace_bytes >= cirs_avg_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, L = cfg->max_len, W = cfg->window;
    size_t total = 0;
    AvgScratch sc = carve_avg(workspace, cfg, R, &total);
    DwList dwl{};
    hipLaunchKernelGGL(gather_dstate, dim3(cdiv((long)R * S, 256)), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    hipLaunchKernelGGL(avg_rows_h, dim3(cdiv(R, 8)), dim3(256), 0, s, (const float*)st->x_hist, row_env, row_t, R, L, W, sc.H);
    launch_rows_gemm_dw(dwl, sc.H, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0, sc.dH,
                        tD, s);
    hipLaunchKernelGGL(avg_window_bwd, dim3(cdiv(R, 8)), dim3(256), 0, s, (const float*)sc.dH, row_env, row_t, offsets, lens, R, W, sc.dX);
    CIRS_CHECK_LAUNCH("avg tracker backward pooling");
    return slots_backward(cfg, w, grads, sc.dX, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
