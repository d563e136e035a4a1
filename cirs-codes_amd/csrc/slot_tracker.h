// slot_tracker.h -- what the seven slot trackers (gru_tracker.hip, lstm_tracker.hip, avg_tracker.hip, caser_tracker.hip, nextitnet_tracker.hip,
// stamp_tracker.hip, narm_tracker.hip) share besides tracker_rows.h.  Device: the sigmoid and the gather of the stored input slots (the recurrent three).  Host: the checks of a
// cfg / weights / grads triple (the six trackers' structs have the same members around a different cell), the carving of a backward's workspace, the bodies
// of the entry points (init, step, workspace size), the walk count of a step launch, and the last stage of the backward (input
// slots + embeddings).
// No device code of the step kernels is here: the staging loop as a shared template changed the GRU step kernel's instruction sequence (1011 -> 1073), and
// the blocks the window trackers' step kernels have in common, moved into device helpers, changed Caser's register allocation.
#pragma once
#include <algorithm>
#include <string>
#include "tracker_rows.h"

namespace cirs {

__device__ __forceinline__ float cell_sigmoid(float a) { return 1.0f / (1.0f + expf(-a)); }

// X[r] = the stored input slot of buffer row r
static __global__ __launch_bounds__(256) void gather_x(const float* __restrict__ x_hist, const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t,
                                                       int R, int L, float* __restrict__ X) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)R * tD) return;
    const int r = (int)(i >> 5), k = (int)(i & 31);
    X[i] = x_hist[((size_t)row_env[r] * L + row_t[r]) * tD + k];
}

// ---- validation ----------------------------------------------------------------------------------------------------------------------
// `what` names the tracker in every message ("gru tracker", "avg tracker", ...); the message is built on the failure path only
inline int slot_fail(int code, const char* what, const char* msg) { return fail(code, std::string(what) + ": " + msg); }
#define CIRS_SLOT_REQUIRE(cond, what, msg)                               \
    do {                                                                 \
        if (!(cond)) return ::cirs::slot_fail(CIRS_E_INVALID, what, msg); \
    } while (0)

// the four checks every slot tracker makes of its cfg, in two pieces: the recurrent trackers report nlayers between them
template <class Cfg>
static int validate_slot_dim_model(const Cfg* cfg, const char* what) {
    if (cfg->dim_model != tD) return slot_fail(CIRS_E_UNSUPPORTED, what, "this build supports dim_model == 32");
    return CIRS_OK;
}
template <class Cfg>
static int validate_slot_sizes(const Cfg* cfg, const char* what) {
    CIRS_SLOT_REQUIRE(cfg->dim_state >= 1 && cfg->dim_state <= 32, what, "dim_state must be in 1..32");
    CIRS_SLOT_REQUIRE(cfg->max_len >= 1 && cfg->max_len <= 4096, what, "max_len out of range");
    CIRS_SLOT_REQUIRE(cfg->n_env >= 1 && cfg->n_users >= 1 && cfg->n_items >= 1, what, "n_env / n_users / n_items must be positive");
    return CIRS_OK;
}
// (a window tracker checks its own cell first, then these)
template <class Cfg>
static int validate_slot_cfg(const Cfg* cfg, const char* what) {
    if (int rc = validate_slot_dim_model(cfg, what)) return rc;
    return validate_slot_sizes(cfg, what);
}

// the eight pointers every slot tracker's weights / grads struct has
template <class Weights>
static int validate_slot_weights(const Weights* w, const char* what) {
    CIRS_SLOT_REQUIRE(w->emb_user && w->emb_item && w->ffn_user_w && w->ffn_user_b && w->gate_w && w->gate_b && w->dec_w && w->dec_b, what,
                      "weight pointer null");
    return CIRS_OK;
}
template <class Grads>
static int validate_slot_grads(const Grads* g, const char* what) {
    CIRS_SLOT_REQUIRE(g->emb_user && g->emb_item && g->ffn_user_w && g->ffn_user_b && g->gate_w && g->gate_b && g->dec_w && g->dec_b, what,
                      "gradient pointer null");
    return CIRS_OK;
}

// GRU and LSTM: the same cfg and the same layer members.  `what`: "gru tracker" / "lstm tracker"
template <class Cfg>
static int validate_recurrent_cfg(const Cfg* cfg, int max_layers, const char* what) {
    CIRS_SLOT_REQUIRE(cfg, what, "cfg/weights null");
    if (int rc = validate_slot_dim_model(cfg, what)) return rc;
    if (cfg->nlayers < 1 || cfg->nlayers > max_layers) return slot_fail(CIRS_E_UNSUPPORTED, what, "nlayers must be 1 or 2");
    return validate_slot_sizes(cfg, what);
}

template <class Cfg, class Weights>
static int validate_recurrent(const Cfg* cfg, const Weights* w, int max_layers, const char* what) {
    CIRS_SLOT_REQUIRE(cfg && w, what, "cfg/weights null");
    if (int rc = validate_recurrent_cfg(cfg, max_layers, what)) return rc;
    if (int rc = validate_slot_weights(w, what)) return rc;
    for (int l = 0; l < cfg->nlayers; ++l)
        CIRS_SLOT_REQUIRE(w->layer[l].w_ih && w->layer[l].w_hh && w->layer[l].b_ih && w->layer[l].b_hh, what, "layer weight pointer null");
    return CIRS_OK;
}

template <class Cfg, class Grads>
static int validate_recurrent_grads(const Cfg* cfg, const Grads* g, const char* what) {
    if (int rc = validate_slot_grads(g, what)) return rc;
    for (int l = 0; l < cfg->nlayers; ++l)
        CIRS_SLOT_REQUIRE(g->layer[l].w_ih && g->layer[l].w_hh && g->layer[l].b_ih && g->layer[l].b_hh, what, "layer gradient pointer null");
    return CIRS_OK;
}

// ---- workspace -----------------------------------------------------------------------------------------------------------------------
// a cursor over a backward's workspace: every piece starts on a multiple of 4 floats.  Over a null workspace it only counts.
struct Carver {
    float *base, *p;
    explicit Carver(void* ws) : base((float*)ws), p((float*)ws) {}
    float* take(size_t n) { float* r = p; p += (n + 3) & ~(size_t)3; return r; }
    size_t total() const { return (size_t)(p - base) + 64; }      // floats, with the slack every tracker's size has carried
};

// what the slot stage needs of a backward's scratch, carved by every tracker with the same sizes after its own pieces
struct SlotScratch {
    float *DU, *EU, *DPRE, *CU, *CI, *GIN, *partial;
    int32_t *key_user, *key_item;
    void* sort;
};

// partial_floats: the slab partials of the tracker's whole list (its own problems and the slot stage's)
inline void carve_slots(Carver& c, SlotScratch& s, long R, long B, size_t partial_floats) {
    s.DU = c.take((size_t)R * tD); s.EU = c.take((size_t)R * tD); s.DPRE = c.take((size_t)R * tD); s.CU = c.take((size_t)R * tD);
    s.CI = c.take((size_t)(R + B) * tD);      // item rows, then one user row per env (the merged scatter's layout)
    s.GIN = c.take((size_t)R * (tD + 1));
    s.key_user = (int32_t*)c.take(R); s.key_item = (int32_t*)c.take(R);
    s.partial = c.take(partial_floats + 4096);
    s.sort = (void*)c.take(emb_sort_bytes(R + B) / 4 + 64);
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
// The bodies of cirs_X_tracker_init / _step / _backward_workspace_bytes.  A tracker hands over its own functions:
//   validate(cfg, w)   launch(cfg, w, st, users, items, rew, env_ids, skip, n, state_out, state_stride, stream)   validate_cfg(cfg)
//   carve(workspace, cfg, n_rows, &total_floats)
// (The head of cirs_X_tracker_backward stays written out in each file: as a template over the tracker's structs it needed a 17-argument call and an
// adaptor per tracker for the grads and range checks, and came out longer than the six copies.)
template <class Cfg, class Weights, class State, class Validate, class Launch>
static int slot_tracker_init(Validate validate, Launch launch, const Cfg* cfg, const Weights* w, State* st, const int32_t* users, const int32_t* env_ids,
                             int32_t n, float* state_out, int64_t state_stride, void* stream) {
    if (int rc = validate(cfg, w)) return rc;
    if (n <= 0) return CIRS_OK;
    CIRS_REQUIRE(users && state_out, "users/state_out null");
    CIRS_REQUIRE(state_stride >= cfg->dim_state, "state_stride < dim_state");
    return launch(cfg, w, st, users, nullptr, nullptr, env_ids, nullptr, n, state_out, (long)state_stride, (hipStream_t)stream);
}

template <class Cfg, class Weights, class State, class Validate, class Launch>
static int slot_tracker_step(Validate validate, Launch launch, const Cfg* cfg, const Weights* w, State* st, const int64_t* items, const double* rew,
                             const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    if (int rc = validate(cfg, w)) return rc;
    if (n <= 0) return CIRS_OK;
    CIRS_REQUIRE(items && rew && state_out, "items/rew/state_out null");
    CIRS_REQUIRE(state_stride >= cfg->dim_state, "state_stride < dim_state");
    return launch(cfg, w, st, nullptr, items, rew, env_ids, skip, n, state_out, (long)state_stride, (hipStream_t)stream);
}

// 0 for exactly the cfgs validate_cfg refuses (and for n_rows <= 0)
template <class Cfg, class ValidateCfg, class Carve>
static int64_t slot_tracker_workspace_bytes(ValidateCfg validate_cfg, Carve carve, const Cfg* cfg, int32_t n_rows) {
    if (n_rows <= 0 || validate_cfg(cfg) != CIRS_OK) return 0;
    size_t total = 0;
    (void)carve(nullptr, cfg, n_rows, &total);
    return (int64_t)total * 4;
}

// how many groups of envs_per_wg rows a workgroup of a step-shaped launch walks: one until every CU holds wg_per_cu workgroups (each site says why its numbers)
inline int slot_walks(long n, int envs_per_wg, int wg_per_cu) { return std::max(1, cdiv(n, (long)envs_per_wg * wg_per_cu * device_cu_count())); }

// ---- backward, last stage --------------------------------------------------------------------------------------------------------------
// (E, second half) input slots + embeddings from dX of the bottom layer: the Transformer tracker's kernels with input scale 1, then every slab partial of
// the pass summed in slab order
template <class Cfg, class Weights, class Grads>
static int slots_backward(const Cfg* cfg, const Weights* w, const Grads* grads, const float* dX, const int32_t* users, const int64_t* act, const double* rew,
                          const int32_t* row_env, const int32_t* row_t, const int32_t* lens, int R, DwList& dwl, const SlotScratch& sc, hipStream_t s) {
    const int B = cfg->n_env;
    cirs_tracker_weights tw{};
    tw.emb_user = w->emb_user; tw.emb_item = w->emb_item; tw.ffn_user_w = w->ffn_user_w; tw.ffn_user_b = w->ffn_user_b; tw.gate_w = w->gate_w; tw.gate_b = w->gate_b;
    const int slot_rpw = R >= (1 << 17) ? 8 : 1;
    hipLaunchKernelGGL(slot_bwd, dim3(cdiv(R, 4 * slot_rpw)), dim3(256), 0, s, tw, dX, users, act, rew, row_env, row_t, R, B, sc.DU, sc.EU, sc.DPRE,
                       sc.GIN, sc.CU, sc.CI, sc.key_user, sc.key_item, sc.CI + (size_t)R * tD, slot_rpw, 1.0f);
    if (int rc = emb_scatter_merged(sc.key_item, users, lens, sc.CI, R, B, cfg->n_items, cfg->n_users, grads->emb_item, grads->emb_user, sc.sort,
                                    emb_sort_bytes(R + B), s))
        return rc;
    DwBatch bt{};
    dw_batch_add(bt, dwl, sc.DU, tD, sc.EU, tD, R, tD, tD, grads->ffn_user_w, grads->ffn_user_b, 0, sc.partial);
    dw_batch_add(bt, dwl, sc.DPRE, tD, sc.GIN, tD + 1, R, tD, tD + 1, grads->gate_w, grads->gate_b, 0, sc.partial);
    dw_batch_launch(bt, R, s);
    launch_dw_list_final(dwl, R, sc.partial, s);
    CIRS_CHECK_LAUNCH("recurrent tracker backward slots");
    return CIRS_OK;
}

}  // namespace cirs
