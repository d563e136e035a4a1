// recurrent.h -- what the two recurrent state trackers (gru_tracker.hip: GRU, lstm_tracker.hip: LSTM) share besides tracker_rows.h: the sigmoid, the
// gather of the stored input slots, the validation of a cfg / weights pair (the two trackers' structs have
// the same members around a different cell), and the last stage of the backward (input slots + embeddings).
// The staging loop of the step kernels is not here: as a shared template it changed the GRU step kernel's instruction sequence (1011 -> 1073).
#pragma once
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

// `what`: "gru tracker" / "lstm tracker"
template <class Cfg, class Weights>
static int validate_recurrent(const Cfg* cfg, const Weights* w, int max_layers, const char* what) {
    const std::string p = std::string(what) + ": ";
    CIRS_REQUIRE(cfg && w, p + "cfg/weights null");
    if (cfg->dim_model != tD) return fail(CIRS_E_UNSUPPORTED, p + "this build supports dim_model == 32");
    if (cfg->nlayers < 1 || cfg->nlayers > max_layers) return fail(CIRS_E_UNSUPPORTED, p + "nlayers must be 1 or 2");
    CIRS_REQUIRE(cfg->dim_state >= 1 && cfg->dim_state <= 32, p + "dim_state must be in 1..32");
    CIRS_REQUIRE(cfg->max_len >= 1 && cfg->max_len <= 4096, p + "max_len out of range");
    CIRS_REQUIRE(cfg->n_env >= 1 && cfg->n_users >= 1 && cfg->n_items >= 1, p + "n_env / n_users / n_items must be positive");
    CIRS_REQUIRE(w->emb_user && w->emb_item && w->ffn_user_w && w->ffn_user_b && w->gate_w && w->gate_b && w->dec_w && w->dec_b, p + "weight pointer null");
    for (int l = 0; l < cfg->nlayers; ++l)
        CIRS_REQUIRE(w->layer[l].w_ih && w->layer[l].w_hh && w->layer[l].b_ih && w->layer[l].b_hh, p + "layer weight pointer null");
    return CIRS_OK;
}

template <class Cfg, class Grads>
static int validate_recurrent_grads(const Cfg* cfg, const Grads* g, const char* what) {
    const std::string p = std::string(what) + ": ";
    CIRS_REQUIRE(g->emb_user && g->emb_item && g->ffn_user_w && g->ffn_user_b && g->gate_w && g->gate_b && g->dec_w && g->dec_b, p + "gradient pointer null");
    for (int l = 0; l < cfg->nlayers; ++l)
        CIRS_REQUIRE(g->layer[l].w_ih && g->layer[l].w_hh && g->layer[l].b_ih && g->layer[l].b_hh, p + "layer gradient pointer null");
    return CIRS_OK;
}

// what the slot stage needs of a backward's scratch, carved by both trackers with the same sizes
struct SlotScratch {
    float *DU, *EU, *DPRE, *CU, *CI, *GIN, *partial;
    int32_t *key_user, *key_item;
    void* sort;
};

// (E, second half) input slots + embeddings from dX of the bottom layer: the Transformer tracker's kernels with input scale 1, then every slab partial of
// the pass summed in slab order
template <class Cfg, class Weights, class Grads>
static int recurrent_slots_backward(const Cfg* cfg, const Weights* w, const Grads* grads, const float* dX, const int32_t* users, const int64_t* act,
                                    const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* lens, int R, DwList& dwl,
                                    const SlotScratch& sc, hipStream_t s) {
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
