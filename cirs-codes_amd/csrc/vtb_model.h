// vtb_model.h -- the rules of cirs_vtb_model_cfg that the rollout (vtb_rollout.hip) and the learner (vtb_learn.hip) share.
#pragma once
#include "common.h"

namespace cirs {

// max_turn (>= 1, checked by the caller) is the stage's collect length.  The capacity limits are not here: the two stages' kernels differ,
// each file checks its own, and the rollout's are the tighter ones (d_hid <= 256, dim_state <= 64, nhead * max_len <= 2048; learner 1024, 128).
inline int vtb_validate_model(const cirs_vtb_model_cfg* m, int max_turn) {
    CIRS_REQUIRE(m->dim_model == CIRS_VTB_ACTION_DIM,
                 "dim_model must be 27: the input slot is sigmoid(fnn_gate([r, a])) * a with the 27 action features");
    CIRS_REQUIRE(m->nhead >= 1 && m->dim_model % m->nhead == 0, "dim_model must be a multiple of nhead");
    CIRS_REQUIRE(m->nlayers >= 1 && m->nlayers <= CIRS_VTB_RO_MAX_LAYERS, "nlayers must lie in [1, 4]");
    CIRS_REQUIRE(max_turn <= m->max_len - 1, "max_turn exceeds the tracker's MAX_TURN - 1 (positions 0..max_turn need pe / cache rows)");
    CIRS_REQUIRE(m->n_hidden >= 1 && m->n_hidden <= CIRS_VTB_RO_MAX_HIDDEN, "the actor trunk must have 1..3 hidden layers");
    for (int i = 0; i < m->n_hidden; ++i) CIRS_REQUIRE(m->hidden[i] >= 1 && m->hidden[i] <= 128, "actor hidden widths must lie in [1, 128]");
    CIRS_REQUIRE(m->dropout_p >= 0.f && m->dropout_p < 1.f, "dropout_p must lie in [0, 1)");
    CIRS_REQUIRE(m->drop_env_base >= 0, "drop_env_base must be >= 0");
    return CIRS_OK;
}

}  // namespace cirs
