"""Device engine of the recurrent state tracker (csrc/gru_tracker.hip): the input slots of the Transformer tracker, a
torch.nn.GRU(D, D, L) recurrence carried as L x 32 floats per env, the same decoder.  One launch per step; the gradient arrives
through cirs_gru_tracker_backward (back-propagation through time, recomputed from the stored slots).  The engine itself is
slot_engine.DeviceSlotTracker with the GRU's structs and entry points: the engine surface of cirs_hip.tracker.DeviceTracker, so the
rollout, the learner and the plugin classes drive either."""
from typing import Dict

import torch

from . import abi
from .slot_engine import DeviceSlotTracker, add_module_params, check_dims, decoder_shapes, head_shapes, own_stream, shared_init_params

MAX_LAYERS = abi.GRU_MAX_LAYERS


def check_gru_shape(dim_model, dim_state, nlayers):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("GRU", dim_model, dim_state)
    if int(nlayers) not in (1, 2):
        raise ValueError(f"the GRU tracker is built for nlayers in {{1, 2}}, got {nlayers}")


def gru_param_shapes(n_users, n_items, dim_model=32, dim_state=20, nlayers=1):
    """Ordered {state_dict name: shape} of the trainable tensors: the Transformer tracker's names for what both share, torch.nn.GRU's
    (under `gru.`) for the recurrence, so that the gru.* entries load into nn.GRU(dim_model, dim_model, nlayers) by name."""
    D = dim_model
    sh = head_shapes(n_users, n_items, D)
    for l in range(nlayers):
        sh.update({f"gru.weight_ih_l{l}": (3 * D, D), f"gru.weight_hh_l{l}": (3 * D, D), f"gru.bias_ih_l{l}": (3 * D,),
                   f"gru.bias_hh_l{l}": (3 * D,)})
    sh.update(decoder_shapes(D, dim_state))
    return sh


def init_gru_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, nlayers=1, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what both trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the GRU
    tensors with torch's default U(-1/sqrt(D), 1/sqrt(D)) from a generator seeded by `seed`.  torch modules are parameter factories only."""
    p = shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std)
    with own_stream(int(seed) + 0x6772):      # the shared tensors do not move when nlayers changes
        add_module_params(p, {"gru": torch.nn.GRU(dim_model, dim_model, nlayers)})
    return {k: p[k] for k in gru_param_shapes(n_users, n_items, dim_model, dim_state, nlayers)}


class DeviceGruTracker(DeviceSlotTracker):
    """`params` maps state_dict names (gru_param_shapes) to device tensors."""
    CFG, WEIGHTS, STATE, ENTRY, check_shape, param_shapes = abi.GruCfg, abi.GruWeights, abi.GruState, "cirs_gru_tracker", check_gru_shape, gru_param_shapes
    FIELDS = [("layer[].w_ih", "gru.weight_ih_l{}"), ("layer[].w_hh", "gru.weight_hh_l{}"), ("layer[].b_ih", "gru.bias_ih_l{}"),
              ("layer[].b_hh", "gru.bias_hh_l{}")]
    COLLECT, NAME = "cirs_rollout_collect_gru", "GRU"
