"""Device engine of the pooled-window state tracker (csrc/avg_tracker.hip): the input slots of the other trackers, h_p = x_0 + the mean
of the last `window_size` item slots, the same decoder.  One launch per step, no cell and nothing carried besides the stored slots; the
gradient arrives through cirs_avg_tracker_backward (the pooling is linear: no sequential pass).  The engine itself is
slot_engine.DeviceSlotTracker with the Avg structs and entry points, so the rollout, the learner and the plugin classes drive it
as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .slot_engine import DeviceSlotTracker, check_dims, check_max_len, decoder_shapes, head_shapes, shared_init_params


def check_avg_shape(dim_model, dim_state, window_size, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("Avg", dim_model, dim_state)
    if int(window_size) < 1:
        raise ValueError(f"the Avg tracker needs window_size >= 1, got {window_size}")
    check_max_len("Avg", max_len)


def avg_param_shapes(n_users, n_items, dim_model=32, dim_state=20):
    """Ordered {state_dict name: shape} of the trainable tensors, embeddings first, decoder last: the other trackers' names; the
    pooling has no parameters."""
    return {**head_shapes(n_users, n_items, dim_model), **decoder_shapes(dim_model, dim_state)}


def init_avg_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: every tensor exactly as engine.init_tracker_params draws it (same seed -> same tensors)."""
    p = shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std)
    return {k: p[k] for k in avg_param_shapes(n_users, n_items, dim_model, dim_state)}


class DeviceAvgTracker(DeviceSlotTracker):
    """`params` maps state_dict names (avg_param_shapes) to device tensors.  Carries nothing: the window is read from x_hist."""
    CFG, WEIGHTS, STATE, ENTRY, param_shapes = abi.AvgCfg, abi.AvgWeights, abi.AvgState, "cirs_avg_tracker", avg_param_shapes
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_avg", "Avg"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, window_size=10,
                 device="cuda"):
        self.window_size = int(window_size)
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=0, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_avg_shape(dim_model, dim_state, self.window_size, self.max_len)
        return {"window": self.window_size}

    def _shape_kw(self):
        return {}      # the window has no parameters
