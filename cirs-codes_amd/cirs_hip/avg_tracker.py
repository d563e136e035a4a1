"""Device engine of the pooled-window state tracker (csrc/avg_tracker.hip): the input slots of the other trackers, h_p = x_0 + the mean
of the last `window_size` item slots, the same decoder.  One launch per step, no cell and nothing carried besides the stored slots; the
gradient arrives through cirs_avg_tracker_backward (the pooling is linear: no sequential pass).  The engine itself is
gru_tracker.DeviceRecurrentTracker with the Avg structs and entry points, so the rollout, the learner and the plugin classes drive it
as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .gru_tracker import DeviceRecurrentTracker

DIM_MODEL = 32
MAX_LEN = 4096


def check_avg_shape(dim_model, dim_state, window_size, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    if int(dim_model) != DIM_MODEL:
        raise ValueError(f"the Avg tracker is built for dim_model == {DIM_MODEL}, got {dim_model}")
    if not 1 <= int(dim_state) <= 32:
        raise ValueError(f"the Avg tracker is built for dim_state in 1..32, got {dim_state}")
    if int(window_size) < 1:
        raise ValueError(f"the Avg tracker needs window_size >= 1, got {window_size}")
    if max_len is not None and not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError(f"the Avg tracker is built for max_len (MAX_TURN + 1) in 1..{MAX_LEN}, got {max_len}")


def avg_param_shapes(n_users, n_items, dim_model=32, dim_state=20):
    """Ordered {state_dict name: shape} of the trainable tensors, embeddings first, decoder last: the other trackers' names; the
    pooling has no parameters."""
    D, S = dim_model, dim_state
    return {"embedding_dict.feat_user.weight": (n_users, D), "embedding_dict.feat_item.weight": (n_items, D),
            "ffn_user.weight": (D, D), "ffn_user.bias": (D,), "fnn_gate.weight": (D, D + 1), "fnn_gate.bias": (D,),
            "decoder.weight": (S, D), "decoder.bias": (S,)}


def init_avg_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: every tensor exactly as engine.init_tracker_params draws it (same seed -> same tensors)."""
    from .engine import init_tracker_params
    shared = init_tracker_params(n_users, n_items, 1, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    return {k: shared[k] for k in avg_param_shapes(n_users, n_items, dim_model, dim_state)}


class DeviceAvgTracker(DeviceRecurrentTracker):
    """`params` maps state_dict names (avg_param_shapes) to device tensors.  Carries nothing: the window is read from x_hist."""
    CFG, WEIGHTS, STATE, LAYER_FIELDS, ENTRY = abi.AvgCfg, abi.AvgWeights, abi.AvgState, (), "cirs_avg_tracker"
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_avg", "Avg"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, window_size=10,
                 device="cuda"):
        self.window_size = int(window_size)
        self._max_len = max_turn + 1
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=0, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_avg_shape(dim_model, dim_state, self.window_size, self._max_len)
        return {"window": self.window_size}
