"""Device engine of the LSTM state tracker (csrc/lstm_tracker.hip): the input slots of the GRU tracker, a torch.nn.LSTM(D, D, L)
recurrence carried as L x 32 floats of h and of c per env, the same decoder.  One launch per step; the gradient arrives through
cirs_lstm_tracker_backward (back-propagation through time through h and c, recomputed from the stored slots).  The engine itself is
slot_engine.DeviceSlotTracker with the LSTM's structs and entry points, so the rollout, the learner and the plugin classes
drive it as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .slot_engine import DeviceSlotTracker, add_module_params, check_dims, decoder_shapes, head_shapes, own_stream, shared_init_params

MAX_LAYERS = abi.LSTM_MAX_LAYERS


def check_lstm_shape(dim_model, dim_state, nlayers):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("LSTM", dim_model, dim_state)
    if int(nlayers) not in (1, 2):
        raise ValueError(f"the LSTM tracker is built for nlayers in {{1, 2}}, got {nlayers}")


def lstm_param_shapes(n_users, n_items, dim_model=32, dim_state=20, nlayers=1):
    """Ordered {state_dict name: shape} of the trainable tensors, embeddings first, decoder last: the other trackers' names for what all
    share, torch.nn.LSTM's (under `lstm.`) for the recurrence, so that the lstm.* entries load into nn.LSTM(dim_model, dim_model,
    nlayers) by name.  Both bias vectors are parameters, as in torch."""
    D = dim_model
    sh = head_shapes(n_users, n_items, D)
    for l in range(nlayers):
        sh.update({f"lstm.weight_ih_l{l}": (4 * D, D), f"lstm.weight_hh_l{l}": (4 * D, D), f"lstm.bias_ih_l{l}": (4 * D,),
                   f"lstm.bias_hh_l{l}": (4 * D,)})
    sh.update(decoder_shapes(D, dim_state))
    return sh


def init_lstm_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, nlayers=1, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what the trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the LSTM
    tensors with torch's default U(-1/sqrt(D), 1/sqrt(D)) from a generator stream of their own; the global torch RNG state is restored."""
    p = shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std)
    with own_stream(int(seed) + 0x6c73):      # the shared tensors do not move when nlayers changes
        add_module_params(p, {"lstm": torch.nn.LSTM(dim_model, dim_model, nlayers)})
    return {k: p[k] for k in lstm_param_shapes(n_users, n_items, dim_model, dim_state, nlayers)}


class DeviceLstmTracker(DeviceSlotTracker):
    """`params` maps state_dict names (lstm_param_shapes) to device tensors.  Carries c [nlayers, B, 32] next to h."""
    CFG, WEIGHTS, STATE, ENTRY, check_shape, param_shapes = abi.LstmCfg, abi.LstmWeights, abi.LstmState, "cirs_lstm_tracker", check_lstm_shape, lstm_param_shapes
    FIELDS = [("layer[].w_ih", "lstm.weight_ih_l{}"), ("layer[].w_hh", "lstm.weight_hh_l{}"), ("layer[].b_ih", "lstm.bias_ih_l{}"),
              ("layer[].b_hh", "lstm.bias_hh_l{}")]
    CARRY = ("h", "c")
    COLLECT, NAME = "cirs_rollout_collect_lstm", "LSTM"
