"""Device engine of the LSTM state tracker (csrc/lstm_tracker.hip): the input slots of the GRU tracker, a torch.nn.LSTM(D, D, L)
recurrence carried as L x 32 floats of h and of c per env, the same decoder.  One launch per step; the gradient arrives through
cirs_lstm_tracker_backward (back-propagation through time through h and c, recomputed from the stored slots).  The engine itself is
gru_tracker.DeviceRecurrentTracker with the LSTM's structs and entry points, so the rollout, the learner and the plugin classes
drive it as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .gru_tracker import DeviceRecurrentTracker

LAYER_FIELDS = [("w_ih", "lstm.weight_ih_l{}"), ("w_hh", "lstm.weight_hh_l{}"), ("b_ih", "lstm.bias_ih_l{}"), ("b_hh", "lstm.bias_hh_l{}")]
DIM_MODEL = 32
MAX_LAYERS = abi.LSTM_MAX_LAYERS


def check_lstm_shape(dim_model, dim_state, nlayers):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    if int(dim_model) != DIM_MODEL:
        raise ValueError(f"the LSTM tracker is built for dim_model == {DIM_MODEL}, got {dim_model}")
    if not 1 <= int(dim_state) <= 32:
        raise ValueError(f"the LSTM tracker is built for dim_state in 1..32, got {dim_state}")
    if int(nlayers) not in (1, 2):
        raise ValueError(f"the LSTM tracker is built for nlayers in {{1, 2}}, got {nlayers}")


def lstm_param_shapes(n_users, n_items, dim_model=32, dim_state=20, nlayers=1):
    """Ordered {state_dict name: shape} of the trainable tensors, embeddings first, decoder last: the other trackers' names for what all
    share, torch.nn.LSTM's (under `lstm.`) for the recurrence, so that the lstm.* entries load into nn.LSTM(dim_model, dim_model,
    nlayers) by name.  Both bias vectors are parameters, as in torch."""
    D, S = dim_model, dim_state
    sh = {"embedding_dict.feat_user.weight": (n_users, D), "embedding_dict.feat_item.weight": (n_items, D),
          "ffn_user.weight": (D, D), "ffn_user.bias": (D,), "fnn_gate.weight": (D, D + 1), "fnn_gate.bias": (D,)}
    for l in range(nlayers):
        sh.update({f"lstm.weight_ih_l{l}": (4 * D, D), f"lstm.weight_hh_l{l}": (4 * D, D), f"lstm.bias_ih_l{l}": (4 * D,),
                   f"lstm.bias_hh_l{l}": (4 * D,)})
    sh.update({"decoder.weight": (S, D), "decoder.bias": (S,)})
    return sh


def init_lstm_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, nlayers=1, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what the trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the LSTM
    tensors with torch's default U(-1/sqrt(D), 1/sqrt(D)) from a generator stream of their own; the global torch RNG state is restored."""
    from .engine import init_tracker_params
    shared = init_tracker_params(n_users, n_items, 1, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    p = {k: v for k, v in shared.items() if not k.startswith("transformer_encoder.") and k != "pos_encoder.pe"}
    torch_state = torch.random.get_rng_state()
    torch.manual_seed(int(seed) + 0x6c73)      # a stream of its own: the shared tensors do not move when nlayers changes
    try:
        lstm = torch.nn.LSTM(dim_model, dim_model, nlayers)
        for k, v in lstm.state_dict().items():
            p["lstm." + k] = v.detach().clone().float()
    finally:
        torch.random.set_rng_state(torch_state)
    return {k: p[k] for k in lstm_param_shapes(n_users, n_items, dim_model, dim_state, nlayers)}


class DeviceLstmTracker(DeviceRecurrentTracker):
    """`params` maps state_dict names (lstm_param_shapes) to device tensors.  Carries c [nlayers, B, 32] next to h."""
    CFG, WEIGHTS, STATE, LAYER_FIELDS, ENTRY, check_shape = abi.LstmCfg, abi.LstmWeights, abi.LstmState, LAYER_FIELDS, "cirs_lstm_tracker", check_lstm_shape
    CARRY = ("h", "c")
    COLLECT, NAME = "cirs_rollout_collect_lstm", "LSTM"
