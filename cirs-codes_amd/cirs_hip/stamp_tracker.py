"""Device engine of the attention-pool state tracker (csrc/stamp_tracker.hip): the input slots of the other trackers, STAMP's attention over
the window of the last `window_size` item slots (a general-interest query m_s, a last-click query m_t, a sigmoid gate network without softmax),
h_p = x_0 + tanh(A m_a + b_A) * tanh(B m_t + b_B), the same decoder.  One launch per step and nothing carried besides the stored slots; the
gradient arrives through cirs_stamp_tracker_backward (no sequential pass).  The engine itself is gru_tracker.DeviceRecurrentTracker with the
STAMP structs and entry points, so the rollout, the learner and the plugin classes drive it as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .gru_tracker import TOP_FIELDS, DeviceRecurrentTracker

DIM_MODEL = 32
MAX_LEN = 4096
MAX_WINDOW = abi.STAMP_MAX_WINDOW      # one 16-row tile
# the struct members of the nine tensors between the shared ones and the decoder, and their state_dict names
STAMP_FIELDS = [("attn_b", "attn.bias"), ("w1", "attn.w1.weight"), ("w2", "attn.w2.weight"), ("w3", "attn.w3.weight"), ("w0", "attn.w0.weight"),
                ("mlp_a_w", "mlp_a.weight"), ("mlp_a_b", "mlp_a.bias"), ("mlp_b_w", "mlp_b.weight"), ("mlp_b_b", "mlp_b.bias")]


def check_stamp_shape(dim_model, dim_state, window_size, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    if int(dim_model) != DIM_MODEL:
        raise ValueError(f"the STAMP tracker is built for dim_model == {DIM_MODEL}, got {dim_model}")
    if not 1 <= int(dim_state) <= 32:
        raise ValueError(f"the STAMP tracker is built for dim_state in 1..32, got {dim_state}")
    if not 1 <= int(window_size) <= MAX_WINDOW:
        raise ValueError(f"the STAMP tracker is built for window_size in 1..{MAX_WINDOW}, got {window_size}")
    if max_len is not None and not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError(f"the STAMP tracker is built for max_len (MAX_TURN + 1) in 1..{MAX_LEN}, got {max_len}")


def stamp_param_shapes(n_users, n_items, dim_model=32, dim_state=20):
    """Ordered {state_dict name: shape} of the 17 trainable tensors: the other trackers' names for what all share, then the attention
    (nn.Linear(D, D, bias=False) under attn.w1 / attn.w2 / attn.w3, the vector attn.bias, nn.Linear(D, 1, bias=False) under attn.w0) and the
    two read-out layers (nn.Linear(D, D) under mlp_a and mlp_b), decoder last -- in the order a torch module with these children lists them in
    its state_dict: attn's own tensor (attn.bias) before its children's.  The window has no parameters."""
    D, S = dim_model, dim_state
    return {"embedding_dict.feat_user.weight": (n_users, D), "embedding_dict.feat_item.weight": (n_items, D),
            "ffn_user.weight": (D, D), "ffn_user.bias": (D,), "fnn_gate.weight": (D, D + 1), "fnn_gate.bias": (D,),
            "attn.bias": (D,), "attn.w1.weight": (D, D), "attn.w2.weight": (D, D), "attn.w3.weight": (D, D), "attn.w0.weight": (1, D),
            "mlp_a.weight": (D, D), "mlp_a.bias": (D,), "mlp_b.weight": (D, D), "mlp_b.bias": (D,),
            "decoder.weight": (S, D), "decoder.bias": (S,)}


def init_stamp_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what all trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the attention
    and the read-out with torch's default nn.Linear init from a generator stream of their own, attn.bias zero.  torch modules are parameter
    factories only."""
    from .engine import init_tracker_params
    shared = init_tracker_params(n_users, n_items, 1, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    shapes = stamp_param_shapes(n_users, n_items, dim_model, dim_state)
    p = {k: shared[k] for k in shapes if k in shared}
    D = dim_model
    torch_state = torch.random.get_rng_state()
    torch.manual_seed(int(seed) + 0x7374616D)      # a stream of its own: the shared tensors do not move with the attention
    try:
        mods = {"attn.w1": torch.nn.Linear(D, D, bias=False), "attn.w2": torch.nn.Linear(D, D, bias=False), "attn.w3": torch.nn.Linear(D, D, bias=False),
                "attn.w0": torch.nn.Linear(D, 1, bias=False), "mlp_a": torch.nn.Linear(D, D), "mlp_b": torch.nn.Linear(D, D)}
        for name, m in mods.items():
            for k, v in m.state_dict().items():
                p[f"{name}.{k}"] = v.detach().clone().float()
        p["attn.bias"] = torch.zeros(D)
    finally:
        torch.random.set_rng_state(torch_state)
    return {k: p[k] for k in shapes}


class DeviceStampTracker(DeviceRecurrentTracker):
    """`params` maps state_dict names (stamp_param_shapes) to device tensors.  Carries nothing: the window is read from x_hist."""
    CFG, WEIGHTS, STATE, LAYER_FIELDS, ENTRY = abi.StampCfg, abi.StampWeights, abi.StampState, (), "cirs_stamp_tracker"
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_stamp", "STAMP"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, window_size=10,
                 device="cuda"):
        self.window_size = int(window_size)
        self._max_len = max_turn + 1
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=0, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_stamp_shape(dim_model, dim_state, self.window_size, self._max_len)
        return {"window": self.window_size}

    def _weights(self, tensors):
        """cirs_stamp_weights (or cirs_stamp_grads: same layout): weights_struct knows the shared fields and per-layer cells only."""
        w = self.WEIGHTS()
        for f, name in TOP_FIELDS + STAMP_FIELDS:
            t = tensors[name]
            assert t.dtype == torch.float32 and t.is_contiguous(), name
            setattr(w, f, t.data_ptr())
        return w
