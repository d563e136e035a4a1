"""Device engine of the attention-pool state tracker (csrc/stamp_tracker.hip): the input slots of the other trackers, STAMP's attention over
the window of the last `window_size` item slots (a general-interest query m_s, a last-click query m_t, a sigmoid gate network without softmax),
h_p = x_0 + tanh(A m_a + b_A) * tanh(B m_t + b_B), the same decoder.  One launch per step and nothing carried besides the stored slots; the
gradient arrives through cirs_stamp_tracker_backward (no sequential pass).  The engine itself is slot_engine.DeviceSlotTracker with the
STAMP structs and entry points, so the rollout, the learner and the plugin classes drive it as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .slot_engine import (DeviceSlotTracker, add_module_params, check_dims, check_max_len, decoder_shapes, head_shapes, own_stream,
                          shared_init_params)

MAX_WINDOW = abi.STAMP_MAX_WINDOW      # one 16-row tile


def check_stamp_shape(dim_model, dim_state, window_size, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("STAMP", dim_model, dim_state)
    if not 1 <= int(window_size) <= MAX_WINDOW:
        raise ValueError(f"the STAMP tracker is built for window_size in 1..{MAX_WINDOW}, got {window_size}")
    check_max_len("STAMP", max_len)


def stamp_param_shapes(n_users, n_items, dim_model=32, dim_state=20):
    """Ordered {state_dict name: shape} of the 17 trainable tensors: the other trackers' names for what all share, then the attention
    (nn.Linear(D, D, bias=False) under attn.w1 / attn.w2 / attn.w3, the vector attn.bias, nn.Linear(D, 1, bias=False) under attn.w0) and the
    two read-out layers (nn.Linear(D, D) under mlp_a and mlp_b), decoder last -- in the order a torch module with these children lists them in
    its state_dict: attn's own tensor (attn.bias) before its children's.  The window has no parameters."""
    D = dim_model
    return {**head_shapes(n_users, n_items, D),
            "attn.bias": (D,), "attn.w1.weight": (D, D), "attn.w2.weight": (D, D), "attn.w3.weight": (D, D), "attn.w0.weight": (1, D),
            "mlp_a.weight": (D, D), "mlp_a.bias": (D,), "mlp_b.weight": (D, D), "mlp_b.bias": (D,),
            **decoder_shapes(D, dim_state)}


def init_stamp_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what all trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the attention
    and the read-out with torch's default nn.Linear init from a generator stream of their own, attn.bias zero.  torch modules are parameter
    factories only."""
    p = shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std)
    D = dim_model
    with own_stream(int(seed) + 0x7374616D):      # the shared tensors do not move with the attention
        mods = {"attn.w1": torch.nn.Linear(D, D, bias=False), "attn.w2": torch.nn.Linear(D, D, bias=False), "attn.w3": torch.nn.Linear(D, D, bias=False),
                "attn.w0": torch.nn.Linear(D, 1, bias=False), "mlp_a": torch.nn.Linear(D, D), "mlp_b": torch.nn.Linear(D, D)}
        add_module_params(p, mods)
        p["attn.bias"] = torch.zeros(D)
    return {k: p[k] for k in stamp_param_shapes(n_users, n_items, dim_model, dim_state)}


class DeviceStampTracker(DeviceSlotTracker):
    """`params` maps state_dict names (stamp_param_shapes) to device tensors.  Carries nothing: the window is read from x_hist."""
    CFG, WEIGHTS, STATE, ENTRY, param_shapes = abi.StampCfg, abi.StampWeights, abi.StampState, "cirs_stamp_tracker", stamp_param_shapes
    FIELDS = [("attn_b", "attn.bias"), ("w1", "attn.w1.weight"), ("w2", "attn.w2.weight"), ("w3", "attn.w3.weight"), ("w0", "attn.w0.weight"),
              ("mlp_a_w", "mlp_a.weight"), ("mlp_a_b", "mlp_a.bias"), ("mlp_b_w", "mlp_b.weight"), ("mlp_b_b", "mlp_b.bias")]
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_stamp", "STAMP"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, window_size=10,
                 device="cuda"):
        self.window_size = int(window_size)
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=0, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_stamp_shape(dim_model, dim_state, self.window_size, self.max_len)
        return {"window": self.window_size}

    def _shape_kw(self):
        return {}      # the window has no parameters
