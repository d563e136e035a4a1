"""Device engine of the filter-MLP state tracker (csrc/fmlp_tracker.hip): the input slots of the other trackers, FMLP-Rec's layers over the
tile of the last `window_size` item slots (a learned per-channel circular filter whose parameters live in the frequency domain, then a
LayerNorm / GELU feed-forward block of width 128), h_p = x_0 + the top layer's newest row, the same decoder.  One launch per step and nothing
carried besides the stored slots; the gradient arrives through cirs_fmlp_tracker_backward (no sequential pass).  The engine itself is
slot_engine.DeviceSlotTracker with the FMLP structs and entry points, so the rollout, the learner and the plugin classes drive it as
they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .slot_engine import (DeviceSlotTracker, add_module_params, check_dims, check_max_len, decoder_shapes, head_shapes, own_stream,
                          shared_init_params)

MAX_WINDOW = abi.FMLP_MAX_WINDOW      # one 16-row tile
MAX_LAYERS = abi.FMLP_MAX_LAYERS
HIDDEN = abi.FMLP_HIDDEN
# the state_dict names of a layer's nine tensors, in the order of abi.FMLP_LAYER_MEMBERS
FMLP_LAYER_NAMES = ("layers.{}.filter.complex_weight", "layers.{}.filter.ln.weight", "layers.{}.filter.ln.bias", "layers.{}.ffn.dense_1.weight",
                    "layers.{}.ffn.dense_1.bias", "layers.{}.ffn.dense_2.weight", "layers.{}.ffn.dense_2.bias", "layers.{}.ffn.ln.weight",
                    "layers.{}.ffn.ln.bias")


def check_fmlp_shape(dim_model, dim_state, window_size, nlayers, d_hid=HIDDEN, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("FMLP", dim_model, dim_state)
    if not 1 <= int(window_size) <= MAX_WINDOW:
        raise ValueError(f"the FMLP tracker is built for window_size in 1..{MAX_WINDOW}, got {window_size}")
    if int(nlayers) not in (1, 2):
        raise ValueError(f"the FMLP tracker is built for nlayers in {{1, 2}}, got {nlayers}")
    if int(d_hid) != HIDDEN:
        raise ValueError(f"the FMLP tracker is built for d_hid == {HIDDEN}, got {d_hid}")
    check_max_len("FMLP", max_len)


def fmlp_param_shapes(n_users, n_items, dim_model=32, dim_state=20, window_size=10, nlayers=2):
    """Ordered {state_dict name: shape} of the 8 + 9 L trainable tensors: the other trackers' names for what all share, then per layer the
    filter (complex_weight [W//2+1, D, 2]: real and imaginary part, what torch.view_as_complex reads; nn.LayerNorm(D) under filter.ln) and the
    feed-forward block (nn.Linear(D, 128) under ffn.dense_1, nn.Linear(128, D) under ffn.dense_2, nn.LayerNorm(D) under ffn.ln), decoder last
    -- in the order a torch module with these children lists them in its state_dict.  The shape of complex_weight depends on the window."""
    D, W = dim_model, int(window_size)
    sh = head_shapes(n_users, n_items, D)
    for l in range(int(nlayers)):
        sh.update({f"layers.{l}.filter.complex_weight": (W // 2 + 1, D, 2), f"layers.{l}.filter.ln.weight": (D,), f"layers.{l}.filter.ln.bias": (D,),
                   f"layers.{l}.ffn.dense_1.weight": (HIDDEN, D), f"layers.{l}.ffn.dense_1.bias": (HIDDEN,),
                   f"layers.{l}.ffn.dense_2.weight": (D, HIDDEN), f"layers.{l}.ffn.dense_2.bias": (D,),
                   f"layers.{l}.ffn.ln.weight": (D,), f"layers.{l}.ffn.ln.bias": (D,)})
    sh.update(decoder_shapes(D, dim_state))
    return sh


def init_fmlp_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, window_size=10, nlayers=2,
                             init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what all trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors); from a generator
    stream of their own complex_weight ~ 0.02 N(0, 1) (FMLP-Rec's) and the Linear / LayerNorm tensors by torch's defaults.  torch modules are
    parameter factories only; the caller's RNG state is restored."""
    p = shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std)
    D, W = dim_model, int(window_size)
    with own_stream(int(seed) + 0x666D6C70):      # the shared tensors do not move with the layers
        for l in range(int(nlayers)):
            p[f"layers.{l}.filter.complex_weight"] = 0.02 * torch.randn(W // 2 + 1, D, 2)
            mods = {"filter.ln": torch.nn.LayerNorm(D), "ffn.dense_1": torch.nn.Linear(D, HIDDEN), "ffn.dense_2": torch.nn.Linear(HIDDEN, D),
                    "ffn.ln": torch.nn.LayerNorm(D)}
            add_module_params(p, mods, f"layers.{l}.")
    return {k: p[k] for k in fmlp_param_shapes(n_users, n_items, dim_model, dim_state, window_size, nlayers)}


class DeviceFmlpTracker(DeviceSlotTracker):
    """`params` maps state_dict names (fmlp_param_shapes) to device tensors.  Carries nothing: the tile is read from x_hist."""
    CFG, WEIGHTS, STATE, ENTRY, param_shapes = abi.FmlpCfg, abi.FmlpWeights, abi.FmlpState, "cirs_fmlp_tracker", fmlp_param_shapes
    FIELDS = [(m + "[]", name) for m, name in zip(abi.FMLP_LAYER_MEMBERS, FMLP_LAYER_NAMES)]      # every layer member is an array over the layers
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_fmlp", "FMLP"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, window_size=10,
                 nlayers=2, device="cuda"):
        self.window_size = int(window_size)
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=nlayers, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_fmlp_shape(dim_model, dim_state, self.window_size, nlayers, HIDDEN, self.max_len)
        return {"window": self.window_size, "nlayers": int(nlayers)}

    def _shape_kw(self):
        return {"window_size": self.window_size, "nlayers": self.nlayers}
