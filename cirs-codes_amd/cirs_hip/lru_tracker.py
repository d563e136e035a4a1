"""Device engine of the linear-recurrence state tracker (csrc/lru_tracker.hip): the input slots of the other trackers, a linear recurrent
unit (a diagonal complex recurrence h_p = lambda * h_{p-1} + gamma * (W_in x_p + b_in), carried as 64 floats per env whatever the position),
a real read-out, LayerNorm, the 32 -> 128 -> 32 GELU feed-forward block of the FMLP tracker, LayerNorm, the same decoder.  One launch per
step, at a cost that does not depend on the position; the gradient arrives through cirs_lru_tracker_backward (every dense product over all
buffer rows at once, one complex multiply-add per position in the two sequential scans).  The engine itself is
slot_engine.DeviceSlotTracker with the LRU structs and entry points, so the rollout, the learner and the plugin classes drive it as
they drive the GRU's."""
import math
from typing import Dict

import torch

from . import abi
from .slot_engine import DeviceSlotTracker, add_module_params, check_dims, check_max_len, decoder_shapes, head_shapes, own_stream

MAX_LAYERS = abi.LRU_MAX_LAYERS
HIDDEN = abi.LRU_HIDDEN
# the state_dict names of the fifteen tensors between the shared ones and the decoder, in the order of abi.LRU_MEMBERS
LRU_NAMES = ("lru.nu_log", "lru.theta_log", "lru.gamma_log", "lru.in_proj.weight", "lru.in_proj.bias", "lru.out_proj.weight", "lru.out_proj.bias",
             "lru.ln.weight", "lru.ln.bias", "ffn.dense_1.weight", "ffn.dense_1.bias", "ffn.dense_2.weight", "ffn.dense_2.bias", "ffn.ln.weight",
             "ffn.ln.bias")


def check_lru_shape(dim_model, dim_state, nlayers=1, d_hid=HIDDEN, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("LRU", dim_model, dim_state)
    if int(nlayers) != MAX_LAYERS:
        raise ValueError(f"the LRU tracker is built for nlayers == {MAX_LAYERS} (one recurrence layer), got {nlayers}")
    if int(d_hid) != HIDDEN:
        raise ValueError(f"the LRU tracker is built for d_hid == {HIDDEN}, got {d_hid}")
    check_max_len("LRU", max_len)


def lru_param_shapes(n_users, n_items, dim_model=32, dim_state=20, nlayers=1):
    """Ordered {state_dict name: shape} of the 23 trainable tensors: the other trackers' names for what all share, then the recurrence under
    `lru.` (the three log vectors as plain parameters; nn.Linear(D, 2 D) under lru.in_proj, nn.Linear(2 D, D) under lru.out_proj,
    nn.LayerNorm(D) under lru.ln), the feed-forward block under `ffn.` (nn.Linear(D, 128), nn.Linear(128, D), nn.LayerNorm(D)), decoder last."""
    D = dim_model
    return {**head_shapes(n_users, n_items, D),
            "lru.nu_log": (D,), "lru.theta_log": (D,), "lru.gamma_log": (D,),
            "lru.in_proj.weight": (2 * D, D), "lru.in_proj.bias": (2 * D,), "lru.out_proj.weight": (D, 2 * D), "lru.out_proj.bias": (D,),
            "lru.ln.weight": (D,), "lru.ln.bias": (D,),
            "ffn.dense_1.weight": (HIDDEN, D), "ffn.dense_1.bias": (HIDDEN,), "ffn.dense_2.weight": (D, HIDDEN), "ffn.dense_2.bias": (D,),
            "ffn.ln.weight": (D,), "ffn.ln.bias": (D,),
            **decoder_shapes(D, dim_state)}


def init_lru_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, nlayers=1, init_std=1e-4, r_min=0.0, r_max=1.0,
                            max_phase=2 * math.pi) -> Dict[str, torch.Tensor]:
    """Fresh parameters: the shared tensors and the decoder exactly as gru_tracker.init_gru_tracker_params draws them at one layer (same seed
    -> same tensors); from a generator stream of their own the ring initialisation of the LRU paper -- u1, u2 ~ U(0, 1), |lambda|^2 = u1
    (r_max^2 - r_min^2) + r_min^2, nu_log = log(-1/2 log |lambda|^2), theta_log = log(max_phase u2), gamma_log = 1/2 log(1 - |lambda|^2), with u1
    clamped to [1e-6, 1 - 1e-6] and u2 to at least 1e-6 so that every log is finite -- and the Linear / LayerNorm tensors by torch's defaults.
    torch modules are parameter factories only; the caller's RNG state is restored."""
    from .gru_tracker import init_gru_tracker_params
    p = init_gru_tracker_params(n_users, n_items, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    D = dim_model
    with own_stream(int(seed) + 0x6C7275):      # nothing shared moves with the recurrence
        u1 = torch.rand(D).clamp(1e-6, 1 - 1e-6)
        u2 = torch.rand(D).clamp(min=1e-6)
        mod2 = u1 * (r_max ** 2 - r_min ** 2) + r_min ** 2
        p["lru.nu_log"] = torch.log(-0.5 * torch.log(mod2))
        p["lru.theta_log"] = torch.log(max_phase * u2)
        p["lru.gamma_log"] = 0.5 * torch.log(1 - mod2)
        add_module_params(p, {"lru.in_proj": torch.nn.Linear(D, 2 * D), "lru.out_proj": torch.nn.Linear(2 * D, D), "lru.ln": torch.nn.LayerNorm(D),
                              "ffn.dense_1": torch.nn.Linear(D, HIDDEN), "ffn.dense_2": torch.nn.Linear(HIDDEN, D), "ffn.ln": torch.nn.LayerNorm(D)})
    return {k: p[k].float() for k in lru_param_shapes(n_users, n_items, dim_model, dim_state)}


class DeviceLruTracker(DeviceSlotTracker):
    """`params` maps state_dict names (lru_param_shapes) to device tensors.  Carries the complex state as h_re and h_im, [1, n_env, 32] each."""
    CFG, WEIGHTS, STATE, ENTRY, check_shape, param_shapes = abi.LruCfg, abi.LruWeights, abi.LruState, "cirs_lru_tracker", check_lru_shape, lru_param_shapes
    FIELDS = list(zip(abi.LRU_MEMBERS, LRU_NAMES))
    CARRY = ("h_re", "h_im")
    COLLECT, NAME = "cirs_rollout_collect_lru", "LRU"

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_lru_shape(dim_model, dim_state, nlayers, HIDDEN, self.max_len)
        return {"nlayers": nlayers}
