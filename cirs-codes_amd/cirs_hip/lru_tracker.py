"""Device engine of the linear-recurrence state tracker (csrc/lru_tracker.hip): the input slots of the other trackers, a linear recurrent
unit (a diagonal complex recurrence h_p = lambda * h_{p-1} + gamma * (W_in x_p + b_in), carried as 64 floats per env whatever the position),
a real read-out, LayerNorm, the 32 -> 128 -> 32 GELU feed-forward block of the FMLP tracker, LayerNorm, the same decoder.  One launch per
step, at a cost that does not depend on the position; the gradient arrives through cirs_lru_tracker_backward (every dense product over all
buffer rows at once, one complex multiply-add per position in the two sequential scans).  The engine itself is
gru_tracker.DeviceRecurrentTracker with the LRU structs and entry points, so the rollout, the learner and the plugin classes drive it as
they drive the GRU's."""
import math
from typing import Dict

import torch

from . import abi
from .gru_tracker import TOP_FIELDS, DeviceRecurrentTracker

DIM_MODEL = 32
MAX_LEN = 4096
MAX_LAYERS = abi.LRU_MAX_LAYERS
HIDDEN = abi.LRU_HIDDEN
# the struct members of the fifteen tensors between the shared ones and the decoder, and their state_dict names
LRU_FIELDS = [("nu_log", "lru.nu_log"), ("theta_log", "lru.theta_log"), ("gamma_log", "lru.gamma_log"),
              ("in_w", "lru.in_proj.weight"), ("in_b", "lru.in_proj.bias"), ("out_w", "lru.out_proj.weight"), ("out_b", "lru.out_proj.bias"),
              ("lln_w", "lru.ln.weight"), ("lln_b", "lru.ln.bias"), ("d1_w", "ffn.dense_1.weight"), ("d1_b", "ffn.dense_1.bias"),
              ("d2_w", "ffn.dense_2.weight"), ("d2_b", "ffn.dense_2.bias"), ("ln_w", "ffn.ln.weight"), ("ln_b", "ffn.ln.bias")]
assert tuple(f for f, _ in LRU_FIELDS) == abi.LRU_MEMBERS


def check_lru_shape(dim_model, dim_state, nlayers=1, d_hid=HIDDEN, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    if int(dim_model) != DIM_MODEL:
        raise ValueError(f"the LRU tracker is built for dim_model == {DIM_MODEL}, got {dim_model}")
    if not 1 <= int(dim_state) <= 32:
        raise ValueError(f"the LRU tracker is built for dim_state in 1..32, got {dim_state}")
    if int(nlayers) != MAX_LAYERS:
        raise ValueError(f"the LRU tracker is built for nlayers == {MAX_LAYERS} (one recurrence layer), got {nlayers}")
    if int(d_hid) != HIDDEN:
        raise ValueError(f"the LRU tracker is built for d_hid == {HIDDEN}, got {d_hid}")
    if max_len is not None and not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError(f"the LRU tracker is built for max_len (MAX_TURN + 1) in 1..{MAX_LEN}, got {max_len}")


def lru_param_shapes(n_users, n_items, dim_model=32, dim_state=20, nlayers=1):
    """Ordered {state_dict name: shape} of the 23 trainable tensors: the other trackers' names for what all share, then the recurrence under
    `lru.` (the three log vectors as plain parameters; nn.Linear(D, 2 D) under lru.in_proj, nn.Linear(2 D, D) under lru.out_proj,
    nn.LayerNorm(D) under lru.ln), the feed-forward block under `ffn.` (nn.Linear(D, 128), nn.Linear(128, D), nn.LayerNorm(D)), decoder last."""
    D, S = dim_model, dim_state
    return {"embedding_dict.feat_user.weight": (n_users, D), "embedding_dict.feat_item.weight": (n_items, D),
            "ffn_user.weight": (D, D), "ffn_user.bias": (D,), "fnn_gate.weight": (D, D + 1), "fnn_gate.bias": (D,),
            "lru.nu_log": (D,), "lru.theta_log": (D,), "lru.gamma_log": (D,),
            "lru.in_proj.weight": (2 * D, D), "lru.in_proj.bias": (2 * D,), "lru.out_proj.weight": (D, 2 * D), "lru.out_proj.bias": (D,),
            "lru.ln.weight": (D,), "lru.ln.bias": (D,),
            "ffn.dense_1.weight": (HIDDEN, D), "ffn.dense_1.bias": (HIDDEN,), "ffn.dense_2.weight": (D, HIDDEN), "ffn.dense_2.bias": (D,),
            "ffn.ln.weight": (D,), "ffn.ln.bias": (D,),
            "decoder.weight": (S, D), "decoder.bias": (S,)}


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
    torch_state = torch.random.get_rng_state()
    torch.manual_seed(int(seed) + 0x6C7275)      # a stream of its own: nothing shared moves with the recurrence
    try:
        u1 = torch.rand(D).clamp(1e-6, 1 - 1e-6)
        u2 = torch.rand(D).clamp(min=1e-6)
        mod2 = u1 * (r_max ** 2 - r_min ** 2) + r_min ** 2
        p["lru.nu_log"] = torch.log(-0.5 * torch.log(mod2))
        p["lru.theta_log"] = torch.log(max_phase * u2)
        p["lru.gamma_log"] = 0.5 * torch.log(1 - mod2)
        mods = {"lru.in_proj": torch.nn.Linear(D, 2 * D), "lru.out_proj": torch.nn.Linear(2 * D, D), "lru.ln": torch.nn.LayerNorm(D),
                "ffn.dense_1": torch.nn.Linear(D, HIDDEN), "ffn.dense_2": torch.nn.Linear(HIDDEN, D), "ffn.ln": torch.nn.LayerNorm(D)}
        for name, m in mods.items():
            for k, v in m.state_dict().items():
                p[f"{name}.{k}"] = v.detach().clone().float()
    finally:
        torch.random.set_rng_state(torch_state)
    return {k: p[k].float() for k in lru_param_shapes(n_users, n_items, dim_model, dim_state)}


class DeviceLruTracker(DeviceRecurrentTracker):
    """`params` maps state_dict names (lru_param_shapes) to device tensors.  Carries the complex state as h_re and h_im, [1, n_env, 32] each."""
    CFG, WEIGHTS, STATE, LAYER_FIELDS, ENTRY, check_shape = abi.LruCfg, abi.LruWeights, abi.LruState, (), "cirs_lru_tracker", check_lru_shape
    CARRY = ("h_re", "h_im")
    COLLECT, NAME = "cirs_rollout_collect_lru", "LRU"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, nlayers=1,
                 device="cuda"):
        self._max_len = max_turn + 1
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=nlayers, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_lru_shape(dim_model, dim_state, nlayers, HIDDEN, self._max_len)
        return {"nlayers": nlayers}

    def _weights(self, tensors):
        """cirs_lru_weights (or cirs_lru_grads: same layout), a flat struct: weights_struct knows the shared fields and per-layer cells only."""
        w = self.WEIGHTS()
        shapes = lru_param_shapes(self.cfg.n_users, self.cfg.n_items, DIM_MODEL, self.cfg.dim_state)
        for f, name in TOP_FIELDS + LRU_FIELDS:
            t = tensors[name]
            assert t.dtype == torch.float32 and t.is_contiguous(), name
            assert tuple(t.shape) == shapes[name], (name, tuple(t.shape))
            setattr(w, f, t.data_ptr())
        return w
