"""Device engine of the GRU-with-attention state tracker (csrc/narm_tracker.hip): the input slots of the other trackers, one torch.nn.GRU layer
carried as 32 floats per env, NARM's additive attention over every hidden state of the session so far (a sigmoid network without softmax), the
bilinear read-out m_p = Bw [h_p ; c_p], the same decoder.  One launch per step; besides h an env keeps its hidden states and their A2
projections (h_hist, q_hist: [n_env, max_len, 32] each), so a step costs O(position).  The gradient arrives through cirs_narm_tracker_backward
(the attention's backward in parallel over the rows, fed into the GRU's sequential back-propagation through time).  The engine itself is
slot_engine.DeviceSlotTracker with the NARM structs and entry points, so the rollout, the learner and the plugin classes drive it as they
drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .slot_engine import DeviceSlotTracker, add_module_params, check_dims, check_max_len, decoder_shapes, head_shapes, own_stream

MAX_LAYERS = abi.NARM_MAX_LAYERS


def check_narm_shape(dim_model, dim_state, nlayers=1, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("NARM", dim_model, dim_state)
    if int(nlayers) != MAX_LAYERS:
        raise ValueError(f"the NARM tracker is built for nlayers == {MAX_LAYERS} (one encoder layer), got {nlayers}")
    check_max_len("NARM", max_len)


def narm_param_shapes(n_users, n_items, dim_model=32, dim_state=20, nlayers=1):
    """Ordered {state_dict name: shape} of the 16 trainable tensors: the other trackers' names for what all share, torch.nn.GRU's (under `gru.`)
    for the encoder, so that they load into nn.GRU(dim_model, dim_model, 1) by name, then the attention (nn.Linear(D, D, bias=False) under
    attn.a1 / attn.a2, nn.Linear(D, 1, bias=False) under attn.v) and the read-out (nn.Linear(2 D, D, bias=False) under bilinear), decoder
    last."""
    D = dim_model
    return {**head_shapes(n_users, n_items, D),
            "gru.weight_ih_l0": (3 * D, D), "gru.weight_hh_l0": (3 * D, D), "gru.bias_ih_l0": (3 * D,), "gru.bias_hh_l0": (3 * D,),
            "attn.a1.weight": (D, D), "attn.a2.weight": (D, D), "attn.v.weight": (1, D), "bilinear.weight": (D, 2 * D),
            **decoder_shapes(D, dim_state)}


def init_narm_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, nlayers=1, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: the shared and the gru.* tensors exactly as gru_tracker.init_gru_tracker_params draws them (same seed -> same
    tensors), the attention and the read-out with torch's default nn.Linear init from a generator stream of their own.  torch modules are
    parameter factories only."""
    from .gru_tracker import init_gru_tracker_params
    p = init_gru_tracker_params(n_users, n_items, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    D = dim_model
    with own_stream(int(seed) + 0x6E61726D):      # nothing shared moves with the attention
        add_module_params(p, {"attn.a1": torch.nn.Linear(D, D, bias=False), "attn.a2": torch.nn.Linear(D, D, bias=False),
                              "attn.v": torch.nn.Linear(D, 1, bias=False), "bilinear": torch.nn.Linear(2 * D, D, bias=False)})
    return {k: p[k] for k in narm_param_shapes(n_users, n_items, dim_model, dim_state)}


class DeviceNarmTracker(DeviceSlotTracker):
    """`params` maps state_dict names (narm_param_shapes) to device tensors.  Carries h; keeps h_hist and q_hist next to x_hist."""
    CFG, WEIGHTS, STATE, ENTRY, check_shape, param_shapes = abi.NarmCfg, abi.NarmWeights, abi.NarmState, "cirs_narm_tracker", check_narm_shape, narm_param_shapes
    FIELDS = [("w_ih", "gru.weight_ih_l0"), ("w_hh", "gru.weight_hh_l0"), ("b_ih", "gru.bias_ih_l0"), ("b_hh", "gru.bias_hh_l0"),
              ("a1", "attn.a1.weight"), ("a2", "attn.a2.weight"), ("v", "attn.v.weight"), ("bw", "bilinear.weight")]
    CARRY = ("h",)
    COLLECT, NAME = "cirs_rollout_collect_narm", "NARM"

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_narm_shape(dim_model, dim_state, nlayers, self.max_len)
        return {"nlayers": nlayers}

    def _state(self, x_hist):
        """The engine's own histories go with every x_hist: the backward over a buffer with another env count reads x_hist only."""
        if not hasattr(self, "h_hist"):
            self.h_hist, self.q_hist = torch.zeros_like(self.x_hist), torch.zeros_like(self.x_hist)
        return self.STATE(x_hist=x_hist.data_ptr(), h=self.h.data_ptr(), h_hist=self.h_hist.data_ptr(), q_hist=self.q_hist.data_ptr(),
                          len=self.len.data_ptr())
