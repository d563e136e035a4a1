"""Device engine of the dilated-convolution state tracker (csrc/nextitnet_tracker.hip): the input slots of the other trackers, NextItNet's
residual blocks of dilated causal convolutions (width 3, LayerNorm, ReLU) over the item slots, h_p = x_0 + the top block's last position, the
same decoder.  One launch per step and nothing carried besides the stored slots; the gradient arrives through
cirs_nextitnet_tracker_backward (no sequential pass).  The engine itself is slot_engine.DeviceSlotTracker with the NextItNet structs and
entry points, so the rollout, the learner and the plugin classes drive it as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .slot_engine import (DeviceSlotTracker, add_module_params, check_dims, check_max_len, decoder_shapes, head_shapes, own_stream,
                          shared_init_params)

KERNEL_SIZE = 3
MAX_BLOCKS = abi.NEXTITNET_MAX_BLOCKS
MAX_DILATION = 4
MAX_DILATION_SUM = 7      # receptive field 1 + 2 * 7 = 15 item slots: one 16-row tile


def check_nextitnet_shape(dim_model, dim_state, dilations, kernel_size=KERNEL_SIZE, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("NextItNet", dim_model, dim_state)
    if int(kernel_size) != KERNEL_SIZE:
        raise ValueError(f"the NextItNet tracker is built for kernel_size == {KERNEL_SIZE}, got {kernel_size}")
    ds = [int(d) for d in dilations]
    if not 1 <= len(ds) <= MAX_BLOCKS:
        raise ValueError(f"the NextItNet tracker is built for n_blocks (len(dilations)) in 1..{MAX_BLOCKS}, got dilations {tuple(dilations)}")
    if any(not 1 <= d <= MAX_DILATION for d in ds):
        raise ValueError(f"the NextItNet tracker is built for dilations each in 1..{MAX_DILATION}, got {tuple(dilations)}")
    if sum(ds) > MAX_DILATION_SUM:
        raise ValueError(f"the NextItNet tracker is built for dilations that sum to at most {MAX_DILATION_SUM} (a receptive field of at most "
                         f"15 item slots), got {tuple(ds)} with sum {sum(ds)}")
    check_max_len("NextItNet", max_len)


def nextitnet_param_shapes(n_users, n_items, dim_model=32, dim_state=20, dilations=(1, 2, 4)):
    """Ordered {state_dict name: shape} of the trainable tensors: the other trackers' names for what all share, then per block the tensors of
    nn.Conv1d(D, D, 3, dilation=d_l) under blocks.<l>.conv and of nn.LayerNorm(D) under blocks.<l>.ln, decoder last."""
    D = dim_model
    sh = head_shapes(n_users, n_items, D)
    for l in range(len(dilations)):
        sh.update({f"blocks.{l}.conv.weight": (D, D, KERNEL_SIZE), f"blocks.{l}.conv.bias": (D,), f"blocks.{l}.ln.weight": (D,),
                   f"blocks.{l}.ln.bias": (D,)})
    sh.update(decoder_shapes(D, dim_state))
    return sh


def init_nextitnet_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, dilations=(1, 2, 4),
                                  init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what all trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the blocks with
    torch's default init from a generator stream of their own.  torch modules are parameter factories only."""
    p = shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std)
    with own_stream(int(seed) + 0x6E696E):      # the shared tensors do not move with the blocks
        for l, d in enumerate(dilations):
            mods = {"conv": torch.nn.Conv1d(dim_model, dim_model, KERNEL_SIZE, dilation=int(d)), "ln": torch.nn.LayerNorm(dim_model)}
            add_module_params(p, mods, f"blocks.{l}.")
    return {k: p[k] for k in nextitnet_param_shapes(n_users, n_items, dim_model, dim_state, dilations)}


class DeviceNextItNetTracker(DeviceSlotTracker):
    """`params` maps state_dict names (nextitnet_param_shapes) to device tensors.  Carries nothing: the receptive field is read from x_hist."""
    CFG, WEIGHTS, STATE, ENTRY, param_shapes = abi.NextItNetCfg, abi.NextItNetWeights, abi.NextItNetState, "cirs_nextitnet_tracker", nextitnet_param_shapes
    FIELDS = [("conv_w[]", "blocks.{}.conv.weight"), ("conv_b[]", "blocks.{}.conv.bias"), ("ln_w[]", "blocks.{}.ln.weight"),
              ("ln_b[]", "blocks.{}.ln.bias")]
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_nextitnet", "NextItNet"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, dilations=(1, 2, 4),
                 kernel_size=KERNEL_SIZE, device="cuda"):
        self.dilations, self.kernel_size = tuple(int(d) for d in dilations), int(kernel_size)
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=0, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_nextitnet_shape(dim_model, dim_state, self.dilations, self.kernel_size, self.max_len)
        ds = self.dilations + (0,) * (abi.NEXTITNET_MAX_BLOCKS - len(self.dilations))
        return {"n_blocks": len(self.dilations), "dilations": (abi.C.c_int32 * abi.NEXTITNET_MAX_BLOCKS)(*ds)}

    def _shape_kw(self):
        return {"dilations": self.dilations}

    def _live(self):
        return len(self.dilations)
