"""Device engine of the convolutional window state tracker (csrc/caser_tracker.hip): the input slots of the other trackers, the window of the
last `window_size` item slots through Caser's horizontal filter banks (max-pooled over time) and its vertical filter, one fc layer, h_p = x_0 +
z, the same decoder.  One launch per step and nothing carried besides the stored slots; the gradient arrives through
cirs_caser_tracker_backward (no sequential pass).  The engine itself is slot_engine.DeviceSlotTracker with the Caser structs and entry
points, so the rollout, the learner and the plugin classes drive it as they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .slot_engine import (DeviceSlotTracker, add_module_params, check_dims, check_max_len, decoder_shapes, head_shapes, own_stream,
                          shared_init_params)

NUM_FILTERS = 16
MAX_WINDOW = 16
MAX_HEIGHT = 4


def check_caser_shape(dim_model, dim_state, window_size, filter_sizes, num_filters=NUM_FILTERS, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    check_dims("Caser", dim_model, dim_state)
    if int(num_filters) != NUM_FILTERS:
        raise ValueError(f"the Caser tracker is built for num_filters == {NUM_FILTERS}, got {num_filters}")
    hs = [int(h) for h in filter_sizes]
    if not hs or any(not 1 <= h <= MAX_HEIGHT for h in hs) or any(b <= a for a, b in zip(hs, hs[1:])):
        raise ValueError(f"the Caser tracker is built for filter_sizes a non-empty, strictly ascending subset of 1..{MAX_HEIGHT}, got {tuple(filter_sizes)}")
    if not hs[-1] <= int(window_size) <= MAX_WINDOW:
        raise ValueError(f"the Caser tracker is built for window_size in max(filter_sizes)..{MAX_WINDOW}, got window_size {window_size} with "
                         f"filter_sizes {tuple(hs)}")
    check_max_len("Caser", max_len)


def caser_param_shapes(n_users, n_items, dim_model=32, dim_state=20, window_size=10, filter_sizes=(2, 3, 4), num_filters=NUM_FILTERS):
    """Ordered {state_dict name: shape} of the trainable tensors: the other trackers' names for what all share, then the filter banks, the
    vertical filter and fc under names that load into nn.Conv2d(1, F, (h, D)) / nn.Conv2d(1, 1, (W, 1)) / nn.Linear by name, decoder last."""
    D, F = dim_model, num_filters
    sh = head_shapes(n_users, n_items, D)
    for i, h in enumerate(filter_sizes):
        sh.update({f"horizontal_cnn.{i}.weight": (F, 1, int(h), D), f"horizontal_cnn.{i}.bias": (F,)})
    sh.update({"vertical_cnn.weight": (1, 1, int(window_size), 1), "vertical_cnn.bias": (1,),
               "fc.weight": (D, F * len(filter_sizes) + D), "fc.bias": (D,), **decoder_shapes(D, dim_state)})
    return sh


def init_caser_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, window_size=10, filter_sizes=(2, 3, 4),
                              num_filters=NUM_FILTERS, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what all trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the filters and fc
    with torch's default init from a generator stream of their own.  torch modules are parameter factories only."""
    p = shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std)
    with own_stream(int(seed) + 0x63617372):      # the shared tensors do not move with the window or the banks
        mods = {f"horizontal_cnn.{i}": torch.nn.Conv2d(1, num_filters, (int(h), dim_model)) for i, h in enumerate(filter_sizes)}
        mods["vertical_cnn"] = torch.nn.Conv2d(1, 1, (int(window_size), 1))
        mods["fc"] = torch.nn.Linear(num_filters * len(filter_sizes) + dim_model, dim_model)
        add_module_params(p, mods)
    return {k: p[k] for k in caser_param_shapes(n_users, n_items, dim_model, dim_state, window_size, filter_sizes, num_filters)}


class DeviceCaserTracker(DeviceSlotTracker):
    """`params` maps state_dict names (caser_param_shapes) to device tensors.  Carries nothing: the window is read from x_hist."""
    CFG, WEIGHTS, STATE, ENTRY, param_shapes = abi.CaserCfg, abi.CaserWeights, abi.CaserState, "cirs_caser_tracker", caser_param_shapes
    FIELDS = [("conv_w[]", "horizontal_cnn.{}.weight"), ("conv_b[]", "horizontal_cnn.{}.bias"), ("vert_w", "vertical_cnn.weight"),
              ("vert_b", "vertical_cnn.bias"), ("fc_w", "fc.weight"), ("fc_b", "fc.bias")]
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_caser", "Caser"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, window_size=10,
                 filter_sizes=(2, 3, 4), num_filters=NUM_FILTERS, device="cuda"):
        self.window_size, self.filter_sizes, self.num_filters = int(window_size), tuple(int(h) for h in filter_sizes), int(num_filters)
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=0, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_caser_shape(dim_model, dim_state, self.window_size, self.filter_sizes, self.num_filters, self.max_len)
        hs = self.filter_sizes + (0,) * (abi.CASER_MAX_HEIGHTS - len(self.filter_sizes))
        return {"window": self.window_size, "n_heights": len(self.filter_sizes), "heights": (abi.C.c_int32 * abi.CASER_MAX_HEIGHTS)(*hs)}

    def _shape_kw(self):
        return {"window_size": self.window_size, "filter_sizes": self.filter_sizes, "num_filters": self.num_filters}

    def _live(self):
        return len(self.filter_sizes)
