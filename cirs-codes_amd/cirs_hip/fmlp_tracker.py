"""Device engine of the filter-MLP state tracker (csrc/fmlp_tracker.hip): the input slots of the other trackers, FMLP-Rec's layers over the
tile of the last `window_size` item slots (a learned per-channel circular filter whose parameters live in the frequency domain, then a
LayerNorm / GELU feed-forward block of width 128), h_p = x_0 + the top layer's newest row, the same decoder.  One launch per step and nothing
carried besides the stored slots; the gradient arrives through cirs_fmlp_tracker_backward (no sequential pass).  The engine itself is
gru_tracker.DeviceRecurrentTracker with the FMLP structs and entry points, so the rollout, the learner and the plugin classes drive it as
they drive the GRU's."""
from typing import Dict

import torch

from . import abi
from .gru_tracker import TOP_FIELDS, DeviceRecurrentTracker

DIM_MODEL = 32
MAX_LEN = 4096
MAX_WINDOW = abi.FMLP_MAX_WINDOW      # one 16-row tile
MAX_LAYERS = abi.FMLP_MAX_LAYERS
HIDDEN = abi.FMLP_HIDDEN
# the struct members of a layer's nine tensors and their state_dict names
FMLP_LAYER_FIELDS = [("cw", "layers.{}.filter.complex_weight"), ("fln_w", "layers.{}.filter.ln.weight"), ("fln_b", "layers.{}.filter.ln.bias"),
                     ("d1_w", "layers.{}.ffn.dense_1.weight"), ("d1_b", "layers.{}.ffn.dense_1.bias"), ("d2_w", "layers.{}.ffn.dense_2.weight"),
                     ("d2_b", "layers.{}.ffn.dense_2.bias"), ("ln_w", "layers.{}.ffn.ln.weight"), ("ln_b", "layers.{}.ffn.ln.bias")]
assert tuple(f for f, _ in FMLP_LAYER_FIELDS) == abi.FMLP_LAYER_MEMBERS


def check_fmlp_shape(dim_model, dim_state, window_size, nlayers, d_hid=HIDDEN, max_len=None):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    if int(dim_model) != DIM_MODEL:
        raise ValueError(f"the FMLP tracker is built for dim_model == {DIM_MODEL}, got {dim_model}")
    if not 1 <= int(dim_state) <= 32:
        raise ValueError(f"the FMLP tracker is built for dim_state in 1..32, got {dim_state}")
    if not 1 <= int(window_size) <= MAX_WINDOW:
        raise ValueError(f"the FMLP tracker is built for window_size in 1..{MAX_WINDOW}, got {window_size}")
    if int(nlayers) not in (1, 2):
        raise ValueError(f"the FMLP tracker is built for nlayers in {{1, 2}}, got {nlayers}")
    if int(d_hid) != HIDDEN:
        raise ValueError(f"the FMLP tracker is built for d_hid == {HIDDEN}, got {d_hid}")
    if max_len is not None and not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError(f"the FMLP tracker is built for max_len (MAX_TURN + 1) in 1..{MAX_LEN}, got {max_len}")


def fmlp_param_shapes(n_users, n_items, dim_model=32, dim_state=20, window_size=10, nlayers=2):
    """Ordered {state_dict name: shape} of the 8 + 9 L trainable tensors: the other trackers' names for what all share, then per layer the
    filter (complex_weight [W//2+1, D, 2]: real and imaginary part, what torch.view_as_complex reads; nn.LayerNorm(D) under filter.ln) and the
    feed-forward block (nn.Linear(D, 128) under ffn.dense_1, nn.Linear(128, D) under ffn.dense_2, nn.LayerNorm(D) under ffn.ln), decoder last
    -- in the order a torch module with these children lists them in its state_dict.  The shape of complex_weight depends on the window."""
    D, S, W = dim_model, dim_state, int(window_size)
    sh = {"embedding_dict.feat_user.weight": (n_users, D), "embedding_dict.feat_item.weight": (n_items, D),
          "ffn_user.weight": (D, D), "ffn_user.bias": (D,), "fnn_gate.weight": (D, D + 1), "fnn_gate.bias": (D,)}
    for l in range(int(nlayers)):
        sh.update({f"layers.{l}.filter.complex_weight": (W // 2 + 1, D, 2), f"layers.{l}.filter.ln.weight": (D,), f"layers.{l}.filter.ln.bias": (D,),
                   f"layers.{l}.ffn.dense_1.weight": (HIDDEN, D), f"layers.{l}.ffn.dense_1.bias": (HIDDEN,),
                   f"layers.{l}.ffn.dense_2.weight": (D, HIDDEN), f"layers.{l}.ffn.dense_2.bias": (D,),
                   f"layers.{l}.ffn.ln.weight": (D,), f"layers.{l}.ffn.ln.bias": (D,)})
    sh.update({"decoder.weight": (S, D), "decoder.bias": (S,)})
    return sh


def init_fmlp_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, window_size=10, nlayers=2,
                             init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what all trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors); from a generator
    stream of their own complex_weight ~ 0.02 N(0, 1) (FMLP-Rec's) and the Linear / LayerNorm tensors by torch's defaults.  torch modules are
    parameter factories only; the caller's RNG state is restored."""
    from .engine import init_tracker_params
    shared = init_tracker_params(n_users, n_items, 1, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    shapes = fmlp_param_shapes(n_users, n_items, dim_model, dim_state, window_size, nlayers)
    p = {k: shared[k] for k in shapes if k in shared}
    D, W = dim_model, int(window_size)
    torch_state = torch.random.get_rng_state()
    torch.manual_seed(int(seed) + 0x666D6C70)      # a stream of its own: the shared tensors do not move with the layers
    try:
        for l in range(int(nlayers)):
            p[f"layers.{l}.filter.complex_weight"] = 0.02 * torch.randn(W // 2 + 1, D, 2)
            mods = {"filter.ln": torch.nn.LayerNorm(D), "ffn.dense_1": torch.nn.Linear(D, HIDDEN), "ffn.dense_2": torch.nn.Linear(HIDDEN, D),
                    "ffn.ln": torch.nn.LayerNorm(D)}
            for name, m in mods.items():
                for k, v in m.state_dict().items():
                    p[f"layers.{l}.{name}.{k}"] = v.detach().clone().float()
    finally:
        torch.random.set_rng_state(torch_state)
    return {k: p[k] for k in shapes}


class DeviceFmlpTracker(DeviceRecurrentTracker):
    """`params` maps state_dict names (fmlp_param_shapes) to device tensors.  Carries nothing: the tile is read from x_hist."""
    CFG, WEIGHTS, STATE, LAYER_FIELDS, ENTRY = abi.FmlpCfg, abi.FmlpWeights, abi.FmlpState, (), "cirs_fmlp_tracker"
    CARRY = ()
    COLLECT, NAME = "cirs_rollout_collect_fmlp", "FMLP"

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, window_size=10,
                 nlayers=2, device="cuda"):
        self.window_size = int(window_size)
        self._max_len = max_turn + 1
        super().__init__(params, n_users, n_items, n_env, max_turn, dim_model=dim_model, dim_state=dim_state, nlayers=nlayers, device=device)

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        check_fmlp_shape(dim_model, dim_state, self.window_size, nlayers, HIDDEN, self._max_len)
        return {"window": self.window_size, "nlayers": int(nlayers)}

    def _weights(self, tensors):
        """cirs_fmlp_weights (or cirs_fmlp_grads: same layout): the shared fields, then every layer member as an array over the layers."""
        w = self.WEIGHTS()
        for f, name in TOP_FIELDS:
            t = tensors[name]
            assert t.dtype == torch.float32 and t.is_contiguous(), name
            setattr(w, f, t.data_ptr())
        W = self.window_size
        for l in range(int(self.nlayers)):
            for f, name in FMLP_LAYER_FIELDS:
                t = tensors[name.format(l)]
                assert t.dtype == torch.float32 and t.is_contiguous(), name
                if f == "cw":
                    assert tuple(t.shape) == (W // 2 + 1, DIM_MODEL, 2), (name, tuple(t.shape))      # the kernel indexes it by the cfg's window
                getattr(w, f)[l] = t.data_ptr()
        return w
