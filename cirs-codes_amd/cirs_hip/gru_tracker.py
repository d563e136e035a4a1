"""Device engine of the recurrent state tracker (csrc/gru_tracker.hip): the input slots of the Transformer tracker, a
torch.nn.GRU(D, D, L) recurrence carried as L x 32 floats per env, the same decoder.  One launch per step; the gradient arrives
through cirs_gru_tracker_backward (back-propagation through time, recomputed from the stored slots).  Same engine surface as
cirs_hip.tracker.DeviceTracker, so the rollout, the learner and the plugin classes drive either."""
import ctypes as C
from typing import Dict

import torch

from . import abi
from .tracker import flat_tracker_params

TOP_FIELDS = [("emb_user", "embedding_dict.feat_user.weight"), ("emb_item", "embedding_dict.feat_item.weight"),
              ("ffn_user_w", "ffn_user.weight"), ("ffn_user_b", "ffn_user.bias"), ("gate_w", "fnn_gate.weight"),
              ("gate_b", "fnn_gate.bias"), ("dec_w", "decoder.weight"), ("dec_b", "decoder.bias")]
LAYER_FIELDS = [("w_ih", "gru.weight_ih_l{}"), ("w_hh", "gru.weight_hh_l{}"), ("b_ih", "gru.bias_ih_l{}"), ("b_hh", "gru.bias_hh_l{}")]
DIM_MODEL = 32
MAX_LAYERS = abi.GRU_MAX_LAYERS


def check_gru_shape(dim_model, dim_state, nlayers):
    """The fixed sizes of this build (include/cirs_hip.h); raises before any device use."""
    if int(dim_model) != DIM_MODEL:
        raise ValueError(f"the GRU tracker is built for dim_model == {DIM_MODEL}, got {dim_model}")
    if not 1 <= int(dim_state) <= 32:
        raise ValueError(f"the GRU tracker is built for dim_state in 1..32, got {dim_state}")
    if int(nlayers) not in (1, 2):
        raise ValueError(f"the GRU tracker is built for nlayers in {{1, 2}}, got {nlayers}")


def gru_param_shapes(n_users, n_items, dim_model=32, dim_state=20, nlayers=1):
    """Ordered {state_dict name: shape} of the trainable tensors: the Transformer tracker's names for what both share, torch.nn.GRU's
    (under `gru.`) for the recurrence, so that the gru.* entries load into nn.GRU(dim_model, dim_model, nlayers) by name."""
    D, S = dim_model, dim_state
    sh = {"embedding_dict.feat_user.weight": (n_users, D), "embedding_dict.feat_item.weight": (n_items, D),
          "ffn_user.weight": (D, D), "ffn_user.bias": (D,), "fnn_gate.weight": (D, D + 1), "fnn_gate.bias": (D,)}
    for l in range(nlayers):
        sh.update({f"gru.weight_ih_l{l}": (3 * D, D), f"gru.weight_hh_l{l}": (3 * D, D), f"gru.bias_ih_l{l}": (3 * D,),
                   f"gru.bias_hh_l{l}": (3 * D,)})
    sh.update({"decoder.weight": (S, D), "decoder.bias": (S,)})
    return sh


def init_gru_tracker_params(n_users, n_items, seed=2021, dim_model=32, dim_state=20, nlayers=1, init_std=1e-4) -> Dict[str, torch.Tensor]:
    """Fresh parameters: what both trackers share exactly as engine.init_tracker_params draws it (same seed -> same tensors), the GRU
    tensors with torch's default U(-1/sqrt(D), 1/sqrt(D)) from a generator seeded by `seed`.  torch modules are parameter factories only."""
    from .engine import init_tracker_params
    shared = init_tracker_params(n_users, n_items, 1, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    p = {k: v for k, v in shared.items() if not k.startswith("transformer_encoder.") and k != "pos_encoder.pe"}
    torch_state = torch.random.get_rng_state()
    torch.manual_seed(int(seed) + 0x6772)      # a stream of its own: the shared tensors do not move when nlayers changes
    try:
        gru = torch.nn.GRU(dim_model, dim_model, nlayers)
        for k, v in gru.state_dict().items():
            p["gru." + k] = v.detach().clone().float()
    finally:
        torch.random.set_rng_state(torch_state)
    return {k: p[k] for k in gru_param_shapes(n_users, n_items, dim_model, dim_state, nlayers)}


def weights_struct(params: Dict[str, torch.Tensor], nlayers: int, struct=abi.GruWeights, layer_fields=None):
    """cirs_gru_weights (or cirs_gru_grads: same layout; `struct` / `layer_fields`: another cell's) from tensors keyed by state_dict names
    (fp32, contiguous, device)."""
    w = struct()
    for f, name in TOP_FIELDS:
        t = params[name]
        assert t.dtype == torch.float32 and t.is_contiguous(), name
        setattr(w, f, t.data_ptr())
    for l in range(nlayers):
        for f, name in layer_fields or LAYER_FIELDS:
            t = params[name.format(l)]
            assert t.dtype == torch.float32 and t.is_contiguous(), name
            setattr(w.layer[l], f, t.data_ptr())
    return w


class DeviceRecurrentTracker:
    """Recurrent tracker state for B envs: what the GRU and the LSTM engine share.  A subclass names its cell: the ctypes structs, the
    layers' state_dict names, the prefix of its entry points, its shape check, and the carried tensors next to h (CARRY).  The pooled-window
    engine (avg_tracker.DeviceAvgTracker) is the same surface with no layers and nothing carried."""
    CFG = WEIGHTS = STATE = LAYER_FIELDS = ENTRY = check_shape = None
    CARRY = ("h",)

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, nlayers=1,
                 device="cuda"):
        cell = self._cell_cfg(dim_model, dim_state, nlayers)
        self.device = torch.device(device)
        self.cfg = self.CFG(n_users=n_users, n_items=n_items, dim_model=dim_model, dim_state=dim_state, max_len=max_turn + 1, n_env=n_env, **cell)
        self.params = params
        self.nlayers = nlayers
        self.w = self._weights(params)
        L, B, D = max_turn + 1, n_env, dim_model
        self.x_hist = torch.zeros((B, L, D), dtype=torch.float32, device=self.device)
        for k in self.CARRY:
            setattr(self, k, torch.zeros((nlayers, B, D), dtype=torch.float32, device=self.device))
        self.len = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.st = self._state(self.x_hist)
        self._bws = None
        self._lib = abi.lib()
        self.dim_state = dim_state

    def _cell_cfg(self, dim_model, dim_state, nlayers):
        """The shape check of this build, then the members of the cfg struct that describe the cell."""
        type(self).check_shape(dim_model, dim_state, nlayers)
        return {"nlayers": nlayers}

    def _weights(self, tensors):
        return weights_struct(tensors, self.nlayers, self.WEIGHTS, self.LAYER_FIELDS)

    def _state(self, x_hist):
        return self.STATE(x_hist=x_hist.data_ptr(), len=self.len.data_ptr(), **{k: getattr(self, k).data_ptr() for k in self.CARRY})

    def _entry(self, suffix):
        return getattr(self._lib, self.ENTRY + suffix), self.ENTRY + suffix

    # nn.GRU / nn.LSTM have dropout between layers only, and that one is not built: nothing to set
    def set_dropout(self, p: float):
        pass

    def set_dropout_key(self, seed: int, tag: int = 0, env_base: int = 0):
        pass

    def refresh_weights(self):
        self.w = self._weights(self.params)

    # ---- training side ------------------------------------------------------------------------------------------
    def enable_training(self, flat_params: torch.Tensor, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        """`flat_params` must be the flat buffer self.params' tensors are views of (tracker.flat_tracker_params)."""
        shapes = {k: tuple(v.shape) for k, v in self.params.items()}
        self.flat = flat_params
        self.flat_grad, self.grad_views = flat_tracker_params(shapes, device=self.device)
        assert self.flat_grad.numel() == flat_params.numel()
        self.g = self._weights(self.grad_views)
        self.adam_m = torch.zeros_like(flat_params)
        self.adam_v = torch.zeros_like(flat_params)
        self.adam_steps = 0
        self.lr, self.betas, self.adam_eps = lr, betas, eps
        self._bws = None

    def _workspace(self, cfg, n_rows):
        need = self._entry("_backward_workspace_bytes")[0](C.byref(cfg), n_rows)
        if self._bws is None or self._bws.numel() < need:
            self._bws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._bws

    def backward(self, users, traj, row_env, row_t, offsets, lens, n_rows, dstate, x_hist=None):
        """d loss / d tracker params from d loss / d obs (dstate [T+1,B,S]); fills self.flat_grad.
        x_hist: stored input slots [B', max_len, D] when the rows come from a buffer whose env count B' = traj.B differs from this
        tracker's own n_env."""
        users = users.to(self.device, torch.int32).contiguous()
        cfg, st = self.cfg, self.st
        if x_hist is not None:
            cfg = self.CFG.from_buffer_copy(self.cfg)
            cfg.n_env = x_hist.shape[0]
            st = self._state(x_hist)
        ws = self._workspace(cfg, n_rows)
        fn, name = self._entry("_backward")
        abi.check(fn(
            C.byref(cfg), C.byref(self.w), C.byref(st), users.data_ptr(), traj.act.data_ptr(), traj.rew.data_ptr(), row_env.data_ptr(),
            row_t.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n_rows, dstate.data_ptr(), C.byref(self.g), ws.data_ptr(), ws.numel(),
            self._stream()), name)

    def reserve_backward(self, max_rows):
        self._workspace(self.cfg, max_rows)

    def adam_update(self):
        """One torch.optim.Adam step over every tracker tensor (the same cirs_adam_step the Transformer tracker takes)."""
        abi.check(self._lib.cirs_adam_step(self.flat.data_ptr(), self.flat_grad.data_ptr(), self.adam_m.data_ptr(),
                                           self.adam_v.data_ptr(), self.flat.numel(), self.adam_steps, 1, self.lr,
                                           self.betas[0], self.betas[1], self.adam_eps, None, 0, self._stream()),
                  "cirs_adam_step")
        self.adam_steps += 1

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def reset(self):
        self.len.zero_()

    def init(self, users, env_ids=None, out=None, out_stride=None):
        users = users.to(self.device, torch.int32).contiguous()
        n = users.numel()
        ids = None if env_ids is None else env_ids.to(self.device, torch.int32).contiguous()
        if out is None:
            out = torch.empty((n, self.dim_state), dtype=torch.float32, device=self.device)
            out_stride = self.dim_state
        fn, name = self._entry("_init")
        abi.check(fn(C.byref(self.cfg), C.byref(self.w), C.byref(self.st), users.data_ptr(), abi.ptr(ids), n, out.data_ptr(), out_stride,
                     self._stream()), name)
        return out

    def step(self, items, rew, env_ids=None, skip=None, out=None, out_stride=None):
        items = items.to(self.device, torch.int64).contiguous()
        rew = rew.to(self.device, torch.float64).contiguous()
        n = items.numel()
        ids = None if env_ids is None else env_ids.to(self.device, torch.int32).contiguous()
        if out is None:
            out = torch.empty((n, self.dim_state), dtype=torch.float32, device=self.device)
            out_stride = self.dim_state
        fn, name = self._entry("_step")
        abi.check(fn(C.byref(self.cfg), C.byref(self.w), C.byref(self.st), items.data_ptr(), rew.data_ptr(), abi.ptr(ids), abi.ptr(skip), n,
                     out.data_ptr(), out_stride, self._stream()), name)
        return out


class DeviceGruTracker(DeviceRecurrentTracker):
    """`params` maps state_dict names (gru_param_shapes) to device tensors."""
    CFG, WEIGHTS, STATE, LAYER_FIELDS, ENTRY, check_shape = abi.GruCfg, abi.GruWeights, abi.GruState, LAYER_FIELDS, "cirs_gru_tracker", check_gru_shape
    COLLECT, NAME = "cirs_rollout_collect_gru", "GRU"
