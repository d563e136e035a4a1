"""What the nine slot trackers' device engines share (GRU, LSTM, Avg, Caser, NextItNet, STAMP, NARM, FMLP, LRU): the engine class, the
table-driven filler of their weight structs with its dtype / contiguity / shape refusals, the checks of the sizes every build fixes, the
shapes of the tensors all of them have, and the scaffolding of their parameter initialisers.  A tracker's own module (x_tracker.py) keeps
what is its own: check_x_shape, x_param_shapes, init_x_tracker_params and the engine subclass with its field table."""
import contextlib
import ctypes as C
from typing import Dict

import torch

from . import abi

# struct member and state_dict name of the tensors every tracker has: six in front of a tracker's own members, the decoder behind them
HEAD_FIELDS = [("emb_user", "embedding_dict.feat_user.weight"), ("emb_item", "embedding_dict.feat_item.weight"),
               ("ffn_user_w", "ffn_user.weight"), ("ffn_user_b", "ffn_user.bias"), ("gate_w", "fnn_gate.weight"), ("gate_b", "fnn_gate.bias")]
DECODER_FIELDS = [("dec_w", "decoder.weight"), ("dec_b", "decoder.bias")]
TOP_FIELDS = HEAD_FIELDS + DECODER_FIELDS
DIM_MODEL = 32
MAX_LEN = 4096


def check_dims(display, dim_model, dim_state):
    """The two sizes every slot tracker's build fixes (include/cirs_hip.h); `display` is the tracker's name in the message."""
    if int(dim_model) != DIM_MODEL:
        raise ValueError(f"the {display} tracker is built for dim_model == {DIM_MODEL}, got {dim_model}")
    if not 1 <= int(dim_state) <= 32:
        raise ValueError(f"the {display} tracker is built for dim_state in 1..32, got {dim_state}")


def check_max_len(display, max_len):
    if max_len is not None and not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError(f"the {display} tracker is built for max_len (MAX_TURN + 1) in 1..{MAX_LEN}, got {max_len}")


def head_shapes(n_users, n_items, dim_model):
    """{state_dict name: shape} of the six tensors in front of a tracker's own."""
    D = dim_model
    return {"embedding_dict.feat_user.weight": (n_users, D), "embedding_dict.feat_item.weight": (n_items, D),
            "ffn_user.weight": (D, D), "ffn_user.bias": (D,), "fnn_gate.weight": (D, D + 1), "fnn_gate.bias": (D,)}


def decoder_shapes(dim_model, dim_state):
    return {"decoder.weight": (dim_state, dim_model), "decoder.bias": (dim_state,)}


def shared_init_params(n_users, n_items, seed, dim_model, dim_state, init_std) -> Dict[str, torch.Tensor]:
    """The eight tensors of TOP_FIELDS exactly as engine.init_tracker_params draws them (same seed -> same tensors)."""
    from .engine import init_tracker_params
    shared = init_tracker_params(n_users, n_items, 1, seed=seed, dim_model=dim_model, dim_state=dim_state, nlayers=1, init_std=init_std)
    return {name: shared[name] for _, name in TOP_FIELDS}


@contextlib.contextmanager
def own_stream(seed):
    """torch's global generator seeded with `seed` inside the block (a tracker's own tensors come from a stream of their own: nothing shared
    moves with its model arguments); the caller's RNG state is restored on the way out."""
    state = torch.random.get_rng_state()
    torch.manual_seed(int(seed))
    try:
        yield
    finally:
        torch.random.set_rng_state(state)


def add_module_params(p, mods, prefix=""):
    """The state_dict tensors of the torch modules `mods` ({name: module}: parameter factories only) into `p` under prefix + name + "."."""
    for name, m in mods.items():
        for k, v in m.state_dict().items():
            p[f"{prefix}{name}.{k}"] = v.detach().clone().float()


def struct_members(struct):
    """The pointer members of a ctypes weight struct in order, spelled as a field table spells them: "m" for a pointer, "m[]" for an array
    of pointers, "m[].f" for every member f of an array of structs."""
    out = []
    for k, ct in struct._fields_:
        if not issubclass(ct, C.Array):
            out.append(k)
        elif issubclass(ct._type_, C.Structure):
            out += [f"{k}[].{f}" for f, _ in ct._type_._fields_]
        else:
            out.append(k + "[]")
    return out


def fill_weights(struct, fields, n_live, expected, tensors):
    """`struct` (a cirs_x_weights, or the cirs_x_grads of the same layout) from tensors keyed by state_dict names.  `fields` is the
    tracker's table of (member, state_dict name) between HEAD_FIELDS and DECODER_FIELDS; an indexed member ("conv_w[]", "layer[].w_ih") has a
    "{}" in its name and is filled at indices 0 .. n_live-1, the rest stay null.  Every tensor must be fp32, contiguous and of the shape
    `expected` gives for its name -- the kernels index these pointers by the cfg's sizes alone -- else ValueError; a missing name is a
    KeyError.  Reads data_ptr() only: works on CPU tensors and without the library."""
    w = struct()
    for member, name in HEAD_FIELDS + list(fields) + DECODER_FIELDS:
        array, indexed, sub = member.partition("[]")
        for i in range(int(n_live)) if indexed else (None,):
            key = name.format(i)
            t = tensors[key]
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{key} must be a contiguous float32 tensor, got {t.dtype}, contiguous: {t.is_contiguous()}")
            if tuple(t.shape) != tuple(expected[key]):
                raise ValueError(f"{key} must have shape {tuple(expected[key])}, got {tuple(t.shape)}")
            if not indexed:
                setattr(w, member, t.data_ptr())
            elif sub:
                setattr(getattr(w, array)[i], sub[1:], t.data_ptr())
            else:
                getattr(w, array)[i] = t.data_ptr()
    return w


class DeviceSlotTracker:
    """Slot-tracker state for B envs: the stored input slots, whatever the model carries from step to step, and the engine surface of
    cirs_hip.tracker.DeviceTracker (init / step / backward / adam_update), so that the rollout, the learner and the plugin classes drive
    any of them.  A subclass names its model: the ctypes structs, FIELDS (the table of its own weight members and their state_dict names),
    the prefix of its entry points, its shape check and param_shapes, and the carried tensors (CARRY: [nlayers, B, 32] each; () where
    the model reads the stored slots only).  One with model arguments of its own sets them before the base constructor runs and says in
    _cell_cfg, _shape_kw and _live what they mean for the cfg, for param_shapes and for the indexed members."""
    CFG = WEIGHTS = STATE = ENTRY = check_shape = param_shapes = None
    FIELDS = ()
    CARRY = ("h",)

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        table = [m for m, _ in HEAD_FIELDS + list(cls.FIELDS) + DECODER_FIELDS]
        if table != struct_members(cls.WEIGHTS):
            raise TypeError(f"{cls.__name__}.FIELDS does not spell the members of {cls.WEIGHTS.__name__}: {table} != {struct_members(cls.WEIGHTS)}")

    def __init__(self, params: Dict[str, torch.Tensor], n_users, n_items, n_env, max_turn, *, dim_model=32, dim_state=20, nlayers=1,
                 device="cuda"):
        self.max_len, self.nlayers = max_turn + 1, nlayers
        cell = self._cell_cfg(dim_model, dim_state, nlayers)
        self.device = torch.device(device)
        self.cfg = self.CFG(n_users=n_users, n_items=n_items, dim_model=dim_model, dim_state=dim_state, max_len=max_turn + 1, n_env=n_env, **cell)
        self.shapes = type(self).param_shapes(n_users, n_items, dim_model, dim_state, **self._shape_kw())
        self.params = params
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
        """The shape check of this build, then the members of the cfg struct that describe the model."""
        type(self).check_shape(dim_model, dim_state, nlayers)
        return {"nlayers": nlayers}

    def _shape_kw(self):
        """The model arguments as param_shapes takes them."""
        return {"nlayers": self.nlayers}

    def _live(self):
        """How many indices of FIELDS' indexed members are in use."""
        return self.nlayers

    def _weights(self, tensors):
        return fill_weights(self.WEIGHTS, self.FIELDS, self._live(), self.shapes, tensors)

    def _state(self, x_hist):
        return self.STATE(x_hist=x_hist.data_ptr(), len=self.len.data_ptr(), **{k: getattr(self, k).data_ptr() for k in self.CARRY})

    def _entry(self, suffix):
        return getattr(self._lib, self.ENTRY + suffix), self.ENTRY + suffix

    # nn.GRU / nn.LSTM have dropout between layers only, and that one is not built; the other models' sites are not built: nothing to set
    def set_dropout(self, p: float):
        pass

    def set_dropout_key(self, seed: int, tag: int = 0, env_base: int = 0):
        pass

    def refresh_weights(self):
        self.w = self._weights(self.params)

    # ---- training side ------------------------------------------------------------------------------------------
    def enable_training(self, flat_params: torch.Tensor, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        """`flat_params` must be the flat buffer self.params' tensors are views of (tracker.flat_tracker_params)."""
        from .tracker import flat_tracker_params      # tracker.py takes TOP_FIELDS and the shared shapes from here
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
