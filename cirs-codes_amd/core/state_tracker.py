"""StateTrackerTransformer (reference core/state_tracker.py:128-250), StateTrackerGRU and StateTrackerLSTM (:282-289, declared empty
there), StateTrackerAvg (a pooled window over the last items; no counterpart there), StateTrackerCaser (Caser's convolutions over that
window; no counterpart there either), StateTrackerNextItNet (NextItNet's dilated causal convolutions over the item slots; no counterpart
either), StateTrackerSTAMP (STAMP's attention pool over that window; no counterpart either), StateTrackerNARM (NARM's GRU encoder with
attention over its hidden states; no counterpart either), StateTrackerFMLP (FMLP-Rec's learnable filter and feed-forward block over that
window; no counterpart either) and StateTrackerLRU (a linear recurrent unit, the diagonal complex recurrence of LRURec, with that
feed-forward block; no counterpart either) on the device engines.

Same constructor keywords and the same three `build_state` call forms the Collector uses (collector.py:127-134,261-269).
Parameters are exposed under state_dict names (the reference's; torch.nn.GRU's / nn.LSTM's for the recurrence) but live in ONE flat device
buffer; the forward is a one-launch step kernel (csrc/tracker.hip: KV-cached decode, csrc/gru_tracker.hip: GRU cells, csrc/lstm_tracker.hip:
LSTM cells, csrc/avg_tracker.hip: the window mean, csrc/caser_tracker.hip: the window's convolutions, csrc/nextitnet_tracker.hip: the dilated
blocks, csrc/stamp_tracker.hip: the attention pool, csrc/narm_tracker.hip: the GRU cell and the attention over its hidden states,
csrc/fmlp_tracker.hip: the filter and the feed-forward block, csrc/lru_tracker.hip: the linear recurrence and the feed-forward block) and the
gradient arrives through cirs_tracker_backward /
cirs_gru_tracker_backward / cirs_lstm_tracker_backward / cirs_avg_tracker_backward / cirs_caser_tracker_backward /
cirs_nextitnet_tracker_backward / cirs_stamp_tracker_backward / cirs_narm_tracker_backward / cirs_fmlp_tracker_backward /
cirs_lru_tracker_backward (no autograd graph)."""
import numpy as np
import torch
from torch import nn

from cirs_hip.avg_tracker import DeviceAvgTracker, avg_param_shapes, check_avg_shape, init_avg_tracker_params
from cirs_hip.caser_tracker import DeviceCaserTracker, caser_param_shapes, check_caser_shape, init_caser_tracker_params
from cirs_hip.engine import init_tracker_params
from cirs_hip.fmlp_tracker import DeviceFmlpTracker, check_fmlp_shape, fmlp_param_shapes, init_fmlp_tracker_params
from cirs_hip.gru_tracker import DeviceGruTracker, check_gru_shape, gru_param_shapes, init_gru_tracker_params
from cirs_hip.lru_tracker import DeviceLruTracker, check_lru_shape, init_lru_tracker_params, lru_param_shapes
from cirs_hip.lstm_tracker import DeviceLstmTracker, check_lstm_shape, init_lstm_tracker_params, lstm_param_shapes
from cirs_hip.narm_tracker import DeviceNarmTracker, check_narm_shape, init_narm_tracker_params, narm_param_shapes
from cirs_hip.nextitnet_tracker import DeviceNextItNetTracker, check_nextitnet_shape, init_nextitnet_tracker_params, nextitnet_param_shapes
from cirs_hip.stamp_tracker import DeviceStampTracker, check_stamp_shape, init_stamp_tracker_params, stamp_param_shapes
from cirs_hip.tracker import DeviceTracker, flat_tracker_params, tracker_param_shapes


class _DeviceStateTracker(nn.Module):
    """What the device state trackers share: the flat parameter buffer under state_dict names, one engine per (env count, owner)
    with shared gradient / Adam state, the three build_state call forms.  A subclass builds its engine in _make_engine."""

    def _setup(self, shapes, init, seed):
        self.flat, views = flat_tracker_params(shapes, device=self.device, init=init)
        self._views = views
        for name, v in views.items():  # register under the state_dict names (dots -> nested attribute path)
            self._register(name, nn.Parameter(v, requires_grad=False))
        self._engines = {}   # n_env -> device engine (all share the flat parameter buffer)
        self._n_env = None
        self._train_state = None  # (flat_grad, grad_views, adam_m, adam_v) shared by whichever engine runs the backward
        self.adam_steps = 0
        # key of the dropout masks of the per-step protocol (build_state without a DeviceRollout): (seed, reset counter) -- every
        # reset starts a rollout with fresh masks, like the reference's fresh nn.Dropout noise at every call
        self._drop_seed, self._drop_resets = int(seed), 0

    def _engine_dropout(self, training):
        """Dropout probability the engines run with in this mode."""
        return self.dropout_p if training else 0.0

    def _make_engine(self, n_env):
        raise NotImplementedError

    def _register(self, dotted, param):
        mod = self
        parts = dotted.split(".")
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, nn.Module())
            mod = getattr(mod, p)
        mod.register_parameter(parts[-1], param)

    def load_state_dict(self, sd, strict=True):
        with torch.no_grad():
            for k, v in self._views.items():
                v.copy_(torch.as_tensor(sd[k]).to(v.device, v.dtype).reshape(v.shape))

    def engine(self, n_env=None, owner=None):
        """Device engine for a vector env of n_env envs; the parameters and the Adam state are shared, the history slots
        (the reference's self.data) and K/V caches / hidden states are per engine.  `owner`: every Collector passes itself, so that two
        collectors with the same env count (training_num == test_num == 100 in CIRS-RL-kuaishou.py) never share slots — the
        tracker backward of policy.update(train_buffer) re-reads the slots of the TRAIN rollout even if a test rollout ran
        in between (onpolicy.py:65-72 with stop_fn + test_in_train).  owner=None: the per-step build_state protocol."""
        n_env = n_env or self._n_env
        key = n_env if owner is None else (n_env, id(owner))
        if owner is not None:
            self._owners = getattr(self, "_owners", {})
            self._owners[id(owner)] = owner      # pin the id
        if key not in self._engines:
            eng = self._make_engine(n_env)
            eng.set_dropout(self._engine_dropout(self.training))
            eng.enable_training(self.flat)
            if self._train_state is None:
                self._train_state = (eng.flat_grad, eng.grad_views, eng.g, eng.adam_m, eng.adam_v)
            else:
                eng.flat_grad, eng.grad_views, eng.g, eng.adam_m, eng.adam_v = self._train_state
            self._engines[key] = eng
        if owner is None:
            self._n_env = n_env
        return self._engines[key]

    def train(self, mode: bool = True):
        super().train(mode)
        for eng in getattr(self, "_engines", {}).values():
            eng.set_dropout(self._engine_dropout(mode))
        return self

    def build_state(self, obs=None, env_id=None, obs_next=None, rew=None, done=None, info=None, policy=None, dim_batch=None,
                    reset=False):
        if reset and dim_batch:
            eng = self.engine(dim_batch)
            eng.reset()
            # the per-step engine is keyed here (DeviceRollout.collect keys the fused one): without it every episode of the
            # stepwise protocol (Collector.collect(random=True), external preprocess_fn users) would reuse the masks of key 0
            self._drop_resets += 1
            eng.set_dropout_key(self._drop_seed, (1 << 40) + self._drop_resets, 0)
            return
        eng = self.engine(self._n_env)
        ids = None if env_id is None else torch.as_tensor(np.asarray(env_id).astype(np.int32)).to(self.device)
        if obs is not None:
            users = torch.as_tensor(np.asarray(obs).reshape(-1))
            return {"obs": eng.init(users, ids)}
        if obs_next is not None:
            items = torch.as_tensor(np.asarray(obs_next).reshape(-1))
            r = torch.as_tensor(np.asarray(rew, dtype=np.float64).reshape(-1))
            return {"obs_next": eng.step(items, r, ids)}
        return {}


class StateTrackerTransformer(_DeviceStateTracker):
    def __new__(cls, user_columns=None, action_columns=None, feedback_columns=None, *args, **kwargs):
        """VirtualTB-v0 (BASELINE configs[0]: CPU plumbing, dense features) is served by the host tracker of core.host_rl, exactly
        as the reference runs it on the CPU; KuaishouEnv-v0 by the device engine below."""
        dataset = kwargs.get("dataset", args[4] if len(args) > 4 else None)
        if dataset is None:      # not given: sparse id columns mean the KuaishouEnv tracker, all-dense columns the VirtualTB one
            from deepctr_torch.inputs import SparseFeat
            dataset = "KuaishouEnv-v0" if any(isinstance(c, SparseFeat) for c in list(user_columns or []) + list(action_columns or [])) else "VirtualTB-v0"
        if cls is StateTrackerTransformer and dataset == "VirtualTB-v0":
            from core.host_rl import HostStateTracker
            return HostStateTracker(user_columns, action_columns, feedback_columns, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, user_columns, action_columns, feedback_columns, dim_model, dim_state, dim_max_batch, dropout=0.1,
                 dataset="KuaishouEnv-v0", has_user_embedding=True, has_action_embedding=True, has_feedback_embedding=False,
                 nhead=8, d_hid=128, nlayers=2, device="cpu", seed=2021, init_std=0.0001, padding_idx=None, MAX_TURN=100):
        super().__init__()
        if dataset != "KuaishouEnv-v0":
            raise NotImplementedError("the device tracker serves KuaishouEnv-v0; VirtualTB-v0 dispatches to core.host_rl.HostStateTracker")
        self.dataset, self.device = dataset, torch.device(device if str(device) != "cpu" else "cuda")
        self.dim_model, self.dim_state, self.nhead, self.d_hid, self.nlayers = dim_model, dim_state, nhead, d_hid, nlayers
        self.MAX_TURN = MAX_TURN + 1
        self.n_users, self.n_items = user_columns[0].vocabulary_size, action_columns[0].vocabulary_size
        # nn.Dropout(p) of PositionalEncoding and of both encoder layers (core/state_tracker.py:155-156): live while the module is in
        # training mode -- which in the reference's scripts is ALWAYS (the tracker is not a sub-module of the policy, so
        # policy.eval() never reaches it).  state_tracker.eval() switches it off (the mode of the parity fixtures).
        self.dropout_p = float(dropout)
        init = init_tracker_params(self.n_users, self.n_items, MAX_TURN, seed=seed, dim_model=dim_model, dim_state=dim_state,
                                   nhead=nhead, d_hid=d_hid, nlayers=nlayers, init_std=init_std)
        self._setup(tracker_param_shapes(self.n_users, self.n_items, dim_model, dim_state, d_hid, nlayers), init, seed)
        self.register_buffer("pe", init["pos_encoder.pe"].to(self.device))

    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        prefix = kwargs.get("prefix", args[1] if len(args) > 1 else "")
        if prefix + "pe" in sd:
            sd[prefix + "pos_encoder.pe"] = sd.pop(prefix + "pe")
        return sd

    def _make_engine(self, n_env):
        params = dict(self._views)
        params["pos_encoder.pe"] = self.pe
        return DeviceTracker(params, self.n_users, self.n_items, n_env, self.MAX_TURN - 1, dim_model=self.dim_model,
                             dim_state=self.dim_state, nhead=self.nhead, d_hid=self.d_hid, nlayers=self.nlayers, device=self.device)


class _RecurrentStateTracker(_DeviceStateTracker):
    """What the plugin classes of the slot trackers (every subclass below) share: StateTrackerTransformer's constructor keywords (a script
    changes the class name only; nhead is accepted and unused, d_hid is kept as an attribute for the _check_model that reads it) plus the
    subclass's own (the keywords of its _check_model, with their defaults), the refusals, the engine.  A subclass names itself (CELL), its
    device engine and the functions of its cirs_hip module; one whose model is not "nlayers cells" says in _check_model and _model_kw what
    it is instead.  dropout: torch applies it between the layers only -- without effect at nlayers == 1 (as in torch); at nlayers == 2 it
    is not built and training mode with dropout > 0 raises."""
    CELL = ENGINE = check_shape = param_shapes = init_params = None

    def __init__(self, user_columns, action_columns, feedback_columns, dim_model, dim_state, dim_max_batch, dropout=0.0,
                 dataset="KuaishouEnv-v0", has_user_embedding=True, has_action_embedding=True, has_feedback_embedding=False,
                 nhead=8, d_hid=128, nlayers=1, device="cpu", seed=2021, init_std=0.0001, padding_idx=None, MAX_TURN=100, **model_kw):
        super().__init__()
        cls = type(self)
        self.d_hid = d_hid
        if dataset != "KuaishouEnv-v0":
            raise NotImplementedError(f"StateTracker{self.CELL} serves KuaishouEnv-v0 only (VirtualTB-v0 is out of scope)")
        self._check_model(dim_model, dim_state, nlayers, dropout, MAX_TURN + 1, **model_kw)
        self.dataset, self.device = dataset, torch.device(device if str(device) != "cpu" else "cuda")
        self.dim_model, self.dim_state = dim_model, dim_state
        self.MAX_TURN = MAX_TURN + 1
        self.n_users, self.n_items = user_columns[0].vocabulary_size, action_columns[0].vocabulary_size
        kw = dict(dim_model=dim_model, dim_state=dim_state, **self._model_kw())
        init = cls.init_params(self.n_users, self.n_items, seed=seed, init_std=init_std, **kw)
        self._setup(cls.param_shapes(self.n_users, self.n_items, **kw), init, seed)

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len):
        """Refuse a model that is not built; set the model arguments (the subclass's own keywords among them), nlayers and dropout_p as
        attributes.  An unknown keyword of the constructor ends here, as Python's TypeError."""
        type(self).check_shape(dim_model, dim_state, nlayers)
        self.dropout_p, self.nlayers = float(dropout), int(nlayers)
        self._check_dropout(self.training)

    def _model_kw(self):
        """The model arguments as init_params and param_shapes take them -- and ENGINE, unless _engine_kw says otherwise."""
        return dict(nlayers=self.nlayers)

    def _engine_kw(self):
        return self._model_kw()

    def _check_dropout(self, training):
        if training and self.nlayers > 1 and self.dropout_p > 0:
            raise ValueError(f"StateTracker{self.CELL}: dropout between {self.CELL} layers is not built (nlayers == 2 with dropout > 0 in "
                             "training mode); use dropout=0.0 or call .eval()")

    def _engine_dropout(self, training):
        return 0.0

    def _make_engine(self, n_env):
        return self.ENGINE(dict(self._views), self.n_users, self.n_items, n_env, self.MAX_TURN - 1, dim_model=self.dim_model,
                           dim_state=self.dim_state, device=self.device, **self._engine_kw())

    def train(self, mode: bool = True):
        self._check_dropout(mode)
        return super().train(mode)


class StateTrackerGRU(_RecurrentStateTracker):
    """The recurrent tracker the reference announces (core/state_tracker.py:282-289: an empty class): the Transformer tracker's input
    slots, torch.nn.GRU(dim_model, dim_model, nlayers) with h_{-1} = 0 over them, the same decoder."""
    CELL, ENGINE = "GRU", DeviceGruTracker
    check_shape, param_shapes, init_params = check_gru_shape, gru_param_shapes, init_gru_tracker_params


class StateTrackerLSTM(_RecurrentStateTracker):
    """The second recurrent tracker the reference announces and leaves empty: the same input slots, torch.nn.LSTM(dim_model, dim_model,
    nlayers) with h_{-1} = c_{-1} = 0 over them, the same decoder."""
    CELL, ENGINE = "LSTM", DeviceLstmTracker
    check_shape, param_shapes, init_params = check_lstm_shape, lstm_param_shapes, init_lstm_tracker_params


class StateTrackerAvg(_RecurrentStateTracker):
    """The cheapest tracker: the same input slots, h_p = x_0 + the mean of the last `window_size` item slots, the same decoder (DESIGN.md
    7.4; the reference has no counterpart).  StateTrackerTransformer's constructor keywords plus window_size; nhead, d_hid, nlayers and
    dropout are accepted and unused (the model has no dropout site).  No sequence model, but the engine surface, the collect and every
    refusal of the recurrent trackers: a _RecurrentStateTracker to whatever asks."""
    CELL, ENGINE, param_shapes, init_params = "Avg", DeviceAvgTracker, avg_param_shapes, init_avg_tracker_params

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len, window_size=10):
        check_avg_shape(dim_model, dim_state, window_size, max_len)
        self.window_size = int(window_size)
        self.dropout_p, self.nlayers = 0.0, 0

    def _model_kw(self):
        return {}      # the window has no parameters

    def _engine_kw(self):
        return dict(window_size=self.window_size)


class StateTrackerCaser(_RecurrentStateTracker):
    """The convolutional window tracker: the same input slots, the window of the last `window_size` item slots through Caser's horizontal
    filter banks (heights `filter_sizes`, `num_filters` each, max-pooled over time) and its vertical filter, one fc layer, h_p = x_0 + z, the
    same decoder (the reference has no counterpart).  StateTrackerTransformer's constructor keywords plus window_size,
    filter_sizes and num_filters; nhead, d_hid and nlayers are accepted and unused.  Caser's dropout on the concatenation is not built:
    dropout > 0 in training mode raises.  A _RecurrentStateTracker to whatever asks: the engine surface, the collect, every refusal."""
    CELL, ENGINE, param_shapes, init_params = "Caser", DeviceCaserTracker, caser_param_shapes, init_caser_tracker_params

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len, window_size=10, filter_sizes=(2, 3, 4), num_filters=16):
        check_caser_shape(dim_model, dim_state, window_size, filter_sizes, num_filters, max_len)
        self.window_size, self.filter_sizes, self.num_filters = int(window_size), tuple(int(h) for h in filter_sizes), int(num_filters)
        self.dropout_p, self.nlayers = float(dropout), 0
        self._check_dropout(self.training)

    def _model_kw(self):
        return dict(window_size=self.window_size, filter_sizes=self.filter_sizes, num_filters=self.num_filters)

    def _check_dropout(self, training):
        if training and self.dropout_p > 0:
            raise ValueError("StateTrackerCaser: dropout on the concatenation is not built (dropout > 0 in training mode); use dropout=0.0 or "
                             "call .eval()")


class StateTrackerNextItNet(_RecurrentStateTracker):
    """The dilated-convolution tracker: the same input slots, NextItNet's residual blocks -- nn.Conv1d(32, 32, 3, dilation=d_l) with causal
    left padding, nn.LayerNorm(32), ReLU on a residual branch -- over the item slots, h_p = x_0 + the top block's last position, the same
    decoder (the reference has no counterpart).  StateTrackerTransformer's constructor keywords plus dilations and
    kernel_size; nhead, d_hid, nlayers and dropout are accepted and unused (the model has no dropout site).  A _RecurrentStateTracker to
    whatever asks: the engine surface, the collect, every refusal."""
    CELL, ENGINE, param_shapes, init_params = "NextItNet", DeviceNextItNetTracker, nextitnet_param_shapes, init_nextitnet_tracker_params

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len, dilations=(1, 2, 4), kernel_size=3):
        check_nextitnet_shape(dim_model, dim_state, dilations, kernel_size, max_len)
        self.dilations, self.kernel_size = tuple(int(d) for d in dilations), int(kernel_size)
        self.dropout_p, self.nlayers = 0.0, 0

    def _model_kw(self):
        return dict(dilations=self.dilations)

    def _engine_kw(self):
        return dict(dilations=self.dilations, kernel_size=self.kernel_size)


class StateTrackerSTAMP(_RecurrentStateTracker):
    """The attention-pool tracker: the same input slots, STAMP's short-term attention over the window of the last `window_size` item slots --
    a general-interest query (the window mean), a last-click query (the newest slot), a sigmoid gate network without softmax, the read-out
    tanh(A m_a + b_A) * tanh(B m_t + b_B) -- h_p = x_0 + that product, the same decoder (the reference has no counterpart).
    StateTrackerTransformer's constructor keywords plus window_size (1..16); nhead, d_hid, nlayers and dropout are accepted and unused (the
    model has no dropout site).  A _RecurrentStateTracker to whatever asks: the engine surface, the collect, every refusal."""
    CELL, ENGINE, param_shapes, init_params = "STAMP", DeviceStampTracker, stamp_param_shapes, init_stamp_tracker_params

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len, window_size=10):
        check_stamp_shape(dim_model, dim_state, window_size, max_len)
        self.window_size = int(window_size)
        self.dropout_p, self.nlayers = 0.0, 0

    def _model_kw(self):
        return {}      # the window has no parameters

    def _engine_kw(self):
        return dict(window_size=self.window_size)


class StateTrackerNARM(_RecurrentStateTracker):
    """The GRU encoder with attention over its hidden states: the same input slots, torch.nn.GRU(dim_model, dim_model, 1) with h_{-1} = 0 over
    them, NARM's additive attention of position p over every hidden state so far -- alpha_{p,j} = v . sigmoid(A1 h_p + A2 h_j), no softmax,
    c_p = sum_j alpha_{p,j} h_j -- the bilinear read-out Bw [h_p ; c_p], the same decoder (the reference has no counterpart).
    StateTrackerTransformer's constructor keywords; nhead and d_hid are accepted and unused; nlayers must be 1 (one encoder layer is built).
    dropout is accepted and unused: the paper's two dropout sites (on the item embeddings and in front of the bilinear read-out) are not
    built.  A _RecurrentStateTracker to whatever asks: the engine surface, the collect, every refusal."""
    CELL, ENGINE, param_shapes, init_params = "NARM", DeviceNarmTracker, narm_param_shapes, init_narm_tracker_params

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len):
        check_narm_shape(dim_model, dim_state, nlayers, max_len)
        self.dropout_p, self.nlayers = 0.0, int(nlayers)


class StateTrackerFMLP(_RecurrentStateTracker):
    """The filter-MLP tracker: the same input slots, FMLP-Rec's layers over the tile of the last `window_size` item slots -- a learned
    per-channel circular filter whose parameters live in the frequency domain (complex_weight [W//2+1, 32, 2]), LayerNorm, the 32 -> 128 -> 32
    feed-forward block with the exact GELU, LayerNorm -- h_p = x_0 + the top layer's newest row, the same decoder (the
    reference has no counterpart).  The ablation partner of StateTrackerTransformer: its constructor keywords plus window_size (1..16);
    nlayers must be 1 or 2 and d_hid 128; nhead is accepted and unused.  dropout is accepted and unused: FMLP-Rec's two dropout sites (after
    the filter, after dense_2) are not built.  A _RecurrentStateTracker to whatever asks: the engine surface, the collect, every refusal."""
    CELL, ENGINE, param_shapes, init_params = "FMLP", DeviceFmlpTracker, fmlp_param_shapes, init_fmlp_tracker_params

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len, window_size=10):
        check_fmlp_shape(dim_model, dim_state, window_size, nlayers, self.d_hid, max_len)
        self.window_size, self.d_hid = int(window_size), int(self.d_hid)
        self.dropout_p, self.nlayers = 0.0, int(nlayers)

    def _model_kw(self):
        return dict(window_size=self.window_size, nlayers=self.nlayers)


class StateTrackerLRU(_RecurrentStateTracker):
    """The linear-recurrence tracker: the same input slots, a linear recurrent unit over them -- the diagonal complex recurrence
    h_p = lambda * h_{p-1} + gamma * (W_in x_p + b_in) with lambda = exp(-exp(nu_log) + i exp(theta_log)), |lambda| < 1 by construction, 64 carried
    floats per env whatever the position -- the real read-out W_out [h_re ; h_im] + b_out, LayerNorm on the residual, the 32 -> 128 -> 32
    feed-forward block with the exact GELU, LayerNorm, the same decoder (the reference has no counterpart).
    StateTrackerTransformer's constructor keywords; nlayers must be 1 and d_hid 128; nhead is accepted and unused.  dropout is accepted and
    unused: LRURec's dropout sites are not built.  A _RecurrentStateTracker to whatever asks: the engine surface, the collect, every refusal."""
    CELL, ENGINE, param_shapes, init_params = "LRU", DeviceLruTracker, lru_param_shapes, init_lru_tracker_params

    def _check_model(self, dim_model, dim_state, nlayers, dropout, max_len):
        check_lru_shape(dim_model, dim_state, nlayers, self.d_hid, max_len)
        self.d_hid = int(self.d_hid)
        self.dropout_p, self.nlayers = 0.0, int(nlayers)
