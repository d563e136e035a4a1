"""Device-resident batched VirtualTaobao: VirtualTB-v0 (raw kind) and SimulatedEnv(VirtualTB-v0) (simulated kind), one launch per
vector step (csrc/virtualtb.hip through cirs_vtb_reset / cirs_vtb_step).

Host-side counterpart of environments/VirtualTaobao/virtualTB/envs/virtualTB.py (VirtualTB) and the VirtualTB branch of
core/env/simulatedEnv/simulated_env.py, which step one env at a time.  The weights come from a mirror VirtualTB (generator, action
model) and, for the simulated kind, from a UserModel_MMOE; they go up once.  The noise is counter-based (Philox, key = seed), not
torch's CPU generator: `noise(ids, events)` returns exactly what the kernels draw for those events, so a CPU mirror fed with it
reproduces a device run.
"""
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import abi

USER_DIM, ACTION_DIM, GROUPS, NOISE_COLS = 88, 27, 11, 237


def _t(w, device):
    """[out, in] torch weight -> contiguous fp32 [in, out] on the device (the kernels' layout)."""
    return w.detach().to(torch.float32).t().contiguous().to(device)


def _v(w, device):
    return w.detach().to(torch.float32).reshape(-1).contiguous().to(device)


def _linears(seq):
    return [m for m in seq if isinstance(m, torch.nn.Linear)]


def _mmoe_shape(model):
    """The MMoE shape fields of cirs_vtb_cfg, read off the module (the library rejects what it does not support)."""
    dnn = model.dnn.linears
    mm = model.mmoe_layer
    return dict(mmoe_d_in=int(dnn[0].in_features), mmoe_dnn_layers=len(dnn), mmoe_h1=int(dnn[0].out_features),
                mmoe_h2=int(dnn[-1].out_features), mmoe_experts=int(mm.num_experts), mmoe_expert_dim=int(mm.out_dim),
                mmoe_tasks=len(model.tower_network), mmoe_task_dim=int(model.tower_network[0].out_features))


def env_weights(vtb_env, dev):
    """The generator's and the action model's fields of cirs_vtb_weights as device tensors, read off a host VirtualTB."""
    g, a = _linears(vtb_env.generator), _linears(vtb_env.action_model)
    if [(m.in_features, m.out_features) for m in g] != [(128, 128), (128, USER_DIM)] or \
            [(m.in_features, m.out_features) for m in a] != [(USER_DIM + 1 + ACTION_DIM, 128), (128, 256), (256, 21)]:
        raise ValueError("unexpected VirtualTB generator / action-model shapes")
    return dict(gen_w1=_t(g[0].weight, dev), gen_b1=_v(g[0].bias, dev), gen_w2=_t(g[1].weight, dev), gen_b2=_v(g[1].bias, dev),
                act_w1=_t(a[0].weight, dev), act_b1=_v(a[0].bias, dev), act_w2=_t(a[1].weight, dev), act_b2=_v(a[1].bias, dev),
                act_w3=_t(a[2].weight, dev), act_b3=_v(a[2].bias, dev))


class DeviceVirtualTB:
    """n_env VirtualTaobao envs stepped by one kernel launch.  user_model=None: raw VirtualTB-v0 (reward = clicks); otherwise
    SimulatedEnv(VirtualTB-v0) with that UserModel_MMOE and the exposure effect."""

    def __init__(self, vtb_env, n_env: int, *, user_model=None, version="v1", tau=1.0, gamma_exposure=1.0,
                 use_exposure_intervention=True, seed=0, device="cuda"):
        if getattr(vtb_env, "static", False):
            raise ValueError("the static state mode (set_state_mode(True)) is not supported by the device env")
        self.device = torch.device(device)
        self.n_env = int(n_env)
        if self.n_env <= 0:
            raise ValueError("n_env must be positive")
        self.max_turn = int(vtb_env.max_turn)
        self.simulated = user_model is not None
        ver = {"v1": 1, "v2": 2}.get(version, version)
        shape = _mmoe_shape(user_model) if self.simulated else dict(
            mmoe_d_in=118, mmoe_dnn_layers=2, mmoe_h1=128, mmoe_h2=128, mmoe_experts=4, mmoe_expert_dim=8, mmoe_tasks=1, mmoe_task_dim=1)
        self.cfg = abi.VtbCfg(n_env=self.n_env, max_turn=self.max_turn, num_leave_compute=int(vtb_env.num_leave_compute),
                              simulated=int(self.simulated), version=int(ver), use_exposure=int(bool(use_exposure_intervention)),
                              leave_threshold=float(vtb_env.leave_threshold), tau=float(tau), gamma_exposure=float(gamma_exposure), **shape)
        dev = self.device
        w = env_weights(vtb_env, dev)
        if self.simulated:
            m = user_model
            w.update(mm_w1=_t(m.dnn.linears[0].weight, dev), mm_b1=_v(m.dnn.linears[0].bias, dev),
                     mm_w2=_t(m.dnn.linears[-1].weight, dev), mm_b2=_v(m.dnn.linears[-1].bias, dev),
                     mm_we=_t(m.mmoe_layer.expert_network.weight, dev), mm_be=_v(m.mmoe_layer.expert_network.bias, dev),
                     mm_wg=_t(m.mmoe_layer.gating_networks[0].weight, dev), mm_wt=_v(m.tower_network[0].weight, dev),
                     mm_wlin=_v(m.linear_model_task[0].weight, dev), mm_bias=_v(m.out[0].bias, dev))
        self._w = w    # keeps the tensors alive
        self._wst = abi.VtbWeights(**{k: t.data_ptr() for k, t in w.items()})
        B, T = self.n_env, self.max_turn
        self.task_user = torch.zeros((B, GROUPS), dtype=torch.int32, device=dev)
        self.sim_user = torch.zeros((B, GROUPS), dtype=torch.int32, device=dev)
        self.turn = torch.zeros(B, dtype=torch.int32, device=dev)
        self.event = torch.zeros(B, dtype=torch.int32, device=dev)    # uint32 on the device side
        self.prev_reward = torch.zeros(B, dtype=torch.float64, device=dev)
        self.cum_reward = torch.zeros(B, dtype=torch.float64, device=dev)
        self.lst_action = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        self.hist = torch.zeros((B, T, ACTION_DIM), dtype=torch.float32, device=dev)
        self._st = abi.VtbState(**{k: getattr(self, k).data_ptr() for k in
                                   ("task_user", "sim_user", "turn", "event", "prev_reward", "cum_reward", "lst_action", "hist")})
        self.host_turn = np.zeros(B, np.int64)       # each env's turn, tracked on the host (no device read)
        self._was_reset = np.zeros(B, bool)
        self._seed = int(seed)
        self._lib = abi.lib()
        self._pinned = {}

    # ---- plumbing ----------------------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ids(self, ids, n_default=None):
        if ids is None:
            return np.arange(self.n_env if n_default is None else n_default, dtype=np.int32)
        if isinstance(ids, torch.Tensor):
            ids = ids.cpu().numpy()
        ids = np.atleast_1d(np.asarray(ids)).astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= self.n_env):
            raise ValueError(f"env ids must lie in [0, {self.n_env})")
        if len(np.unique(ids)) != len(ids):
            raise ValueError("env ids of one call must be distinct")
        return ids.astype(np.int32)

    def _buf(self, name, nbytes, pinned):
        key = (name, pinned)
        b = self._pinned.get(key)
        if b is None or b.numel() < nbytes:
            b = torch.empty(max(nbytes, 64), dtype=torch.uint8, pin_memory=True) if pinned else \
                torch.empty(max(nbytes, 64), dtype=torch.uint8, device=self.device)
            self._pinned[key] = b
        return b

    def seed(self, s=0):
        """Philox key = s; the per-env event counters restart, so the same seed replays the same noise."""
        self._seed = int(s) & ((1 << 64) - 1)
        self.event.zero_()

    # ---- protocol ----------------------------------------------------------------------------------------------------------
    def reset(self, ids=None) -> torch.Tensor:
        """Draw a user for each env of `ids` (default: all) and clear its turn, rewards and history -> obs fp64 [k, 91]."""
        ids_np = self._ids(ids)
        k = len(ids_np)
        obs = torch.empty((k, USER_DIM + 3), dtype=torch.float64, device=self.device)
        if k == 0:
            return obs
        d_ids = torch.from_numpy(ids_np).to(self.device, non_blocking=False)
        abi.check(self._lib.cirs_vtb_reset(C.byref(self.cfg), C.byref(self._wst), C.byref(self._st), self._seed, d_ids.data_ptr(), k,
                                           obs.data_ptr(), self._stream()), "cirs_vtb_reset")
        self.host_turn[ids_np] = 0
        self._was_reset[ids_np] = True
        return obs

    def _check_turns(self, ids_np):
        if not self._was_reset[ids_np].all():
            raise ValueError("step() on an env that was never reset")
        if self.simulated and (self.host_turn[ids_np] > self.max_turn).any():
            raise ValueError(f"SimulatedEnv(VirtualTB-v0) cannot step past turn {self.max_turn} without a reset "
                             "(the reference's exposure effect fails there too)")

    def _launch(self, actions_ptr, ids_ptr, k, out, want_exposure):
        """out: a device byte buffer; obs [k,30] f64 | rew [k] f64 | ctr [k] f64 | expo [k] f64 | done [k] u8 packed in that order."""
        o = out.data_ptr()
        p_obs, p_rew = o, o + 8 * 30 * k
        p_ctr, p_expo = p_rew + 8 * k, p_rew + 16 * k
        p_done = p_rew + 24 * k
        abi.check(self._lib.cirs_vtb_step(C.byref(self.cfg), C.byref(self._wst), C.byref(self._st), self._seed, actions_ptr, ids_ptr, k,
                                          p_obs, p_rew, p_done, p_ctr, p_expo if want_exposure else None, self._stream()),
                  "cirs_vtb_step")

    @staticmethod
    def _packed_bytes(k):
        return 8 * 33 * k + k

    @staticmethod
    def _unpack(buf, k):
        f = buf[:8 * 33 * k].view(torch.float64)
        return f[:30 * k].view(k, 30), f[30 * k:31 * k], buf[8 * 33 * k:8 * 33 * k + k], f[31 * k:32 * k], f[32 * k:33 * k]

    def step(self, actions, ids=None, want_exposure=False):
        """actions [k, 27] (fp32 on the device or the host) for envs `ids` -> (obs fp64 [k,30], rew fp64 [k], done u8 [k], ctr fp64 [k]),
        device tensors (plus the exposure effect fp64 [k] when want_exposure)."""
        ids_np = self._ids(ids, None if ids is not None else self.n_env)
        k = len(ids_np)
        self._check_turns(ids_np)
        a = torch.as_tensor(actions).to(device=self.device, dtype=torch.float32).reshape(k, ACTION_DIM).contiguous()
        d_ids = torch.from_numpy(ids_np).to(self.device)
        out = torch.empty(self._packed_bytes(k), dtype=torch.uint8, device=self.device)
        if k:
            self._launch(a.data_ptr(), d_ids.data_ptr(), k, out, want_exposure)
        self.host_turn[ids_np] += 1
        obs, rew, done, ctr, expo = self._unpack(out, k)
        return (obs, rew, done, ctr, expo) if want_exposure else (obs, rew, done, ctr)

    def step_numpy(self, actions: np.ndarray, ids: np.ndarray):
        """The vector-env path: one H2D copy of (actions, ids), one launch, one packed D2H copy into pinned memory.  Returns numpy views
        (obs [k,30], rew [k], done [k] bool, ctr [k]) that stay valid until the next call."""
        ids_np = self._ids(ids)
        k = len(ids_np)
        self._check_turns(ids_np)
        words = k * (ACTION_DIM + 1)
        h_in = self._buf("in", 4 * words, True)
        fin = h_in[:4 * words].view(torch.float32)
        fin[:k * ACTION_DIM].numpy().reshape(k, ACTION_DIM)[:] = np.asarray(actions, np.float32).reshape(k, ACTION_DIM)
        h_in[4 * k * ACTION_DIM:4 * words].view(torch.int32).numpy()[:] = ids_np
        d_in = self._buf("in", 4 * words, False)
        d_in[:4 * words].copy_(h_in[:4 * words], non_blocking=True)
        nb = self._packed_bytes(k)
        d_out = self._buf("out", nb, False)
        h_out = self._buf("out", nb, True)
        if k:
            self._launch(d_in.data_ptr(), d_in.data_ptr() + 4 * k * ACTION_DIM, k, d_out, False)
        h_out[:nb].copy_(d_out[:nb], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self.host_turn[ids_np] += 1
        obs, rew, done, ctr, _ = self._unpack(h_out, k)
        return obs.numpy(), rew.numpy(), done.numpy().astype(bool), ctr.numpy()

    def noise(self, ids, events) -> torch.Tensor:
        """The noise the kernels draw for (env ids[j], event events[j]): fp32 [k, 237] = [21 step Gumbels | z (128) | 88 user Gumbels]."""
        ids_np = np.atleast_1d(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)).astype(np.int32)
        ev_np = np.atleast_1d(np.asarray(events.cpu() if isinstance(events, torch.Tensor) else events)).astype(np.int64)
        ids_np, ev_np = np.broadcast_arrays(ids_np, ev_np)
        k = ids_np.size
        out = torch.empty((k, NOISE_COLS), dtype=torch.float32, device=self.device)
        if k:
            d_ids = torch.from_numpy(np.ascontiguousarray(ids_np.reshape(-1))).to(self.device)
            d_ev = torch.from_numpy(np.ascontiguousarray(ev_np.reshape(-1).astype(np.uint32).view(np.int32))).to(self.device)
            abi.check(self._lib.cirs_vtb_noise(self._seed, d_ids.data_ptr(), d_ev.data_ptr(), k, out.data_ptr(), self._stream()),
                      "cirs_vtb_noise")
        return out

    def mmoe_forward(self, x) -> torch.Tensor:
        """UserModel_MMOE.forward on x [n, 118] (unclamped) through the step kernel's user-model code."""
        if not self.simulated:
            raise ValueError("the raw kind has no user model")
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).contiguous()
        y = torch.empty(x.shape[0], dtype=torch.float32, device=self.device)
        abi.check(self._lib.cirs_vtb_mmoe_forward(C.byref(self.cfg), C.byref(self._wst), x.data_ptr(), x.shape[0], y.data_ptr(),
                                                  self._stream()), "cirs_vtb_mmoe_forward")
        return y
