"""DeviceVtbRollout: whole VirtualTaobao PPO collects on the GPU (csrc/vtb_rollout.hip through cirs_vtb_rollout_collect).

The policy side of the per-step loop -- HostStateTracker (core/host_rl.py) as a K/V-cached decode and ActorProb over its Net trunk
with the Gaussian draw -- runs in vtb_policy_step_kernel, the env side in the DeviceVirtualTB's vtb_step_kernel; two launches per
vector step and no host synchronisation until the collect ends.  The parameters stay where the host update keeps them (plain torch
modules): before every collect they are packed into one flat fp32 buffer and sent up with one H2D copy.
"""
import ctypes as C
import operator

import numpy as np
import torch

from . import abi
from .vtb_host import ACTION_DIM, DROP_ATTN, DROP_FF, DROP_POS, DROP_RES1, DROP_RES2, USER_DIM
from .vtb_model import VtbModel, stream, u64

_BOUND = {"": 0, None: 0, "clip": 1, "tanh": 2}


def image_parts(model, policy):
    """The rollout's flat parameter image as (name, tensor, transposed, offset in floats) in order, and its total floats: the model's
    tensors without the critic's, a matrix stored transposed ([out][in] -> [in][out]) and a vector flat, plus the rollout's own pe (after
    the input slot's) and action box; every tensor 16-byte aligned."""
    parts = [(name, p, p.dim() == 2) for name, p in model.tracker_tensors() + model.policy_tensors() if not name.startswith("critic")]
    parts.insert(4, ("pe", model.tracker.pos_encoder.pe[:, 0, :], False))
    if policy.action_scaling:
        box = policy.action_space
        parts += [(k, torch.as_tensor(np.asarray(v, np.float32)), False) for k, v in (("act_low", box.low), ("act_high", box.high))]
    offs = np.concatenate([[0], np.cumsum([(p.numel() + 3) // 4 * 4 for _, p, _ in parts])])
    return [part + (int(o),) for part, o in zip(parts, offs)], int(offs[-1])


def fill_image(host, parts):
    for _, p, transposed, o in parts:
        src = p.detach().to(torch.float32)
        host[o:o + p.numel()] = (src.t() if transposed else src).reshape(-1)


def _weight_slots(w, nlayers, n_hidden):
    """name of an image part -> (setter, holder, key): where its pointer goes in cirs_vtb_policy_weights."""
    slots = {k: (setattr, w, k) for k in ("user_w", "user_b", "gate_w", "gate_b", "pe", "dec_w", "dec_b", "mu_w", "mu_b", "sigma_w", "sigma_b",
                                          "sigma_param", "act_low", "act_high")}
    slots.update({f"layer{l}.{k}": (setattr, w.layer[l], k) for l in range(nlayers) for k in abi.VTB_LAYER_FIELDS})
    slots.update({f"trunk{i}_{k}": (operator.setitem, getattr(w, f"trunk_{k}"), i) for i in range(n_hidden) for k in "wb"})
    return slots


class DeviceVtbRollout:
    """n_env = the DeviceVirtualTB's env count; `tracker` a HostStateTracker, `actor` an ActorProb over a Net trunk, `policy` the
    HostPPOPolicy that maps its actions."""

    def __init__(self, vtb, tracker, actor, policy, force_length=0, dropout_redraw=False):
        self.model = VtbModel(tracker, actor)
        self.dropout_redraw = bool(dropout_redraw)
        self.vtb, self.tracker, self.actor, self.policy = vtb, tracker, actor, policy
        self.device = vtb.device
        B, T = vtb.n_env, vtb.max_turn
        if policy.action_bound_method not in _BOUND:
            raise ValueError(f"unsupported action_bound_method {policy.action_bound_method!r}")
        m = self.model.model_cfg()
        self.cfg = abi.VtbRolloutCfg(n_env=B, max_turn=T, force_length=int(force_length), bound_method=_BOUND[policy.action_bound_method],
                                     action_scaling=int(bool(policy.action_scaling)), model=m)
        D, S, L, nlayers = m.dim_model, m.dim_state, m.max_len, m.nlayers
        # the flat parameter image: one pinned staging buffer, one device buffer, the kernel's pointers into it
        self._parts, total = image_parts(self.model, policy)
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._host = torch.zeros(total, dtype=torch.float32, pin_memory=True)
        self._w = abi.VtbPolicyWeights()
        slots = _weight_slots(self._w, nlayers, m.n_hidden)
        for name, _, _, o in self._parts:
            put, holder, key = slots[name]
            put(holder, key, self.flat.data_ptr() + 4 * o)
        # trajectory + scratch
        dev = self.device
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        self.traj = dict(state=torch.zeros((T + 1, B, S), **f32), act=torch.zeros((T, B, ACTION_DIM), **f32),
                         act_mapped=torch.zeros((T, B, ACTION_DIM), **f32), obs0=torch.zeros((B, USER_DIM + 3), **f64),
                         obs=torch.zeros((T, B, ACTION_DIM + 3), **f64), rew=torch.zeros((T, B), **f64),
                         done=torch.zeros((T, B), dtype=torch.uint8, device=dev), ctr=torch.zeros((T, B), **f64),
                         len=torch.zeros(B, dtype=torch.int32, device=dev),
                         kcache=torch.zeros((nlayers, B, L, D), **f32), vcache=torch.zeros((nlayers, B, L, D), **f32),
                         lists=torch.zeros((T + 1, B), dtype=torch.int32, device=dev), counts=torch.zeros(T + 1, dtype=torch.int32, device=dev),
                         act_buf=torch.zeros((B, ACTION_DIM), **f32), step_obs=torch.zeros((B, ACTION_DIM + 3), **f64),
                         step_rew=torch.zeros(B, **f64), step_ctr=torch.zeros(B, **f64),
                         step_done=torch.zeros(B, dtype=torch.uint8, device=dev))
        self._tr = abi.VtbTraj(**{k: self.traj[k].data_ptr() for k in abi.VTB_TRAJ_FIELDS})
        # exact redraw: the kept slots and the lower layers' output rows of the prefix pass
        self._redraw_ws = torch.zeros(L * B * D * nlayers, **f32) if self.dropout_redraw else None
        self._lib = abi.lib()

    def pack(self):
        """The current host parameters -> the device image (one H2D copy)."""
        fill_image(self._host, self._parts)
        self.flat.copy_(self._host, non_blocking=True)

    dropout_p = property(lambda self: self.model.dropout_p)

    def collect(self, seed, collect_id, dropout_seed=0, force_length=None, greedy=False):
        """One collect of every env; returns the episode lengths (numpy, the only synchronisation).
        greedy: act = mu, no Gaussian draw (cirs_vtb_rollout_collect_greedy: deterministic_eval in eval mode); seed / collect_id are unused."""
        if force_length is not None:
            self.cfg.force_length = int(force_length)
        self.cfg.model.dropout_p = self.dropout_p
        self.cfg.model.dropout_seed = u64(dropout_seed)
        self.cfg.env_seed = u64(self.vtb._seed)
        self.pack()
        args = (C.byref(self.cfg), C.byref(self._w), C.byref(self.vtb.cfg), C.byref(self.vtb._wst), C.byref(self.vtb._st), C.byref(self._tr))
        key = (u64(seed), int(collect_id) & 0xFFFFFFFF, stream(self.device))
        if greedy:
            abi.check(self._lib.cirs_vtb_rollout_collect_greedy(*args, abi.ptr(self._redraw_ws) if self.dropout_redraw else None, key[2]),
                      "cirs_vtb_rollout_collect_greedy")
        elif self.dropout_redraw:
            abi.check(self._lib.cirs_vtb_rollout_collect_redraw(*args, self._redraw_ws.data_ptr(), *key), "cirs_vtb_rollout_collect_redraw")
        else:
            abi.check(self._lib.cirs_vtb_rollout_collect(*args, *key), "cirs_vtb_rollout_collect")
        lens = self.traj["len"].cpu().numpy().astype(np.int64)
        self.vtb.host_turn[:] = lens          # the env's turns as the host tracks them (DeviceVirtualTB._check_turns)
        self.vtb._was_reset[:] = True
        return lens

    # ---- what the kernels draw -----------------------------------------------------------------------------------------------
    def noise(self, seed, collect_id, env_ids, ts, dims=ACTION_DIM) -> torch.Tensor:
        """z [n, dims] of (env_ids[j], ts[j]) for that collect key, bit for bit what the policy kernel draws."""
        ids = torch.as_tensor(np.asarray(env_ids, np.int32).reshape(-1), device=self.device)
        tt = torch.as_tensor(np.asarray(ts, np.int32).reshape(-1), device=self.device)
        out = torch.empty((ids.numel(), dims), dtype=torch.float32, device=self.device)
        abi.check(self._lib.cirs_vtb_rollout_noise(u64(seed), int(collect_id) & 0xFFFFFFFF, ids.data_ptr(), tt.data_ptr(), ids.numel(), dims,
                                                   out.data_ptr(), stream(self.device)), "cirs_vtb_rollout_noise")
        return out

    def masks(self, dropout_seed, n_pos, env0=0, n_env=None, p=None):
        """The scaled keep masks of positions 0..n_pos-1 in the layout vtb_host.states_from_slots takes (host fp32 tensors)."""
        lib, B = self._lib, self.vtb.n_env if n_env is None else n_env
        p = self.dropout_p if p is None else p
        mc = self.cfg.model
        D, H, d_hid = mc.dim_model, mc.nhead, mc.d_hid

        def one(layer, site, n_elem):
            out = torch.empty((B, n_pos, n_elem), dtype=torch.float32, device=self.device)
            abi.check(lib.cirs_vtb_rollout_masks(u64(dropout_seed), float(p), int(mc.drop_env_base) + env0, B, 0, n_pos, layer, site, n_elem,
                                                 out.data_ptr(), stream(self.device)), "cirs_vtb_rollout_masks")
            return out.cpu()

        m = {"pos": one(0, DROP_POS, D)}
        for l in range(mc.nlayers):
            m[(l, DROP_ATTN)] = one(l, DROP_ATTN, n_pos * H)
            m[(l, DROP_RES1)] = one(l, DROP_RES1, D)
            m[(l, DROP_FF)] = one(l, DROP_FF, d_hid)
            m[(l, DROP_RES2)] = one(l, DROP_RES2, D)
        return m

    def call_masks(self, dropout_seed, c):
        """Exact redraw: the masks of call c (positions 0..c) of every env, those of dropout env ids drop_env_base + c * n_env + e."""
        return self.masks(dropout_seed, c + 1, env0=c * self.vtb.n_env)
