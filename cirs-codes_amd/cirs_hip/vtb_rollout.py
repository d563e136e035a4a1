"""DeviceVtbRollout: whole VirtualTaobao PPO collects on the GPU (csrc/vtb_rollout.hip through cirs_vtb_rollout_collect).

The policy side of the per-step loop -- HostStateTracker (core/host_rl.py) as a K/V-cached decode and ActorProb over its Net trunk
with the Gaussian draw -- runs in vtb_policy_step_kernel, the env side in the DeviceVirtualTB's vtb_step_kernel; two launches per
vector step and no host synchronisation until the collect ends.  The parameters stay where the host update keeps them (plain torch
modules): before every collect they are packed into one flat fp32 buffer and sent up with one H2D copy.
"""
import ctypes as C

import numpy as np
import torch
from torch import nn

from . import abi
from .vtb_host import ACTION_DIM, DROP_ATTN, DROP_FF, DROP_POS, DROP_RES1, DROP_RES2, USER_DIM

_BOUND = {"": 0, None: 0, "clip": 1, "tanh": 2}


def _linears(mlp, what):
    """The nn.Linear layers of a tianshou MLP; every hidden layer must be followed by a ReLU."""
    mods = list(mlp.model)
    lin = [m for m in mods if isinstance(m, nn.Linear)]
    for i, m in enumerate(mods):
        if isinstance(m, nn.Linear):
            continue
        if not isinstance(m, nn.ReLU):
            raise ValueError(f"{what}: only Linear + ReLU layers are supported, found {type(m).__name__}")
    return lin


class DeviceVtbRollout:
    """n_env = the DeviceVirtualTB's env count; `tracker` a HostStateTracker, `actor` an ActorProb over a Net trunk, `policy` the
    HostPPOPolicy that maps its actions."""

    def __init__(self, vtb, tracker, actor, policy, force_length=0):
        from tianshou.utils.net.continuous import ActorProb
        if not isinstance(actor, ActorProb):
            raise TypeError("the device VirtualTaobao rollout needs a continuous ActorProb actor (Independent(Normal) policy)")
        self.vtb, self.tracker, self.actor, self.policy = vtb, tracker, actor, policy
        self.device = vtb.device
        B, T = vtb.n_env, vtb.max_turn
        layers = tracker.transformer_encoder.layers
        D, S = int(tracker.dim_model), int(tracker.dim_state)
        nhead = int(layers[0].self_attn.num_heads)
        d_hid = int(layers[0].linear1.out_features)
        trunk = _linears(actor.preprocess.model, "actor trunk")
        mu = _linears(actor.mu, "actor mu head")
        if len(mu) != 1:
            raise ValueError("ActorProb heads with hidden layers are not supported by the device rollout (hidden_sizes=() only)")
        sig = _linears(actor.sigma, "actor sigma head") if actor._c_sigma else []
        if actor._c_sigma and len(sig) != 1:
            raise ValueError("a conditioned sigma head with hidden layers is not supported by the device rollout")
        if int(actor.output_dim) != ACTION_DIM:
            raise ValueError(f"the actor must output the {ACTION_DIM} VirtualTaobao action features")
        if not 1 <= len(trunk) <= 3 or trunk[0].in_features != S:
            raise ValueError("the actor trunk must be a Net of 1..3 hidden layers over the tracker state")
        if policy.action_bound_method not in _BOUND:
            raise ValueError(f"unsupported action_bound_method {policy.action_bound_method!r}")
        hidden = [int(m.out_features) for m in trunk] + [0] * (abi.VTB_RO_MAX_HIDDEN - len(trunk))
        self.cfg = abi.VtbRolloutCfg(n_env=B, max_turn=T, force_length=int(force_length), dim_model=D, nhead=nhead, d_hid=d_hid,
                                     nlayers=len(layers), dim_state=S, max_len=int(tracker.MAX_TURN), n_hidden=len(trunk),
                                     hidden=(C.c_int32 * abi.VTB_RO_MAX_HIDDEN)(*hidden), unbounded=int(bool(actor._unbounded)),
                                     conditioned_sigma=int(bool(actor._c_sigma)), bound_method=_BOUND[policy.action_bound_method],
                                     action_scaling=int(bool(policy.action_scaling)), max_action=float(actor._max))
        # the flat parameter image: (name, host fp32 tensor of the kernel's layout) in a fixed order
        t_ = lambda w: w.detach().to(torch.float32).t()      # noqa: E731  [out, in] -> [in, out]
        v_ = lambda w: w.detach().to(torch.float32).reshape(-1)   # noqa: E731
        parts = [("user_w", lambda: t_(tracker.ffn_user.weight)), ("user_b", lambda: v_(tracker.ffn_user.bias)),
                 ("gate_w", lambda: t_(tracker.fnn_gate.weight)), ("gate_b", lambda: v_(tracker.fnn_gate.bias)),
                 ("pe", lambda: v_(tracker.pos_encoder.pe[:, 0, :]))]
        for l, ly in enumerate(layers):
            parts += [((l, "in_w"), lambda ly=ly: t_(ly.self_attn.in_proj_weight)), ((l, "in_b"), lambda ly=ly: v_(ly.self_attn.in_proj_bias)),
                      ((l, "out_w"), lambda ly=ly: t_(ly.self_attn.out_proj.weight)), ((l, "out_b"), lambda ly=ly: v_(ly.self_attn.out_proj.bias)),
                      ((l, "lin1_w"), lambda ly=ly: t_(ly.linear1.weight)), ((l, "lin1_b"), lambda ly=ly: v_(ly.linear1.bias)),
                      ((l, "lin2_w"), lambda ly=ly: t_(ly.linear2.weight)), ((l, "lin2_b"), lambda ly=ly: v_(ly.linear2.bias)),
                      ((l, "norm1_w"), lambda ly=ly: v_(ly.norm1.weight)), ((l, "norm1_b"), lambda ly=ly: v_(ly.norm1.bias)),
                      ((l, "norm2_w"), lambda ly=ly: v_(ly.norm2.weight)), ((l, "norm2_b"), lambda ly=ly: v_(ly.norm2.bias))]
        parts += [("dec_w", lambda: t_(tracker.decoder.weight)), ("dec_b", lambda: v_(tracker.decoder.bias))]
        for i, m in enumerate(trunk):
            parts += [(("trunk_w", i), lambda m=m: t_(m.weight)), (("trunk_b", i), lambda m=m: v_(m.bias))]
        parts += [("mu_w", lambda: t_(mu[0].weight)), ("mu_b", lambda: v_(mu[0].bias))]
        if actor._c_sigma:
            parts += [("sigma_w", lambda: t_(sig[0].weight)), ("sigma_b", lambda: v_(sig[0].bias))]
        else:
            parts += [("sigma_param", lambda: v_(actor.sigma_param))]
        if policy.action_scaling:
            box = policy.action_space
            low, high = torch.as_tensor(np.asarray(box.low, np.float32)), torch.as_tensor(np.asarray(box.high, np.float32))
            parts += [("act_low", lambda: low.reshape(-1)), ("act_high", lambda: high.reshape(-1))]
        self._parts = parts
        sizes = [int(f().numel()) for _, f in parts]
        offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in sizes])])      # 16-byte aligned tensors
        self.flat = torch.zeros(int(offs[-1]), dtype=torch.float32, device=self.device)
        self._host = torch.zeros(int(offs[-1]), dtype=torch.float32, pin_memory=True)
        self._slices = [(int(o), n) for o, n in zip(offs[:-1], sizes)]
        w = abi.VtbPolicyWeights()
        base, fsz = self.flat.data_ptr(), 4
        for (name, _), (o, _n) in zip(parts, self._slices):
            p = base + fsz * o
            if isinstance(name, tuple) and isinstance(name[0], int):
                setattr(w.layer[name[0]], name[1], p)
            elif isinstance(name, tuple):
                getattr(w, name[0])[name[1]] = p
            else:
                setattr(w, name, p)
        self._w = w
        # trajectory + scratch
        dev = self.device
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        L = int(tracker.MAX_TURN)
        self.traj = dict(state=torch.zeros((T + 1, B, S), **f32), act=torch.zeros((T, B, ACTION_DIM), **f32),
                         act_mapped=torch.zeros((T, B, ACTION_DIM), **f32), obs0=torch.zeros((B, USER_DIM + 3), **f64),
                         obs=torch.zeros((T, B, ACTION_DIM + 3), **f64), rew=torch.zeros((T, B), **f64),
                         done=torch.zeros((T, B), dtype=torch.uint8, device=dev), ctr=torch.zeros((T, B), **f64),
                         len=torch.zeros(B, dtype=torch.int32, device=dev),
                         kcache=torch.zeros((len(layers), B, L, D), **f32), vcache=torch.zeros((len(layers), B, L, D), **f32),
                         lists=torch.zeros((T + 1, B), dtype=torch.int32, device=dev), counts=torch.zeros(T + 1, dtype=torch.int32, device=dev),
                         act_buf=torch.zeros((B, ACTION_DIM), **f32), step_obs=torch.zeros((B, ACTION_DIM + 3), **f64),
                         step_rew=torch.zeros(B, **f64), step_ctr=torch.zeros(B, **f64),
                         step_done=torch.zeros(B, dtype=torch.uint8, device=dev))
        self._tr = abi.VtbTraj(**{k: self.traj[k].data_ptr() for k in abi.VTB_TRAJ_FIELDS})
        self._lib = abi.lib()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def pack(self):
        """The current host parameters -> the device image (one H2D copy)."""
        for (_, f), (o, n) in zip(self._parts, self._slices):
            self._host[o:o + n] = f().reshape(-1)
        self.flat.copy_(self._host, non_blocking=True)

    @property
    def dropout_p(self):
        """nn.Dropout is live while the tracker is in training mode (the reference never switches it off)."""
        return float(self.tracker.pos_encoder.dropout.p) if self.tracker.training else 0.0

    def collect(self, seed, collect_id, dropout_seed=0, force_length=None):
        """One collect of every env; returns the episode lengths (numpy, the only synchronisation)."""
        if force_length is not None:
            self.cfg.force_length = int(force_length)
        self.cfg.dropout_p = self.dropout_p
        self.cfg.dropout_seed = int(dropout_seed) & 0xFFFFFFFFFFFFFFFF
        self.cfg.env_seed = int(self.vtb._seed) & 0xFFFFFFFFFFFFFFFF
        self.pack()
        abi.check(self._lib.cirs_vtb_rollout_collect(C.byref(self.cfg), C.byref(self._w), C.byref(self.vtb.cfg), C.byref(self.vtb._wst),
                                                     C.byref(self.vtb._st), C.byref(self._tr), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                     int(collect_id) & 0xFFFFFFFF, self._stream()), "cirs_vtb_rollout_collect")
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
        abi.check(self._lib.cirs_vtb_rollout_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(collect_id) & 0xFFFFFFFF, ids.data_ptr(), tt.data_ptr(),
                                                   ids.numel(), dims, out.data_ptr(), self._stream()), "cirs_vtb_rollout_noise")
        return out

    def masks(self, dropout_seed, n_pos, env0=0, n_env=None, p=None):
        """The scaled keep masks of positions 0..n_pos-1 in the layout vtb_host.states_from_slots takes (host fp32 tensors)."""
        lib, B = self._lib, self.vtb.n_env if n_env is None else n_env
        p = self.dropout_p if p is None else p
        D, H, d_hid = self.cfg.dim_model, self.cfg.nhead, self.cfg.d_hid

        def one(layer, site, n_elem):
            out = torch.empty((B, n_pos, n_elem), dtype=torch.float32, device=self.device)
            abi.check(lib.cirs_vtb_rollout_masks(int(dropout_seed) & 0xFFFFFFFFFFFFFFFF, float(p), int(self.cfg.drop_env_base) + env0, B, 0, n_pos,
                                                 layer, site, n_elem, out.data_ptr(), self._stream()), "cirs_vtb_rollout_masks")
            return out.cpu()

        m = {"pos": one(0, DROP_POS, D)}
        for l in range(self.cfg.nlayers):
            m[(l, DROP_ATTN)] = one(l, DROP_ATTN, n_pos * H)
            m[(l, DROP_RES1)] = one(l, DROP_RES1, D)
            m[(l, DROP_FF)] = one(l, DROP_FF, d_hid)
            m[(l, DROP_RES2)] = one(l, DROP_RES2, D)
        return m
