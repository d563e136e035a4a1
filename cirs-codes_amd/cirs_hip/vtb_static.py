"""Evaluation of the VirtualTaobao static baselines on the device: evaluation.test_taobao with every trajectory played in lock step by
ONE launch (csrc/vtb_static.hip through cirs_vtb_static_eval).

Host-side counterpart of the reference's evaluation.py:238-282, which MLP-taobao.py and MLP-epsilonGreedy-taobao.py call at every
epoch end: a two-task UserModel_MMOE (static state 91 -> 27 item features + 1 click prediction) plays `n_traj` trajectories against a
VirtualTB in static-state mode.  The weights go up once; `run` is one launch, one metrics reduction and one read-back of
(metrics, lengths).  The noise is counter-based (Philox, key = seed) like DeviceVirtualTB's: `noise(ids, turns)` returns exactly what
the kernel drew, so the CPU mirror fed with it and with the recorded actions reproduces a device run.
"""
import ctypes as C

import numpy as np
import torch

from . import abi
from .virtualtb import ACTION_DIM, GROUPS, _t, _v, env_weights

STATE_DIM, NOISE_COLS = abi.VTB_STATIC_STATE_DIM, abi.VTB_STATIC_NOISE_COLS
MAX_HIDDEN, MAX_EXPERT_OUT = 256, 64


def policy_shape(model) -> dict:
    """The fields of cirs_vtb_mmoe_shape read off a UserModel_MMOE; ValueError for a model the kernel does not run.  Pure host code."""
    def no(why):
        return ValueError("the device evaluation runs the static baselines' model only (all-dense UserModel_MMOE: 91 inputs, 1 to 3 hidden "
                          f"layers of at most {MAX_HIDDEN}, num_experts * expert_dim <= {MAX_EXPERT_OUT}, the two regression tasks "
                          f"feat_item (27) and y (1)): {why}")
    try:
        dnn = list(model.dnn.linears)
        mm, towers, outs, lins = model.mmoe_layer, list(model.tower_network), list(model.out), list(model.linear_model_task)
        names = [f.name for f in model.y_columns]
        dims = [int(model.task_logit_dim[n]) for n in names]
    except (AttributeError, KeyError, TypeError) as exc:
        raise no(f"not a UserModel_MMOE ({exc})") from None
    if not dnn or int(dnn[0].in_features) != STATE_DIM:
        raise no(f"{int(dnn[0].in_features) if dnn else 0} inputs")
    hidden = [int(m.out_features) for m in dnn]
    if not 1 <= len(hidden) <= abi.VTB_STATIC_MAX_DNN:
        raise no(f"{len(hidden)} hidden layers")
    if max(hidden) > MAX_HIDDEN:
        raise no(f"hidden widths {tuple(hidden)}")
    E, D = int(mm.num_experts), int(mm.out_dim)
    if E < 1 or D < 1 or E * D > MAX_EXPERT_OUT:
        raise no(f"{E} experts of dim {D}")
    if names != ["feat_item", "y"] or dims != [ACTION_DIM, 1] or len(towers) != 2 or len(outs) != 2 or len(mm.gating_networks) != 2 or \
            [int(t.out_features) for t in towers] != dims:
        raise no(f"tasks {list(zip(names, dims))}")
    if len(lins) != 2 or lins[0] is not None or lins[1] is None:
        raise no("linear_model_task must exist on the dim-1 task only")
    return dict(d_in=STATE_DIM, n_dnn=len(hidden), hidden=hidden, experts=E, expert_dim=D, n_tasks=2, task_dim=dims)


def shape_struct(shape: dict) -> abi.VtbMmoeShape:
    hid = list(shape["hidden"]) + [0] * (abi.VTB_STATIC_MAX_DNN - len(shape["hidden"]))
    return abi.VtbMmoeShape(d_in=shape["d_in"], n_dnn=shape["n_dnn"], hidden=(C.c_int32 * abi.VTB_STATIC_MAX_DNN)(*hid), experts=shape["experts"],
                            expert_dim=shape["expert_dim"], n_tasks=shape["n_tasks"], task_dim=(C.c_int32 * 2)(*shape["task_dim"]))


def check_static_env(vtb_env):
    if not getattr(vtb_env, "static", False):
        raise ValueError("test_taobao plays the static baselines: the env must be in static-state mode (env.set_state_mode(True)); the "
                         "policy's 91 inputs are the static state [user | last clicks, last second draw | turn]")


class DeviceVtbStaticEval:
    """`n_traj` trajectories of `model` against `vtb_env` (a host VirtualTB in static-state mode), all inside one kernel launch."""

    def __init__(self, vtb_env, model, n_traj: int, *, seed=0, device="cuda"):
        shape = policy_shape(model)          # every refusal happens on the host, before anything touches the GPU
        check_static_env(vtb_env)
        self.n_traj, self.max_turn = int(n_traj), int(vtb_env.max_turn)
        if self.n_traj <= 0:
            raise ValueError("n_traj must be positive")
        self._cfg = dict(n_traj=self.n_traj, max_turn=self.max_turn, num_leave_compute=int(vtb_env.num_leave_compute),
                         leave_threshold=float(vtb_env.leave_threshold), policy=shape_struct(shape))
        self.device = dev = torch.device(device)
        self._seed = int(seed) & ((1 << 64) - 1)
        self._ew = env_weights(vtb_env, dev)
        self._ewst = abi.VtbWeights(**{k: t.data_ptr() for k, t in self._ew.items()})
        m = model
        nd = shape["n_dnn"]
        self._pw = dict(dnn_w=[_t(l.weight, dev) for l in m.dnn.linears], dnn_b=[_v(l.bias, dev) for l in m.dnn.linears],
                        expert_w=_t(m.mmoe_layer.expert_network.weight, dev), expert_b=_v(m.mmoe_layer.expert_network.bias, dev),
                        gate_w=[_t(g.weight, dev) for g in m.mmoe_layer.gating_networks], tower_w=[_t(t.weight, dev) for t in m.tower_network],
                        lin_w=_v(m.linear_model_task[1].weight, dev), bias=[_v(o.bias, dev) for o in m.out])
        pad = [None] * (abi.VTB_STATIC_MAX_DNN - nd)
        pw = self._pw
        self._pwst = abi.VtbMmoeWeights(
            dnn_w=(C.c_void_p * abi.VTB_STATIC_MAX_DNN)(*([t.data_ptr() for t in pw["dnn_w"]] + pad)),
            dnn_b=(C.c_void_p * abi.VTB_STATIC_MAX_DNN)(*([t.data_ptr() for t in pw["dnn_b"]] + pad)),
            expert_w=pw["expert_w"].data_ptr(), expert_b=pw["expert_b"].data_ptr(), gate_w=(C.c_void_p * 2)(*[t.data_ptr() for t in pw["gate_w"]]),
            tower_w=(C.c_void_p * 2)(*[t.data_ptr() for t in pw["tower_w"]]), lin_w=pw["lin_w"].data_ptr(),
            bias=(C.c_void_p * 2)(*[t.data_ptr() for t in pw["bias"]]))
        self._lib = abi.lib()
        self._bufs = None
        self.last_epsilon = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def seed(self, s=0):
        self._seed = int(s) & ((1 << 64) - 1)

    def _alloc(self):
        n, T, dev = self.n_traj, self.max_turn, self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731  (turns past a trajectory's end stay 0)
        return dict(user=z((n, GROUPS), torch.int32), state=z((n, T, STATE_DIM), torch.float32), action=z((n, T, ACTION_DIM), torch.float32),
                    reward_pred=z((n, T), torch.float32), reward=z((n, T), torch.int32), done=z((n, T), torch.uint8),
                    explore=z((n, T), torch.uint8), metrics=z(abi.vtb_static_metrics_bytes(n) + 8, torch.uint8))

    def run(self, epsilon=0.0) -> dict:
        """One evaluation -> {"ctr", "click_loss", "len_tra", "R_tra"} (evaluation.py:273-280)."""
        epsilon = float(epsilon)
        if not 0.0 <= epsilon <= 1.0:
            raise ValueError("epsilon must lie in [0, 1]")
        cfg = abi.VtbStaticCfg(epsilon=epsilon, **self._cfg)
        nbytes = int(self._lib.cirs_vtb_static_workspace_bytes(C.byref(cfg)))
        if nbytes < 0:
            abi.check(-1, "cirs_vtb_static_workspace_bytes")
        b = self._alloc()
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        out = abi.VtbStaticOut(**{k: t.data_ptr() for k, t in b.items()})
        abi.check(self._lib.cirs_vtb_static_eval(C.byref(cfg), C.byref(self._ewst), C.byref(self._pwst), self._seed, C.byref(out), ws.data_ptr(),
                                                 ws.numel() * 8, self._stream()), "cirs_vtb_static_eval")
        nb = abi.vtb_static_metrics_bytes(self.n_traj)
        host = b["metrics"][:nb].cpu().numpy()                  # the one read-back: metrics and lengths together
        m = host[:32].view(np.float64)
        self.totals = tuple(int(v) for v in host[32:48].view(np.int64))     # (clicks, turns)
        self.lengths = host[48:nb].view(np.int32).copy()
        self._bufs, self.last_epsilon = b, epsilon
        return {"ctr": float(m[0]), "click_loss": float(m[1]), "len_tra": float(m[2]), "R_tra": float(m[3])}

    def trajectory(self) -> dict:
        """The last run, per (trajectory, turn): state [n,T,91], action [n,T,27], reward_pred [n,T], reward [n,T] (clicks), done,
        explore [n,T] bool; per trajectory: len [n], user [n,11] (one-hot positions).  Turns >= len are zero."""
        if self._bufs is None:
            raise ValueError("run() first")
        b = {k: v.cpu().numpy() for k, v in self._bufs.items() if k != "metrics"}
        b["done"], b["explore"] = b["done"].astype(bool), b["explore"].astype(bool)
        b["len"] = self.lengths.copy()
        return b

    def noise(self, ids, turns) -> torch.Tensor:
        """What the kernel draws for (trajectory ids[j], turn turns[j]): fp32 [k, 265] = [21 step Gumbels | z (128) | 88 user Gumbels |
        epsilon uniform | 27 exploration uniforms]."""
        ids_np, t_np = np.broadcast_arrays(np.atleast_1d(np.asarray(ids)).astype(np.int32), np.atleast_1d(np.asarray(turns)).astype(np.int32))
        k = ids_np.size
        if k and (ids_np.min() < 0 or t_np.min() < 0):
            raise ValueError("trajectory ids and turns must be >= 0")
        out = torch.empty((k, NOISE_COLS), dtype=torch.float32, device=self.device)
        if k:
            d_ids = torch.from_numpy(np.ascontiguousarray(ids_np.reshape(-1))).to(self.device)
            d_t = torch.from_numpy(np.ascontiguousarray(t_np.reshape(-1))).to(self.device)
            abi.check(self._lib.cirs_vtb_static_noise(self._seed, d_ids.data_ptr(), d_t.data_ptr(), k, out.data_ptr(), self._stream()),
                      "cirs_vtb_static_noise")
        return out
