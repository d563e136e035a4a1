"""Device training of the VirtualTaobao MMoE user model (csrc/mmoe_train.hip: cirs_mmoe_train_step / cirs_mmoe_train_epoch) and the
exposure effect of a VirtualTaobao log (cirs_vtb_exposure_history).

Host-side counterpart of UserModel_MMOE.fit_data's inner loop (reference core/user_model.py:150-170): parameters, gradients and the
Adam moments live in ONE flat fp32 device buffer each; named views follow the reference's state_dict."""
import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import abi
from .flat_train import FlatTrainer
from .mmoe_host import ACTION_COLS, D_IN, USER_COLS, mlp_shape_of, mlp_shapes, shapes

class _FlatTrainer(FlatTrainer):
    """What both trainers share on top of the flat buffers: the named slots (some stored transposed) and the calls of the library's
    _step / _epoch entries.  A subclass's __init__ reads its shape off the state_dict and
    calls _setup; it names its four ABI functions and supplies _cols(*columns) -> the validated, contiguous data columns (x first)."""
    _param_count = _workspace_bytes = _step_fn = _epoch_fn = None   # names of the ABI functions

    def _setup(self, cfg, sd, shapes, order, device):
        """cfg: the ABI's cfg struct; shapes: [(state_dict name, shape)] in state_dict order; order: [(name, stored transposed)] in
        buffer order."""
        total = getattr(abi.lib(), self._param_count)(C.byref(cfg))
        if total <= 0:
            msg = abi.lib().cirs_last_error()
            raise ValueError(msg.decode() if msg else "unsupported MMoE shape")
        self._shapes = shapes
        want = dict(shapes)
        if set(sd) != set(want):
            raise ValueError(f"unexpected parameters for the VirtualTaobao MMoE: {sorted(set(sd) ^ set(want))}")
        self._alloc(cfg, total, device)
        self._slots = {}
        off = 0
        for name, transposed in order:
            shape = want[name]
            n = int(np.prod(shape))
            self._slots[name] = (off, n, shape, transposed)
            src = sd[name].to(self.device, torch.float32).reshape(shape)
            self.flat[off:off + n].copy_((src.t() if transposed else src).reshape(-1))
            off += n
        assert off == total and set(self._slots) == set(want)
        self.loss = torch.zeros(2, dtype=torch.float32, device=self.device)

    def _named(self, flat):
        out = {}
        for name, _ in self._shapes:
            off, n, shape, transposed = self._slots[name]
            v = flat[off:off + n]
            out[name] = v.view(shape[1], shape[0]).t().contiguous() if transposed else v.view(shape).clone()
        return out

    def state_dict(self):
        """The parameters under the reference's state_dict names and shapes (copies)."""
        return self._named(self.flat)

    def moments(self):
        return self._named(self.adam_m), self._named(self.adam_v)

    def gradients(self):
        """The gradients of loss + reg of the last step, under the same names."""
        return self._named(self.grads)

    def _step(self, cols):
        n = cols[0].shape[0]
        if n == 0:
            raise ValueError("empty batch")
        ws = self._workspace(n)
        abi.check(getattr(self._lib, self._step_fn)(*self._buffers(), *(c.data_ptr() for c in cols), n, self.loss.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), self._stream()), self._step_fn)
        self.step_count += 1
        return self.loss

    def _epoch(self, cols, order, batch_size):
        order = torch.as_tensor(order).to(self.device, torch.int64).contiguous()
        n, bs = int(order.numel()), int(batch_size)
        if n == 0 or bs <= 0 or cols[0].shape[0] == 0:
            raise ValueError("empty data set, index array or batch size")
        steps = (n + bs - 1) // bs
        losses = torch.zeros((steps, 2), dtype=torch.float32, device=self.device)
        ws = self._workspace(min(bs, n))
        abi.check(getattr(self._lib, self._epoch_fn)(*self._buffers(), *(c.data_ptr() for c in cols), cols[0].shape[0], order.data_ptr(), n, bs,
                                                     losses.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._epoch_fn)
        self.step_count += steps
        return losses


def _tensors(state_dict):
    return {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v) for k, v in state_dict.items()}


class MMoETrainer(_FlatTrainer):
    _param_count, _workspace_bytes = "cirs_mmoe_train_param_count", "cirs_mmoe_train_workspace_bytes"
    _step_fn, _epoch_fn = "cirs_mmoe_train_step", "cirs_mmoe_train_epoch"
    # (state_dict name, stored transposed) in buffer order -- must match layout() in csrc/mmoe_train.hip
    _ORDER = [("dnn.linears.1.weight", False), ("mmoe_layer.expert_network.weight", False), ("mmoe_layer.gating_networks.0.weight", False),
              ("dnn.linears.0.weight", True), ("dnn.linears.0.bias", False), ("dnn.linears.1.bias", False),
              ("mmoe_layer.expert_network.bias", False), ("tower_network.0.weight", False), ("linear_model.weight", False),
              ("linear_model_task.0.weight", False), ("out.0.bias", False)]

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, l2_linear=1e-5, l2_all=1e-2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device="cuda"):
        sd = _tensors(state_dict)
        w1, w2 = sd["dnn.linears.0.weight"], sd["dnn.linears.1.weight"]
        if len([k for k in sd if k.startswith("dnn.linears.") and k.endswith(".weight")]) != 2:
            raise ValueError("the device step trains UserModel_MMOE with two hidden layers")
        h1, h2 = int(w1.shape[0]), int(w2.shape[0])
        ex = sd["mmoe_layer.expert_network.weight"].shape[0]
        ng = sd["mmoe_layer.gating_networks.0.weight"].shape[0]
        n_tasks = len([k for k in sd if k.startswith("tower_network.")])
        cfg = abi.MmoeTrainCfg(d_in=int(w1.shape[1]), h1=h1, h2=h2, n_experts=int(ng), expert_dim=int(ex // max(ng, 1)), n_tasks=n_tasks,
                               task_dim=int(sd["tower_network.0.weight"].shape[0]), l2_linear=float(l2_linear), l2_all=float(l2_all),
                               lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps))
        self._setup(cfg, sd, shapes(h1, h2), self._ORDER, device)

    def _cols(self, x, y, exposure):
        x = torch.as_tensor(x).to(self.device, torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != D_IN:
            raise ValueError(f"x must be [n, {D_IN}]")
        y = torch.as_tensor(y).to(self.device, torch.float32).reshape(-1).contiguous()
        e = torch.as_tensor(exposure).to(self.device, torch.float32).reshape(-1).contiguous()
        if y.numel() != x.shape[0] or e.numel() != x.shape[0]:
            raise ValueError("x, y and exposure must have one row per sample")
        return x, y, e

    def step(self, x, y, exposure):
        """One optimiser step on the batch x [n, 118], y [n] or [n, 1], exposure [n] or [n, 1] -> the device vector {loss, reg}."""
        return self._step(self._cols(x, y, exposure))

    def epoch(self, x, y, exposure, order, batch_size):
        """All steps of one pass over the device-resident data set in the row order `order` (int64), the last batch short as in DataLoader
        -> device tensor [steps, 2] of per-step {loss, reg}.  Nothing is synchronised: the launches are queued and the call returns."""
        return self._epoch(self._cols(x, y, exposure), order, batch_size)


class MlpTrainer(_FlatTrainer):
    """The same surface for the two-task build of the static baselines (csrc/mlp_train.hip: cirs_mlp_train_step / _epoch; reference
    MLP-taobao.py, MLP-epsilonGreedy-taobao.py): x [n, 91] static states, y [n, 28] = [27 item features | click].  The shape is read
    off the state_dict: whatever cirs_hip.vtb_static evaluates can be trained."""
    _param_count, _workspace_bytes = "cirs_mlp_train_param_count", "cirs_mlp_train_workspace_bytes"
    _step_fn, _epoch_fn = "cirs_mlp_train_step", "cirs_mlp_train_epoch"

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, l2_linear=1e-5, l2_all=1e-2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device="cuda"):
        sd = _tensors(state_dict)
        hidden, experts, expert_dim = mlp_shape_of(sd)
        self.hidden, self.experts, self.expert_dim = tuple(hidden), experts, expert_dim
        hid = list(hidden[:abi.VTB_STATIC_MAX_DNN]) + [0] * max(0, abi.VTB_STATIC_MAX_DNN - len(hidden))
        shape = abi.VtbMmoeShape(d_in=USER_COLS, n_dnn=len(hidden), hidden=(C.c_int32 * abi.VTB_STATIC_MAX_DNN)(*hid), experts=experts,
                                 expert_dim=expert_dim, n_tasks=2, task_dim=(C.c_int32 * 2)(ACTION_COLS, 1))
        cfg = abi.MlpTrainCfg(shape=shape, l2_linear=float(l2_linear), l2_all=float(l2_all), lr=float(lr), beta1=float(betas[0]),
                              beta2=float(betas[1]), eps=float(eps))
        L = len(hidden)
        # (state_dict name, stored transposed) in buffer order -- must match layout() in csrc/mlp_train.hip
        order = [(f"dnn.linears.{l}.weight", False) for l in range(1, L)] + \
                [("mmoe_layer.expert_network.weight", False), ("mmoe_layer.gating_networks.0.weight", False),
                 ("mmoe_layer.gating_networks.1.weight", False), ("dnn.linears.0.weight", True)] + \
                [(f"dnn.linears.{l}.bias", False) for l in range(L)] + \
                [("mmoe_layer.expert_network.bias", False), ("tower_network.0.weight", False), ("tower_network.1.weight", False),
                 ("out.0.bias", False), ("out.1.bias", False), ("linear_model.weight", False), ("linear_model_task.1.weight", False)]
        self._setup(cfg, sd, mlp_shapes(hidden, experts, expert_dim), order, device)

    def _cols(self, x, y):
        x = torch.as_tensor(x).to(self.device, torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != USER_COLS:
            raise ValueError(f"x must be [n, {USER_COLS}]")
        y = torch.as_tensor(y).to(self.device, torch.float32).contiguous()
        if y.dim() != 2 or tuple(y.shape) != (x.shape[0], ACTION_COLS + 1):
            raise ValueError(f"y must be [n, {ACTION_COLS + 1}] (27 item features | click) with one row per sample")
        return x, y

    def step(self, x, y):
        """One optimiser step on the batch x [n, 91], y [n, 28] -> the device vector {loss, reg}."""
        return self._step(self._cols(x, y))

    def epoch(self, x, y, order, batch_size):
        """All steps of one pass over the device-resident data set in the row order `order` (int64), the last batch short as in DataLoader
        -> device tensor [steps, 2] of per-step {loss, reg}.  Nothing is synchronised: the launches are queued and the call returns."""
        return self._epoch(self._cols(x, y), order, batch_size)


def vtb_exposure_history(timestamp, action, tau, device="cuda"):
    """compute_exposure_effect_virtualTaobao on the device: timestamp [n] (host; a row with 1 opens a session), action [n, 27]
    -> exposure float64 [n, 1] (device tensor)."""
    ts = np.ascontiguousarray(np.asarray(timestamp).reshape(-1).astype(np.int32))
    a = torch.as_tensor(np.asarray(action, np.float64) if not isinstance(action, torch.Tensor) else action).to(device, torch.float64).contiguous()
    n = len(ts)
    if a.shape != (n, ACTION_COLS):
        raise ValueError(f"action must be [n, {ACTION_COLS}] with one row per timestamp")
    out = torch.zeros((n, 1), dtype=torch.float64, device=device)
    start = torch.empty(max(n, 1), dtype=torch.int64, device=device)
    abi.check(abi.lib().cirs_vtb_exposure_history(ts.ctypes.data, a.data_ptr(), n, float(tau), start.data_ptr(), out.data_ptr(),
                                                  torch.cuda.current_stream(torch.device(device)).cuda_stream), "cirs_vtb_exposure_history")
    return out
