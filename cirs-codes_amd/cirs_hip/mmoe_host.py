"""Host restatements for the VirtualTaobao user-model training (csrc/mmoe_train.hip); imports without libcirs_hip.so.

exposure_virtualtaobao   compute_exposure_effect_virtualTaobao (reference CIRS-UserModel-taobao.py:52-70) in numpy float64.
torch_train              the optimiser steps of UserModel_MMOE.fit_data (reference core/user_model.py:150-170) restated in plain torch
                         (autograd + torch.optim.Adam) over a state_dict under the reference's names: loss_taobao, the regulariser
                         over linear_model (l2_linear) and over EVERY parameter (l2_all).  The comparison object of the device step, in
                         tests and in tools/probe_mmoe_train.py.
mlp_torch_train          the same for the two-task build of the static baselines (reference MLP-taobao.py: 91 static-state inputs ->
                         feat_item (27) and y (1), its own loss_taobao, MLP-taobao.py:137-155), for run-time shapes: the comparison
                         object of csrc/mlp_train.hip, in tests and in tools/probe_mlp_train.py.
loss_and_grad            the loss columns {loss, reg} and the gradient of loss + reg of ONE batch by autograd over the same forward, loss
mlp_loss_and_grad        and regulariser, in the dtype asked for: the float64 reference of a device step's gradient buffer.
hidden_preactivations    the inputs of every hidden layer's relu for a batch (a unit within rounding of zero may take the other side
                         of the kink in another precision).
"""
import numpy as np
import torch

D_IN, N_EXPERTS, EXPERT_DIM = 118, 4, 8
USER_COLS, ACTION_COLS = 91, 27


def shapes(h1, h2):
    """(state_dict name, shape) of UserModel_MMOE's all-dense one-task build, in state_dict order."""
    return [("linear_model.weight", (D_IN, 1)), ("dnn.linears.0.weight", (h1, D_IN)), ("dnn.linears.0.bias", (h1,)),
            ("dnn.linears.1.weight", (h2, h1)), ("dnn.linears.1.bias", (h2,)),
            ("mmoe_layer.expert_network.weight", (N_EXPERTS * EXPERT_DIM, h2)), ("mmoe_layer.expert_network.bias", (N_EXPERTS * EXPERT_DIM,)),
            ("mmoe_layer.gating_networks.0.weight", (N_EXPERTS, h2)), ("tower_network.0.weight", (1, EXPERT_DIM)), ("out.0.bias", (1, 1)),
            ("linear_model_task.0.weight", (D_IN, 1))]


def exposure_virtualtaobao(timestamp, action, tau):
    """timestamp [n] (a row with 1 opens a session), action [n, 27] -> exposure [n, 1] float64:
    sum over the session's earlier rows j of exp(-(r - j) * ||a_r - a_j||_2 / tau); 0 for tau <= 0."""
    timestamp = np.asarray(timestamp).astype(np.int64).reshape(-1)
    action = np.asarray(action, np.float64)
    n = len(timestamp)
    out = np.zeros((n, 1))
    if n == 0:
        return out
    if timestamp[0] != 1:
        raise ValueError("the first row of the log must open a session (timestamp column == 1)")
    if tau <= 0:
        return out
    start = 0
    for r in range(n):
        if timestamp[r] == 1:
            start = r
            continue
        dist = np.sqrt(((action[start:r] - action[r]) ** 2).sum(1))
        out[r, 0] = np.exp(-(r - np.arange(start, r)) * dist / tau).sum()
    return out


def forward(p, x):
    """UserModel_MMOE.forward over the parameter dict p (reference names) -> [n, 1]."""
    h = torch.relu(x @ p["dnn.linears.0.weight"].t() + p["dnn.linears.0.bias"])
    h = torch.relu(h @ p["dnn.linears.1.weight"].t() + p["dnn.linears.1.bias"])
    experts = (h @ p["mmoe_layer.expert_network.weight"].t() + p["mmoe_layer.expert_network.bias"]).reshape(-1, EXPERT_DIM, N_EXPERTS)
    gate = (h @ p["mmoe_layer.gating_networks.0.weight"].t()).softmax(1)
    mix = torch.bmm(experts, gate.unsqueeze(-1)).squeeze(-1)
    logit = x @ p["linear_model_task.0.weight"] + mix @ p["tower_network.0.weight"].t()
    return logit + p["out.0.bias"]


def loss_taobao(y_pred, y, exposure):
    return (((1 / (1 + exposure) * y_pred - y) ** 2) * (y + 1)).mean()


def _regulariser(p, l2_linear, l2_all, dtype, device):
    """core/user_model.py's two lists: linear_model.weight (l2_linear) and EVERY parameter, linear_model.weight among them (l2_all) -> [1]."""
    reg = torch.zeros((1,), dtype=dtype, device=device)
    w = p["linear_model.weight"]
    reg = reg + torch.sum(l2_linear * w * w)
    for k in p:      # state_dict order = the reference's parameter order
        reg = reg + torch.sum(l2_all * p[k] * p[k])
    return reg


def _torch_train(forward_loss, init, cols, batch_size, steps, order, l2_linear, l2_all, lr, betas, eps, dtype, device, keep):
    """The optimiser loop of torch_train / mlp_torch_train: forward_loss(p, *batch columns) -> the data loss; cols: the columns as 2-d
    tensors, x first."""
    p = {k: torch.nn.Parameter(torch.as_tensor(np.asarray(v)).to(device, dtype).clone()) for k, v in init.items()}
    names = list(p)      # state_dict order = the reference's parameter order
    opt = torch.optim.Adam([p[k] for k in names], lr=lr, betas=betas, eps=eps)
    order = torch.arange(cols[0].shape[0], device=device) if order is None else torch.as_tensor(order).to(device)
    n_steps = (len(order) + batch_size - 1) // batch_size
    steps = n_steps if steps is None else min(steps, n_steps)
    losses, kept = [], {}
    for st in range(steps):
        idx = order[st * batch_size:(st + 1) * batch_size]
        loss = forward_loss(p, *(c[idx] for c in cols))
        opt.zero_grad()
        reg = _regulariser(p, l2_linear, l2_all, dtype, device)
        (loss + reg.squeeze()).backward()
        opt.step()
        losses.append([float(loss.detach()), float(reg.detach())])
        if st in keep:
            kept[st] = {k: v.detach().cpu().numpy().copy() for k, v in p.items()}
    return np.array(losses), kept, {k: v.detach().cpu().numpy().copy() for k, v in p.items()}


def torch_train(init, x, y, exposure, batch_size, steps=None, order=None, l2_linear=1e-5, l2_all=1e-2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                dtype=torch.float32, device="cpu", keep=()):
    """-> (losses [steps, 2] = {loss, reg}, {step index: parameters after that step (numpy) for the indices in `keep`}, final parameters)."""
    cols = [torch.as_tensor(np.asarray(x)).to(device, dtype)] + [torch.as_tensor(np.asarray(c)).to(device, dtype).reshape(-1, 1) for c in (y, exposure)]
    return _torch_train(lambda p, xb, yb, eb: loss_taobao(forward(p, xb), yb, eb), init, cols, batch_size, steps, order, l2_linear, l2_all, lr,
                        betas, eps, dtype, device, keep)


def _loss_and_grad(forward_loss, p, cols, l2_linear, l2_all, dtype):
    """One batch of _torch_train's loop without the optimiser -> (tensor {loss, reg}, {name: d (loss + reg) / d p[name]}), detached."""
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    cols = [torch.as_tensor(np.asarray(c)).to(dtype) for c in cols]
    loss = forward_loss(p, *cols)
    reg = _regulariser(p, l2_linear, l2_all, dtype, "cpu").squeeze()
    grads = torch.autograd.grad(loss + reg, list(p.values()))
    return torch.stack([loss.detach(), reg.detach()]), dict(zip(p, grads))


def loss_and_grad(p, x, y, exposure, l2_linear=1e-5, l2_all=1e-2, dtype=torch.float64):
    """p: a state_dict (numpy) of the one-task build, x [n, 118], y and exposure [n] or [n, 1] -> (the columns the device writes to
    loss_out = {data loss, regulariser}, {name: gradient of loss + reg}) in `dtype`."""
    x, y, e = np.asarray(x), np.asarray(y).reshape(-1, 1), np.asarray(exposure).reshape(-1, 1)
    return _loss_and_grad(lambda q, xb, yb, eb: loss_taobao(forward(q, xb), yb, eb), p, (x, y, e), l2_linear, l2_all, dtype)


def hidden_preactivations(p, x, dtype=torch.float64):
    """[z_0, z_1, ...]: z_l [n, H_l] = h_{l-1} W_l^T + b_l of every dnn.linears layer of p (either build), h_l = relu(z_l), in `dtype`."""
    h = torch.as_tensor(np.asarray(x)).to(dtype)
    out = []
    while f"dnn.linears.{len(out)}.weight" in p:
        w, b = (torch.as_tensor(np.asarray(p[f"dnn.linears.{len(out)}.{t}"])).to(dtype) for t in ("weight", "bias"))
        out.append(h @ w.t() + b)
        h = torch.relu(out[-1])
    return out


# ---- the two-task build of the static baselines (MLP-taobao.py, MLP-epsilonGreedy-taobao.py) ------------------------------------------
MLP_TASK_DIMS = (ACTION_COLS, 1)


def mlp_shapes(hidden, experts=N_EXPERTS, expert_dim=EXPERT_DIM):
    """(state_dict name, shape) of UserModel_MMOE's all-dense build with the tasks feat_item (27) and y (1), in state_dict order."""
    dims = [USER_COLS] + list(hidden)
    out = [("linear_model.weight", (USER_COLS, 1))]
    for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        out += [(f"dnn.linears.{l}.weight", (b, a)), (f"dnn.linears.{l}.bias", (b,))]
    out += [("mmoe_layer.expert_network.weight", (experts * expert_dim, dims[-1])), ("mmoe_layer.expert_network.bias", (experts * expert_dim,)),
            ("mmoe_layer.gating_networks.0.weight", (experts, dims[-1])), ("mmoe_layer.gating_networks.1.weight", (experts, dims[-1])),
            ("tower_network.0.weight", (ACTION_COLS, expert_dim)), ("tower_network.1.weight", (1, expert_dim)),
            ("out.0.bias", (1, ACTION_COLS)), ("out.1.bias", (1, 1)), ("linear_model_task.1.weight", (USER_COLS, 1))]
    return out


def mlp_shape_of(sd):
    """(hidden, experts, expert_dim) read off a state_dict of the two-task build; ValueError when it is not one."""
    try:
        n = len([k for k in sd if k.startswith("dnn.linears.") and k.endswith(".weight")])
        hidden = [int(sd[f"dnn.linears.{l}.weight"].shape[0]) for l in range(n)]
        experts = int(sd["mmoe_layer.gating_networks.0.weight"].shape[0])
        expert_dim = int(sd["mmoe_layer.expert_network.weight"].shape[0]) // max(experts, 1)
        want = dict(mlp_shapes(hidden, experts, expert_dim))
    except (KeyError, IndexError, AttributeError) as exc:
        raise ValueError(f"not the two-task UserModel_MMOE of the static baselines ({exc})") from None
    if n < 1 or set(sd) != set(want) or any(tuple(sd[k].shape) != want[k] for k in want):
        diff = sorted(set(sd) ^ set(want)) or sorted(k for k in want if tuple(sd[k].shape) != want[k])
        raise ValueError(f"unexpected parameters for the two-task UserModel_MMOE of the static baselines: {diff}")
    return hidden, experts, expert_dim


def mlp_forward(p, x):
    """UserModel_MMOE.forward of the two-task build over the parameter dict p (reference names) -> [n, 28] = [feat_item | y]."""
    h = x
    l = 0
    while f"dnn.linears.{l}.weight" in p:
        h = torch.relu(h @ p[f"dnn.linears.{l}.weight"].t() + p[f"dnn.linears.{l}.bias"])
        l += 1
    n_exp = p["mmoe_layer.gating_networks.0.weight"].shape[0]
    experts = (h @ p["mmoe_layer.expert_network.weight"].t() + p["mmoe_layer.expert_network.bias"]).reshape(len(x), -1, n_exp)
    outs = []
    for t in range(2):
        gate = (h @ p[f"mmoe_layer.gating_networks.{t}.weight"].t()).softmax(1)
        logit = torch.bmm(experts, gate.unsqueeze(-1)).squeeze(-1) @ p[f"tower_network.{t}.weight"].t()
        if t == 1:               # linear_model_task exists on the dimension-1 task only
            logit = x @ p["linear_model_task.1.weight"] + logit
        outs.append(logit + p[f"out.{t}.bias"])
    return torch.cat(outs, -1)


def loss_taobao_mlp(y_pred, y):
    """loss_taobao of MLP-taobao.py:137-155: the action task is masked by the click column (rows without a click teach no action),
    the click task is a plain mse; y = [27 item features | click]."""
    click = y[:, -1:]
    mse = torch.nn.functional.mse_loss
    return mse(click * y_pred[:, :ACTION_COLS], click * y[:, :ACTION_COLS]) + mse(y_pred[:, ACTION_COLS:], y[:, ACTION_COLS:])


def mlp_torch_train(init, x, y, batch_size, steps=None, order=None, l2_linear=1e-5, l2_all=1e-2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    dtype=torch.float32, device="cpu", keep=()):
    """x [N, 91], y [N, 28] -> (losses [steps, 2] = {loss, reg}, {step index: parameters after that step (numpy) for the indices in
    `keep`}, final parameters): torch_train for the two-task build."""
    cols = [torch.as_tensor(np.asarray(x)).to(device, dtype), torch.as_tensor(np.asarray(y)).to(device, dtype).reshape(-1, ACTION_COLS + 1)]
    return _torch_train(lambda p, xb, yb: loss_taobao_mlp(mlp_forward(p, xb), yb), init, cols, batch_size, steps, order, l2_linear, l2_all, lr,
                        betas, eps, dtype, device, keep)


def mlp_loss_and_grad(p, x, y, l2_linear=1e-5, l2_all=1e-2, dtype=torch.float64):
    """loss_and_grad for the two-task build: x [n, 91], y [n, 28]."""
    y = np.asarray(y).reshape(-1, ACTION_COLS + 1)
    return _loss_and_grad(lambda q, xb, yb: loss_taobao_mlp(mlp_forward(q, xb), yb), p, (np.asarray(x), y), l2_linear, l2_all, dtype)
