"""What the host restatements of the two Kuaishou trainers share (deepfm_host.py, dice_host.py); imports without libcirs_hip.so.

tower         the FM cross term and the DNN of one DeepFM network over a list of embedding rows
regulariser   core/user_model.py:401-417: embedding_dict.* (l2_embedding), linear_model.* (l2_linear), every parameter (l2_all)
tensor, leaf  the conversion of arrays / tensors to the run's dtype and of a state_dict's entries to autograd leaves
total_grad    d (loss + regulariser) / d p with the padding row of the feature table set to the regulariser's 2 c p
torch_train   the optimiser steps of fit_data (core/user_model.py:150-170) in plain torch (autograd + torch.optim.Adam) around a
              model's loss_and_grad"""
import numpy as np
import torch

FEAT = "embedding_dict.feat.weight"


def tower(p, dnn, last, out, vs, dense):
    """vs: the embedding rows [n,E] of the sparse fields, dense: [n,1] columns; dnn / last / out: the prefixes of the tower's parameter names
    -> (fm, dnn, out bias), separately: the two models add them to their linear part in different orders."""
    S = sum(vs)
    fm = 0.5 * ((S * S) - sum(v * v for v in vs)).sum(1)
    x = torch.cat(vs + dense, dim=1)
    h1 = torch.relu(x @ p[f"{dnn}.linears.0.weight"].T + p[f"{dnn}.linears.0.bias"])
    h2 = torch.relu(h1 @ p[f"{dnn}.linears.1.weight"].T + p[f"{dnn}.linears.1.bias"])
    return fm, (h2 @ p[f"{last}.weight"].T)[:, 0], p[f"{out}.bias"].reshape(())


def regulariser(p, l2_embedding=1e-5, l2_linear=1e-5, l2_all=0.1):
    reg = 0.0
    for k, v in p.items():
        c = l2_all + (l2_embedding if k.startswith("embedding_dict.") else 0.0) + (l2_linear if k.startswith("linear_model.") else 0.0)
        reg = reg + c * (v * v).sum()
    return reg


def tensor(v, dtype, device=None):
    v = v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    return v.to(v.device if device is None else device, dtype)


def leaf(v, dtype, device=None):
    """A leaf tensor of `dtype` that requires a gradient is used as it is."""
    if isinstance(v, torch.Tensor) and v.requires_grad and v.is_leaf and v.dtype == dtype:
        return v
    return tensor(v, dtype, device).clone().requires_grad_(True)


def total_grad(p, loss, reg, l2_embedding, l2_all):
    names = list(p)
    grads = dict(zip(names, torch.autograd.grad(loss + reg, [p[k] for k in names])))
    # nn.Embedding(padding_idx=0): the padding row never receives a data gradient, but it is regularised
    grads[FEAT][0] = 2 * (l2_all + l2_embedding) * p[FEAT].detach()[0]
    return grads


def torch_train(loss_and_grad, init, x, y, score, batch_size, steps, order, lr, betas, eps, dtype, keep, device="cpu"):
    """loss_and_grad(p, x, y, score) -> (loss columns, {name: gradient}) of one batch at the leaves p.  init: state_dict (numpy / tensors);
    batch b = rows order[b * batch_size : ...] (None: file order).  -> (losses [steps, columns], {step index: parameters after that step
    for the indices in `keep`}, final parameters)."""
    p = {k: tensor(v, dtype, device).clone().requires_grad_(True) for k, v in init.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr, betas=betas, eps=eps)
    x, y, score = tensor(x, dtype, device), tensor(y, dtype, device).reshape(-1), tensor(score, dtype, device).reshape(-1)
    order = torch.arange(x.shape[0], device=device) if order is None else torch.as_tensor(np.asarray(order)).long().to(device)
    n_steps = (len(order) + batch_size - 1) // batch_size
    steps = n_steps if steps is None else min(steps, n_steps)
    losses, kept = [], {}
    for st in range(steps):
        idx = order[st * batch_size:(st + 1) * batch_size]
        cols, grads = loss_and_grad(p, x[idx], y[idx], score[idx])
        for k, v in p.items():
            v.grad = grads[k]
        opt.step()
        losses.append(cols)
        if st in keep:
            kept[st] = {k: v.detach().cpu().clone().numpy() for k, v in p.items()}
    return torch.stack(losses).cpu().numpy().astype(np.float64), kept, {k: v.detach().cpu().clone().numpy() for k, v in p.items()}
