"""Host restatement of the DeepFM user-model training step (csrc/deepfm_train.hip) for its three loss kinds; imports without
libcirs_hip.so.

torch_train   the optimiser steps of UserModel_Pairwise.fit_data (reference core/user_model.py:150-170) in plain torch (autograd +
              torch.optim.Adam) over a state_dict under the reference's names, in fp32 or fp64:
                forward      core/user_model_pairwise.py:98-132 (linear + FM + DNN)
                loss         "pairwise"  loss_kuaishou_pairwise       CIRS-UserModel-kuaishou.py:262-278
                             "ips"       loss_kuaishou_IPS_pairwise   DeepFM-IPS-pairwise.py:249-258
                             "pd"        loss_kuaishou_PD_pairwise    PD-pairwise.py:242-251
                regulariser  core/user_model.py:401-417: embedding_dict.* (l2_embedding), linear_model.* (l2_linear), every
                             parameter (l2_all); the padding row of the feature table gets no data gradient and still decays
              The comparison object of the device step for the two debiasing losses, which the test oracle does not know, in tests
              and in tools/probe_usertrain.py.
loss_and_grad the loss columns and the total gradient (loss + regulariser) of one batch; torch_train's step and, in float64, the
              reference of the device's gradient buffer (tests/gradcase.py)."""
import torch

from . import usertrain_host as H

LOSS_KINDS = ("pairwise", "ips", "pd")


def pair_forward(p, X):
    """X [n,7] = [user, photo, feat0..3, duration] -> y [n] over the parameter dict p (reference names)."""
    ids = X[:, :6].long()
    dur = X[:, 6:7]
    vs = [p["embedding_dict.user_id.weight"][ids[:, 0]], p["embedding_dict.photo_id.weight"][ids[:, 1]]] + \
         [p["embedding_dict.feat.weight"][ids[:, 2 + q]] for q in range(4)]
    lin = p["linear.embedding_dict.user_id.weight"][ids[:, 0], 0] + p["linear.embedding_dict.photo_id.weight"][ids[:, 1], 0]
    for q in range(4):
        lin = lin + p["linear.embedding_dict.feat.weight"][ids[:, 2 + q], 0]
    lin = lin + dur[:, 0] * p["linear.weight"].reshape(())
    fm, dnn, out = H.tower(p, "dnn", "last", "out", vs, [dur])
    return lin + fm + dnn + out


def loss_terms(kind, y, yp, yn, score, alpha=None, beta=None):
    """-> (loss_y, bpr, loss_ab) of one batch; score = exposure ("pairwise"), IPS weight ("ips") or popularity ** gamma ("pd")."""
    log_sg = torch.log(torch.sigmoid(yp - yn))
    zero = torch.zeros((), dtype=yp.dtype, device=yp.device)
    if kind == "pairwise":
        ex_new, loss_ab = score, zero
        if alpha is not None:
            ex_new = score * alpha * beta
            loss_ab = ((alpha - 1) ** 2).mean() + ((beta - 1) ** 2).mean()
        return ((yp / (1 + ex_new) - y) ** 2).mean(), -log_sg.mean(), loss_ab
    if kind == "ips":
        return (((yp - y) ** 2) * score).mean(), -(log_sg * score).mean(), zero
    if kind == "pd":
        return ((yp * score - y) ** 2).mean(), -log_sg.mean(), zero
    raise ValueError(f"loss kind must be one of {LOSS_KINDS}, got {kind!r}")


def loss_and_grad(p, x, y, score, kind="pairwise", use_ab=False, lambda_ab=0.0, l2_embedding=1e-5, l2_linear=1e-5, l2_all=0.1,
                  dtype=torch.float64):
    """Loss and total gradient of one batch: p a state_dict (numpy / tensors; leaf tensors of `dtype` that require a gradient are used as
    they are), x [n,14], y and score [n] or [n,1].  -> (loss columns in the device's order {loss, loss_y, bpr, loss_ab, reg} as one detached
    tensor, {name: d (loss + reg) / d p[name]}).  The padding row 0 of embedding_dict.feat.weight carries the regulariser's 2 c p only
    (nn.Embedding(padding_idx=0)); linear_model.* is moved by the regulariser alone; without alpha/beta the ab_* tensors are not
    parameters: absent from p, they are absent from the gradient."""
    if use_ab and kind != "pairwise":
        raise ValueError(f"the {kind!r} loss takes no alpha/beta")

    p = {k: H.leaf(v, dtype) for k, v in p.items()}
    xb, yb, sb = H.tensor(x, dtype), H.tensor(y, dtype).reshape(-1), H.tensor(score, dtype).reshape(-1)
    yp, yn = pair_forward(p, xb[:, :7]), pair_forward(p, xb[:, 7:])
    alpha = beta = None
    if use_ab:
        alpha = p["ab_embedding_dict.alpha_u.weight"][xb[:, 0].long(), 0]
        beta = p["ab_embedding_dict.beta_i.weight"][xb[:, 1].long(), 0]
    loss_y, bpr, loss_ab = loss_terms(kind, yb, yp, yn, sb, alpha, beta)
    loss = loss_y + bpr + lambda_ab * loss_ab
    reg = H.regulariser(p, l2_embedding, l2_linear, l2_all)
    grads = H.total_grad(p, loss, reg, l2_embedding, l2_all)
    return torch.stack([t.detach() for t in (loss, loss_y, bpr, loss_ab, reg)]), grads


def torch_train(init, x, y, score, batch_size, steps=None, order=None, kind="pairwise", use_ab=False, lambda_ab=0.0, l2_embedding=1e-5,
                l2_linear=1e-5, l2_all=0.1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float32, keep=()):
    """init: state_dict (numpy / tensors); x [N,14], y [N] or [N,1], score likewise; batch b = rows order[b * batch_size : ...] (None: file
    order).  -> (losses [steps, 5] = {loss, loss_y, bpr, loss_ab, reg}, {step index: parameters after that step for the indices in
    `keep`}, final parameters)."""
    if use_ab and kind != "pairwise":
        raise ValueError(f"the {kind!r} loss takes no alpha/beta")
    return H.torch_train(lambda p, xb, yb, sb: loss_and_grad(p, xb, yb, sb, kind, use_ab, lambda_ab, l2_embedding, l2_linear, l2_all, dtype),
                         init, x, y, score, batch_size, steps, order, lr, betas, eps, dtype, keep)
