"""Host restatement of the DICE debiasing baseline (csrc/dice_train.hip); imports without libcirs_hip.so.

forward       UserModel_DICE.forward (reference core/user_model_DICE.py:189-192): the main DeepFM with the user and the photo id in
              both of their columns
get_loss      UserModel_DICE.get_loss (:162-187): the main DeepFM on the positive and the negative row, the UI DeepFM on the int and
              the con (user, photo) pair of each, then loss_kuaishou_DICE (DICE.py:273-286)
torch_train   the optimiser steps of fit_data (core/user_model.py:150-170) in plain torch (autograd + torch.optim.Adam) over a
              state_dict under the reference's names, in fp32 or fp64, on any device.  Regulariser (core/user_model.py:401-417):
              embedding_dict.* (l2_embedding), linear_model.* (l2_linear; unused in the forward, still decayed), every parameter
              (l2_all); the padding row of the feature table gets no data gradient and still decays.
              The comparison object of the device step in tests and in tools/probe_usertrain.py.
loss_and_grad the loss columns and the total gradient (loss + regulariser) of one batch; torch_train's step and, in float64, the
              reference of the device's gradient buffer (tests/gradcase.py)."""
import torch

from . import usertrain_host as H
from .usertrain_host import regulariser  # noqa: F401  (tools/probe_usertrain.py times it as part of this model's step)

TABLES = ("user_int", "user_con", "photo_int", "photo_con")


def _tower(p, name, vs, dense):
    fm, dnn, out = H.tower(p, f"dnn_{name}", f"last_{name}", f"out_{name}", vs, dense)
    return fm + dnn + out


def main_forward(p, X):
    """X [n,9] = [user_int, user_con, photo_int, photo_con, feat0..3, duration] -> y [n] (is_main=True)."""
    ids = X[:, :8].long()
    dur = X[:, 8:9]
    vs = [p[f"embedding_dict.{t}.weight"][ids[:, q]] for q, t in enumerate(TABLES)] + [p["embedding_dict.feat.weight"][ids[:, 4 + q]] for q in range(4)]
    lin = sum(p[f"linear_main.embedding_dict.{t}.weight"][ids[:, q], 0] for q, t in enumerate(TABLES))
    for q in range(4):
        lin = lin + p["linear_main.embedding_dict.feat.weight"][ids[:, 4 + q], 0]
    lin = lin + dur[:, 0] * p["linear_main.weight"].reshape(())
    return lin + _tower(p, "main", vs, [dur])


def ui_forward(p, u, i, kind):
    """(user ids, photo ids) [n] of the `kind` ("int" / "con") columns -> y [n] (is_main=False).  linear_ui owns the tables user_int and
    photo_int only and is indexed with whatever ids the call was given (core/user_model_DICE.py:92, 173-181)."""
    u, i = u.long(), i.long()
    vs = [p[f"embedding_dict.user_{kind}.weight"][u], p[f"embedding_dict.photo_{kind}.weight"][i]]
    lin = p["linear_ui.embedding_dict.user_int.weight"][u, 0] + p["linear_ui.embedding_dict.photo_int.weight"][i, 0]
    return lin + _tower(p, "ui", vs, [])


def forward(p, x7):
    """x7 [n,7] = [user, photo, feat0..3, duration] -> y [n]."""
    return main_forward(p, torch.cat([x7[:, 0:1], x7[:, 0:2], x7[:, 1:]], dim=1))


def loss_terms(y, yp, yn, ypi, yni, ypc, ync, score):
    """loss_kuaishou_DICE -> (loss_y, bpr_click, bpr_con, bpr_int)."""
    return (((yp - y) ** 2).mean(), -torch.sigmoid(yp - yn).log().mean(), -(torch.sigmoid(ypc - ync).log() * score).mean(),
            -(torch.sigmoid(ypi - yni).log() * (score < 0)).mean())


def get_loss(p, x, y, score):
    """x [n,16] -> (loss_y, bpr_click, bpr_con, bpr_int)."""
    yp = main_forward(p, x[:, :9])
    yn = main_forward(p, torch.cat([x[:, :2], x[:, 9:]], dim=1))
    ypi, yni = ui_forward(p, x[:, 0], x[:, 2], "int"), ui_forward(p, x[:, 0], x[:, 9], "int")
    ypc, ync = ui_forward(p, x[:, 1], x[:, 3], "con"), ui_forward(p, x[:, 1], x[:, 10], "con")
    return loss_terms(y, yp, yn, ypi, yni, ypc, ync, score)


def loss_and_grad(p, x, y, score, l2_embedding=1e-5, l2_linear=1e-5, l2_all=0.1, dtype=torch.float64, device=None):
    """Loss and total gradient of one batch: p a state_dict (numpy / tensors; leaf tensors of `dtype` that require a gradient are used as
    they are), x [n,16], y and score [n] or [n,1].  -> (loss columns in the device's order {loss, loss_y, bpr_click, bpr_con, bpr_int,
    reg} as one detached tensor, {name: d (loss + reg) / d p[name]}).  The padding row 0 of embedding_dict.feat.weight carries the
    regulariser's 2 c p only (nn.Embedding(padding_idx=0)); linear_model.* is moved by the regulariser alone."""
    p = {k: H.leaf(v, dtype, device) for k, v in p.items()}
    terms = get_loss(p, H.tensor(x, dtype, device), H.tensor(y, dtype, device).reshape(-1), H.tensor(score, dtype, device).reshape(-1))
    loss = terms[0] + terms[1] + terms[2] + terms[3]
    reg = regulariser(p, l2_embedding, l2_linear, l2_all)
    grads = H.total_grad(p, loss, reg, l2_embedding, l2_all)
    return torch.stack([v.detach() for v in (loss,) + terms + (reg,)]), grads


def torch_train(init, x, y, score, batch_size, steps=None, order=None, l2_embedding=1e-5, l2_linear=1e-5, l2_all=0.1, lr=1e-3,
                betas=(0.9, 0.999), eps=1e-8, dtype=torch.float32, keep=(), device="cpu"):
    """init: state_dict (numpy / tensors); x [N,16], y [N] or [N,1], score likewise; batch b = rows order[b * batch_size : ...] (None: file
    order).  -> (losses [steps, 6] = {loss, loss_y, bpr_click, bpr_con, bpr_int, reg}, {step index: parameters after that step for the
    indices in `keep`}, final parameters)."""
    return H.torch_train(lambda p, xb, yb, sb: loss_and_grad(p, xb, yb, sb, l2_embedding, l2_linear, l2_all, dtype, device),
                         init, x, y, score, batch_size, steps, order, lr, betas, eps, dtype, keep, device)
