"""Device training of the pairwise DeepFM user model (csrc/deepfm_train.hip, cirs_deepfm_train_step / cirs_deepfm_train_epoch).

Host-side counterpart of fit_data's inner loop (reference core/user_model.py:150-170): parameters, gradients and the Adam
moments live in ONE flat fp32 device buffer each; named views follow the reference's state_dict.
`loss_kind` selects the loss of the row kernel: "pairwise" (loss_kuaishou_pairwise, CIRS-UserModel-kuaishou.py:262-278), "ips"
(loss_kuaishou_IPS_pairwise, DeepFM-IPS-pairwise.py:249-258) or "pd" (loss_kuaishou_PD_pairwise, PD-pairwise.py:242-251)."""
import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import abi

# (state_dict name, layout slot) in buffer order -- must match train_layout() in csrc/deepfm_train.hip
def layout(U: int, I: int, F: int, E: int):
    K = 6 * E + 1
    return [("embedding_dict.user_id.weight", (U, E)), ("embedding_dict.photo_id.weight", (I, E)), ("embedding_dict.feat.weight", (F, E)),
            ("linear.embedding_dict.user_id.weight", (U, 1)), ("linear.embedding_dict.photo_id.weight", (I, 1)),
            ("linear.embedding_dict.feat.weight", (F, 1)), ("linear.weight", (1, 1)),
            ("dnn.linears.0.weight", (64, K)), ("dnn.linears.0.bias", (64,)), ("dnn.linears.1.weight", (64, 64)), ("dnn.linears.1.bias", (64,)),
            ("last.weight", (1, 64)), ("out.bias", (1, 1)),
            ("ab_embedding_dict.alpha_u.weight", (U, 1)), ("ab_embedding_dict.beta_i.weight", (I, 1)),
            ("linear_model.embedding_dict.user_id.weight", (U, 1)), ("linear_model.embedding_dict.photo_id.weight", (I, 1)),
            ("linear_model.embedding_dict.feat.weight", (F, 1)), ("linear_model.weight", (1, 1))]


LOSS_KINDS = {"pairwise": 0, "ips": 1, "pd": 2}


def split_columns(x, y, score, device):
    """x [n,14] = positive pair columns [user, photo, feat0..3, duration] then the negative pair's (user_model_pairwise.py:136-137),
    y and score [n] or [n,1] -> the ten device columns the kernels take (eight pair columns, y, score)."""
    x = torch.as_tensor(x).to(device)
    ids = x[:, [0, 1, 7, 8]].to(torch.int64)
    cols = [ids[:, 0].contiguous(), ids[:, 1].contiguous(), x[:, 2:6].to(torch.int32).contiguous(), x[:, 6].to(torch.float32).contiguous(),
            ids[:, 2].contiguous(), ids[:, 3].contiguous(), x[:, 9:13].to(torch.int32).contiguous(), x[:, 13].to(torch.float32).contiguous()]
    y = torch.as_tensor(y).to(device, torch.float32).reshape(-1).contiguous()
    score = torch.as_tensor(score).to(device, torch.float32).reshape(-1).contiguous()
    assert y.numel() == x.shape[0] and score.numel() == x.shape[0], "x, y and score must have one row per sample"
    return cols + [y, score]


class DeepFMTrainer:
    def __init__(self, state_dict: Dict[str, torch.Tensor], *, use_ab=True, lambda_ab=1.0, l2_embedding=1e-5, l2_linear=1e-5, l2_all=1e-1,
                 lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device="cuda", loss_kind="pairwise"):
        if loss_kind not in LOSS_KINDS:
            raise ValueError(f"loss_kind must be one of {sorted(LOSS_KINDS)}, got {loss_kind!r}")
        if use_ab and loss_kind != "pairwise":
            raise ValueError(f"the {loss_kind!r} loss takes no alpha/beta: build the trainer with use_ab=False")
        self.loss_kind = loss_kind
        self.device = torch.device(device)
        sd = {k: torch.as_tensor(v) for k, v in state_dict.items()}
        U, E = sd["embedding_dict.user_id.weight"].shape
        I = sd["embedding_dict.photo_id.weight"].shape[0]
        F = sd["embedding_dict.feat.weight"].shape[0]
        self.cfg = abi.DeepFMCfg(n_user_vocab=U, n_item_vocab=I, n_feat_vocab=F, emb_dim=E, hidden=64)
        self._lib = abi.lib()
        total = self._lib.cirs_deepfm_train_param_count(C.byref(self.cfg))
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.views = {}
        off = 0
        for name, shape in layout(U, I, F, E):
            n = int(np.prod(shape))
            self.views[name] = self.flat[off:off + n].view(shape)
            if name in sd:
                self.views[name].copy_(sd[name].to(self.device, torch.float32).reshape(shape))
            elif name.startswith("ab_embedding_dict"):
                # without alpha/beta the model has no such parameters: zeros carry neither a regulariser term nor a gradient
                self.views[name].fill_(1.0 if use_ab else 0.0)
            off += n
        assert off == total
        self.grads = torch.zeros_like(self.flat)
        self.adam_m = torch.zeros_like(self.flat)
        self.adam_v = torch.zeros_like(self.flat)
        self.step_count = 0
        self.use_ab, self.lambda_ab = bool(use_ab), float(lambda_ab)
        self.l2 = (float(l2_embedding), float(l2_linear), float(l2_all))
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self._ws = None
        self._data = None
        self.loss = torch.zeros(5, dtype=torch.float32, device=self.device)

    def state_dict(self):
        return {k: v.clone() for k, v in self.views.items() if self.use_ab or not k.startswith("ab_embedding_dict")}

    def _workspace(self, n):
        need = self._lib.cirs_deepfm_train_workspace_bytes(C.byref(self.cfg), n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def validate(self, valset, want_pred=False, want_sums=True):
        """The validation pass (cirs_deepfm_validate) of the LIVE parameters over a cirs_hip.userval.ValSet: the weights struct points
        into the flat buffer's views -> (pred or None, sums or None)."""
        from .deepfm import STATE_DICT_MAP
        from .userval import deepfm_validate
        if getattr(self, "_val_w", None) is None:
            self._val_w = abi.DeepFMWeights(**{f: self.views[k].data_ptr() for k, f in STATE_DICT_MAP.items()})
        return deepfm_validate(self.cfg, self._val_w, valset, want_pred, want_sums)

    def _hyper(self):
        return (int(self.use_ab), self.lambda_ab, *self.l2, self.lr, self.betas[0], self.betas[1], self.eps)

    def step(self, x: torch.Tensor, y: torch.Tensor, score: torch.Tensor):
        """x [n,14] = positive pair columns [user, photo, feat0..3, duration] then the negative pair's (user_model_pairwise.py:136-137);
        y [n] or [n,1]; score [n] or [n,1] = exposure (IPS weight / popularity for the other two loss kinds).  Returns the device loss
        vector {loss, loss_y, bpr, loss_ab, reg_loss}."""
        cols = split_columns(x, y, score, self.device)
        n = cols[0].numel()
        if self.loss_kind != "pairwise":     # one step of the IPS / PD loss = a pass of one batch over these rows
            self.loss.copy_(self._run_epoch(cols, n, None, n, n)[0])
            return self.loss
        ws = self._workspace(n)
        abi.check(self._lib.cirs_deepfm_train_step(
            C.byref(self.cfg), self.flat.data_ptr(), self.grads.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.step_count,
            *[c.data_ptr() for c in cols], n, *self._hyper(), self.loss.data_ptr(), ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream(self.device).cuda_stream), "cirs_deepfm_train_step")
        self.step_count += 1
        return self.loss

    def load(self, x, y, score):
        """Make the data set resident on the device in the column form of the kernels (the split runs once); epoch() trains on it."""
        self._data = split_columns(x, y, score, self.device)
        return self._data[0].numel()

    def _run_epoch(self, cols, n_rows, order, n_order, batch_size):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        if n_rows < 1 or n_order < 1:
            raise ValueError("empty data set or index array")
        steps = (n_order + batch_size - 1) // batch_size
        losses = torch.zeros(steps, 5, dtype=torch.float32, device=self.device)
        ws = self._workspace(min(int(batch_size), n_order))
        abi.check(self._lib.cirs_deepfm_train_epoch(
            C.byref(self.cfg), self.flat.data_ptr(), self.grads.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.step_count,
            *[c.data_ptr() for c in cols], n_rows, abi.ptr(order), n_order, int(batch_size), LOSS_KINDS[self.loss_kind], *self._hyper(),
            losses.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream), "cirs_deepfm_train_epoch")
        self.step_count += steps
        return losses

    def epoch(self, order, batch_size, check=True):
        """One pass over the loaded data set from one call: batch b is the rows order[b * batch_size : (b + 1) * batch_size] (int64 indices
        into the data set; None = every row in file order), the last batch short.  Returns the [steps, 5] device tensor of per-step
        {loss, loss_y, bpr, loss_ab, reg_loss}.  check=False skips the range check of `order` (one read-back in front of the pass) for a
        caller that built the permutation itself; the kernel answers an index outside the data set with a NaN loss, not a read."""
        assert getattr(self, "_data", None) is not None, "call load(x, y, score) first"
        n_rows = self._data[0].numel()
        if order is None:
            return self._run_epoch(self._data, n_rows, None, n_rows, batch_size)
        order = torch.as_tensor(order).to(self.device, torch.int64).reshape(-1).contiguous()
        if check and order.numel():
            lo, hi = torch.aminmax(order)     # checked in front of the pass; the steps themselves run without a host round trip
            if int(lo) < 0 or int(hi) >= n_rows:
                raise IndexError(f"order holds row indices outside [0, {n_rows})")
        return self._run_epoch(self._data, n_rows, order, order.numel(), batch_size)
