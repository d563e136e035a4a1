"""Device training of the pairwise DeepFM user model (csrc/deepfm_train.hip, cirs_deepfm_train_step / cirs_deepfm_train_epoch).

Host-side counterpart of fit_data's inner loop (reference core/user_model.py:150-170): parameters, gradients and the Adam
moments live in ONE flat fp32 device buffer each; named views follow the reference's state_dict.
`loss_kind` selects the loss of the row kernel: "pairwise" (loss_kuaishou_pairwise, CIRS-UserModel-kuaishou.py:262-278), "ips"
(loss_kuaishou_IPS_pairwise, DeepFM-IPS-pairwise.py:249-258) or "pd" (loss_kuaishou_PD_pairwise, PD-pairwise.py:242-251)."""
import ctypes as C
from typing import Dict

import torch

from . import abi
from .flat_train import TableTrainer

# (state_dict name, shape) in buffer order -- must match train_layout() in csrc/deepfm_train.hip (the six dnn / last / out slots: tower_net()
# of csrc/deepfm_tower.h)
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


class DeepFMTrainer(TableTrainer):
    _param_count, _workspace_bytes, _epoch_fn = "cirs_deepfm_train_param_count", "cirs_deepfm_train_workspace_bytes", "cirs_deepfm_train_epoch"
    LOSS_COLUMNS = ("loss", "loss_y", "bpr", "loss_ab", "reg_loss")
    split_columns = staticmethod(split_columns)

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, use_ab=True, lambda_ab=1.0, l2_embedding=1e-5, l2_linear=1e-5, l2_all=1e-1,
                 lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device="cuda", loss_kind="pairwise"):
        if loss_kind not in LOSS_KINDS:
            raise ValueError(f"loss_kind must be one of {sorted(LOSS_KINDS)}, got {loss_kind!r}")
        if use_ab and loss_kind != "pairwise":
            raise ValueError(f"the {loss_kind!r} loss takes no alpha/beta: build the trainer with use_ab=False")
        self.loss_kind = loss_kind
        self.use_ab, self.lambda_ab = bool(use_ab), float(lambda_ab)
        sd = {k: torch.as_tensor(v) for k, v in state_dict.items()}
        U, E = sd["embedding_dict.user_id.weight"].shape
        I = sd["embedding_dict.photo_id.weight"].shape[0]
        F = sd["embedding_dict.feat.weight"].shape[0]
        cfg = abi.DeepFMCfg(n_user_vocab=U, n_item_vocab=I, n_feat_vocab=F, emb_dim=E, hidden=64)
        # without alpha/beta the model has no such parameters: zeros carry neither a regulariser term nor a gradient
        self._setup(cfg, layout(U, I, F, E), sd, lambda name: 1.0 if use_ab and name.startswith("ab_embedding_dict") else 0.0,
                    (l2_embedding, l2_linear, l2_all), lr, betas, eps, device)

    def state_dict(self):
        return {k: v for k, v in super().state_dict().items() if self.use_ab or not k.startswith("ab_embedding_dict")}

    def validate(self, valset, want_pred=False, want_sums=True):
        """The validation pass (cirs_deepfm_validate) of the LIVE parameters over a cirs_hip.userval.ValSet: the weights struct points
        into the flat buffer's views -> (pred or None, sums or None)."""
        from .deepfm import STATE_DICT_MAP
        from .userval import deepfm_validate
        if getattr(self, "_val_w", None) is None:
            self._val_w = abi.DeepFMWeights(**{f: self.views[k].data_ptr() for k, f in STATE_DICT_MAP.items()})
        return deepfm_validate(self.cfg, self._val_w, valset, want_pred, want_sums)

    def _hyper(self):
        return (int(self.use_ab), self.lambda_ab, *self._adam())

    def _epoch_args(self):
        return (LOSS_KINDS[self.loss_kind], *self._hyper())

    def step(self, x: torch.Tensor, y: torch.Tensor, score: torch.Tensor):
        """x [n,14] = positive pair columns [user, photo, feat0..3, duration] then the negative pair's (user_model_pairwise.py:136-137);
        y [n] or [n,1]; score [n] or [n,1] = exposure (IPS weight / popularity for the other two loss kinds).  Returns the device loss
        vector {loss, loss_y, bpr, loss_ab, reg_loss}."""
        cols = split_columns(x, y, score, self.device)
        if self.loss_kind != "pairwise":     # the step entry knows the pairwise loss only
            return self._step_as_epoch(cols)
        n = cols[0].numel()
        ws = self._workspace(n)
        abi.check(self._lib.cirs_deepfm_train_step(*self._buffers(), *[c.data_ptr() for c in cols], n, *self._hyper(), self.loss.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), self._stream()), "cirs_deepfm_train_step")
        self.step_count += 1
        return self.loss
