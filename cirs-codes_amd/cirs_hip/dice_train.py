"""Device training and evaluation of the DICE debiasing baseline (csrc/dice_train.hip: cirs_dice_train_epoch, cirs_dice_forward).

Host-side counterpart of fit_data's inner loop (reference core/user_model.py:150-170) for UserModel_DICE (core/user_model_DICE.py,
loss_kuaishou_DICE of DICE.py:273-286): parameters, gradients and the Adam moments live in ONE flat fp32 device buffer each; named
views follow the reference's state_dict.  DeviceDice is the evaluation side (forward / sweep) over the same flat layout."""
import ctypes as C
from typing import Dict

import torch

from . import abi
from .flat_train import TableTrainer, fill_views

TABLES = (("user_int", "U"), ("user_con", "U"), ("photo_int", "I"), ("photo_con", "I"), ("feat", "F"))
LOSS_COLUMNS = ("loss", "loss_y", "bpr_click", "bpr_con", "bpr_int", "reg")


# (state_dict name, shape) in buffer order -- must match dice_layout() in csrc/dice_train.hip (a tower's six slots: tower_net() of
# csrc/deepfm_tower.h)
def layout(U: int, I: int, F: int, E: int):
    V = {"U": U, "I": I, "F": F}

    def tower(name, K):
        return [(f"dnn_{name}.linears.0.weight", (64, K)), (f"dnn_{name}.linears.0.bias", (64,)), (f"dnn_{name}.linears.1.weight", (64, 64)),
                (f"dnn_{name}.linears.1.bias", (64,)), (f"last_{name}.weight", (1, 64)), (f"out_{name}.bias", (1, 1))]
    return [(f"embedding_dict.{t}.weight", (V[v], E)) for t, v in TABLES] + \
           [(f"linear_main.embedding_dict.{t}.weight", (V[v], 1)) for t, v in TABLES] + [("linear_main.weight", (1, 1))] + \
           [("linear_ui.embedding_dict.user_int.weight", (U, 1)), ("linear_ui.embedding_dict.photo_int.weight", (I, 1))] + \
           tower("main", 8 * E + 1) + tower("ui", 2 * E) + \
           [(f"linear_model.embedding_dict.{t}.weight", (V[v], 1)) for t, v in TABLES] + [("linear_model.weight", (2, 1))]


def _cfg_of(state_dict):
    """-> (tensors of the state_dict, cfg, its layout)."""
    sd = {k: torch.as_tensor(v) for k, v in state_dict.items()}
    U, E = sd["embedding_dict.user_int.weight"].shape
    I = sd["embedding_dict.photo_int.weight"].shape[0]
    F = sd["embedding_dict.feat.weight"].shape[0]
    if E not in (8, 16, 32):
        raise ValueError(f"the DICE device model takes an embedding size of 8, 16 or 32, got {E}")
    if tuple(sd["dnn_main.linears.0.weight"].shape) != (64, 8 * E + 1) or tuple(sd["dnn_ui.linears.0.weight"].shape) != (64, 2 * E):
        raise ValueError("the DICE device model takes dnn_hidden_units == (64, 64) and entity_dim == feature_dim")
    return sd, abi.DiceCfg(n_user_vocab=U, n_item_vocab=I, n_feat_vocab=F, emb_dim=E, hidden=64), layout(U, I, F, E)


def _absent(name):
    if name.startswith("linear_model."):       # the unused copy may be absent from a hand-made dict
        return 0.0
    raise KeyError(name)


def split_columns(x, y, score, device):
    """x [n,16] = [user_int, user_con, photo_int, photo_con, feat0..3, dur | photo_int_neg, photo_con_neg, feat0..3_neg, dur_neg]
    (reference DICE.py:153-173), y and score [n] or [n,1] -> the twelve device columns of cirs_dice_train_epoch."""
    x = torch.as_tensor(x).to(device)
    assert x.dim() == 2 and x.shape[1] == 16, "x must have the 16 columns of load_dataset_kuaishou_DICE"
    ids = x[:, [0, 1, 2, 3, 9, 10]].to(torch.int64)
    cols = [ids[:, 0].contiguous(), ids[:, 1].contiguous(), ids[:, 2].contiguous(), ids[:, 3].contiguous(),
            x[:, 4:8].to(torch.int32).contiguous(), x[:, 8].to(torch.float32).contiguous(),
            ids[:, 4].contiguous(), ids[:, 5].contiguous(), x[:, 11:15].to(torch.int32).contiguous(), x[:, 15].to(torch.float32).contiguous()]
    y = torch.as_tensor(y).to(device, torch.float32).reshape(-1).contiguous()
    score = torch.as_tensor(score).to(device, torch.float32).reshape(-1).contiguous()
    assert y.numel() == x.shape[0] and score.numel() == x.shape[0], "x, y and score must have one row per sample"
    return cols + [y, score]


class DiceTrainer(TableTrainer):
    _param_count, _workspace_bytes, _epoch_fn = "cirs_dice_train_param_count", "cirs_dice_train_workspace_bytes", "cirs_dice_train_epoch"
    LOSS_COLUMNS = LOSS_COLUMNS
    split_columns = staticmethod(split_columns)

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, l2_embedding=1e-5, l2_linear=1e-5, l2_all=1e-1, lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, device="cuda"):
        sd, cfg, names = _cfg_of(state_dict)
        self._setup(cfg, names, sd, _absent, (l2_embedding, l2_linear, l2_all), lr, betas, eps, device)

    _epoch_args = TableTrainer._adam

    def _check_ids(self, cols):
        """The kernels index the tables with the data set's ids as they are: one range check per data set, in front of the passes."""
        c = self.cfg
        for what, ts, hi in (("user", (cols[0], cols[1]), c.n_user_vocab), ("photo", (cols[2], cols[3], cols[6], cols[7]), c.n_item_vocab),
                             ("feat", (cols[4], cols[8]), c.n_feat_vocab)):
            for t in ts:
                lo, up = torch.aminmax(t)
                if int(lo) < 0 or int(up) >= hi:
                    raise IndexError(f"{what} ids outside [0, {hi})")

    def validate(self, valset, want_pred=False, want_sums=True):
        """The validation pass (cirs_dice_validate) of the LIVE parameters over a cirs_hip.userval.ValSet -> (pred or None, sums or None)."""
        from .userval import dice_validate
        return dice_validate(self.cfg, self.flat, valset, want_pred, want_sums)

    def step(self, x, y, score):
        """One optimiser step on the batch x [n,16], y, score [n] or [n,1].  Returns the device loss vector {loss, loss_y, bpr_click,
        bpr_con, bpr_int, reg}."""
        cols = split_columns(x, y, score, self.device)
        self._check_ids(cols)
        return self._step_as_epoch(cols)


class DeviceDice:
    """UserModel_DICE.forward on the device: the interface of cirs_hip.deepfm.DeviceDeepFM that UserModel.recommend_k_item,
    evaluation.interactive_evaluation and KuaishouEnv.compute_normed_reward call."""
    PAIRS_PER_CALL = 1 << 22

    def __init__(self, state_dict, device="cuda"):
        self.device = torch.device(device)
        self._lib = abi.lib()
        sd, self.cfg, names = _cfg_of(state_dict)
        self.flat = torch.zeros(self._lib.cirs_dice_train_param_count(C.byref(self.cfg)), dtype=torch.float32, device=self.device)
        self.views = fill_views(self.flat, names, sd, _absent)

    def forward(self, uid, pid, feats, dur):
        dev = self.device
        uid = torch.as_tensor(uid).to(dev, torch.int64).contiguous(); pid = torch.as_tensor(pid).to(dev, torch.int64).contiguous()
        feats = torch.as_tensor(feats).to(dev, torch.int32).contiguous(); dur = torch.as_tensor(dur).to(dev, torch.float32).contiguous()
        n = uid.numel()
        assert pid.numel() == n and dur.numel() == n and feats.numel() == 4 * n, "one (uid, pid, feats[4], dur) per row"
        out = torch.empty(n, dtype=torch.float32, device=dev)
        abi.check(self._lib.cirs_dice_forward(C.byref(self.cfg), self.flat.data_ptr(), uid.data_ptr(), pid.data_ptr(), feats.data_ptr(),
                                              dur.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cirs_dice_forward")
        return out

    def validate(self, valset, want_pred=False, want_sums=True):
        """The validation pass (cirs_dice_validate) over a cirs_hip.userval.ValSet -> (pred [n] fp32 or None, float64 device pair
        {sum |pred - y|, sum (pred - y)^2} or None)."""
        from .userval import dice_validate
        return dice_validate(self.cfg, self.flat, valset, want_pred, want_sums)

    def sweep(self, user_ids, item_ids, item_feats, item_dur, want_pred=True):
        """All (user, item) pairs -> (pred [nu, ni] fp32, minmax [2]): cirs_dice_forward over the nu * ni pairs, a block of users per call."""
        dev = self.device
        user_ids = torch.as_tensor(user_ids).to(dev, torch.int64).reshape(-1); item_ids = torch.as_tensor(item_ids).to(dev, torch.int64).reshape(-1)
        item_feats = torch.as_tensor(item_feats).to(dev, torch.int32).reshape(-1, 4); item_dur = torch.as_tensor(item_dur).to(dev, torch.float32).reshape(-1)
        nu, ni = user_ids.numel(), item_ids.numel()
        pred = torch.empty((nu, ni), dtype=torch.float32, device=dev)
        ub = max(1, self.PAIRS_PER_CALL // max(ni, 1))
        for u0 in range(0, nu, ub):
            u = user_ids[u0:u0 + ub]
            k = u.numel()
            pred[u0:u0 + k] = self.forward(u.repeat_interleave(ni), item_ids.repeat(k), item_feats.repeat(k, 1), item_dur.repeat(k)).view(k, ni)
        lo, hi = torch.aminmax(pred)
        return pred, torch.stack([lo, hi])

    def normed_reward(self, user_ids, item_ids, item_feats, item_dur):
        """KuaishouEnv.compute_normed_reward: float64 (pred - min) / (max - min) over all users x items."""
        pred, mm = self.sweep(user_ids, item_ids, item_feats, item_dur)
        out = torch.empty(pred.shape, dtype=torch.float64, device=self.device)
        abi.check(self._lib.cirs_normed_reward(pred.data_ptr(), pred.numel(), mm.data_ptr(), out.data_ptr(),
                                               torch.cuda.current_stream(self.device).cuda_stream), "cirs_normed_reward")
        return out
