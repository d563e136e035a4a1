"""Device training and evaluation of the DICE debiasing baseline (csrc/dice_train.hip: cirs_dice_train_epoch, cirs_dice_forward).

Host-side counterpart of fit_data's inner loop (reference core/user_model.py:150-170) for UserModel_DICE (core/user_model_DICE.py,
loss_kuaishou_DICE of DICE.py:273-286): parameters, gradients and the Adam moments live in ONE flat fp32 device buffer each; named
views follow the reference's state_dict.  DeviceDice is the evaluation side (forward / sweep) over the same flat layout."""
import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import abi

TABLES = (("user_int", "U"), ("user_con", "U"), ("photo_int", "I"), ("photo_con", "I"), ("feat", "F"))
LOSS_COLUMNS = ("loss", "loss_y", "bpr_click", "bpr_con", "bpr_int", "reg")


# (state_dict name, shape) in buffer order -- must match dice_layout() in csrc/dice_train.hip
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


def _cfg_of(sd):
    U, E = sd["embedding_dict.user_int.weight"].shape
    I = sd["embedding_dict.photo_int.weight"].shape[0]
    F = sd["embedding_dict.feat.weight"].shape[0]
    if E not in (8, 16, 32):
        raise ValueError(f"the DICE device model takes an embedding size of 8, 16 or 32, got {E}")
    if tuple(sd["dnn_main.linears.0.weight"].shape) != (64, 8 * E + 1) or tuple(sd["dnn_ui.linears.0.weight"].shape) != (64, 2 * E):
        raise ValueError("the DICE device model takes dnn_hidden_units == (64, 64) and entity_dim == feature_dim")
    return abi.DiceCfg(n_user_vocab=U, n_item_vocab=I, n_feat_vocab=F, emb_dim=E, hidden=64), (U, I, F, E)


def _flatten(state_dict, device):
    """-> (cfg, flat fp32 device buffer, {name: view})."""
    sd = {k: torch.as_tensor(v) for k, v in state_dict.items()}
    cfg, (U, I, F, E) = _cfg_of(sd)
    total = abi.lib().cirs_dice_train_param_count(C.byref(cfg))
    flat = torch.zeros(total, dtype=torch.float32, device=device)
    views, off = {}, 0
    for name, shape in layout(U, I, F, E):
        n = int(np.prod(shape))
        views[name] = flat[off:off + n].view(shape)
        if not name.startswith("linear_model.") or name in sd:       # the unused copy may be absent from a hand-made dict
            views[name].copy_(sd[name].to(device, torch.float32).reshape(shape))
        off += n
    assert off == total
    return cfg, flat, views


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


class DiceTrainer:
    def __init__(self, state_dict: Dict[str, torch.Tensor], *, l2_embedding=1e-5, l2_linear=1e-5, l2_all=1e-1, lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, device="cuda"):
        self.device = torch.device(device)
        self._lib = abi.lib()
        self.cfg, self.flat, self.views = _flatten(state_dict, self.device)
        self.grads = torch.zeros_like(self.flat)
        self.adam_m = torch.zeros_like(self.flat)
        self.adam_v = torch.zeros_like(self.flat)
        self.step_count = 0
        self.l2 = (float(l2_embedding), float(l2_linear), float(l2_all))
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self._ws = None
        self._data = None
        self.loss = torch.zeros(6, dtype=torch.float32, device=self.device)

    def state_dict(self):
        return {k: v.clone() for k, v in self.views.items()}

    def _workspace(self, n):
        need = self._lib.cirs_dice_train_workspace_bytes(C.byref(self.cfg), n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _check_ids(self, cols):
        """The kernels index the tables with the data set's ids as they are: one range check per data set, in front of the passes."""
        c = self.cfg
        for what, ts, hi in (("user", (cols[0], cols[1]), c.n_user_vocab), ("photo", (cols[2], cols[3], cols[6], cols[7]), c.n_item_vocab),
                             ("feat", (cols[4], cols[8]), c.n_feat_vocab)):
            for t in ts:
                lo, up = torch.aminmax(t)
                if int(lo) < 0 or int(up) >= hi:
                    raise IndexError(f"{what} ids outside [0, {hi})")

    def _run_epoch(self, cols, n_rows, order, n_order, batch_size):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        if n_rows < 1 or n_order < 1:
            raise ValueError("empty data set or index array")
        steps = (n_order + batch_size - 1) // batch_size
        losses = torch.zeros(steps, 6, dtype=torch.float32, device=self.device)
        ws = self._workspace(min(int(batch_size), n_order))
        abi.check(self._lib.cirs_dice_train_epoch(
            C.byref(self.cfg), self.flat.data_ptr(), self.grads.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.step_count,
            *[c.data_ptr() for c in cols], n_rows, abi.ptr(order), n_order, int(batch_size), *self.l2, self.lr, self.betas[0], self.betas[1],
            self.eps, losses.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream), "cirs_dice_train_epoch")
        self.step_count += steps
        return losses

    def validate(self, valset, want_pred=False, want_sums=True):
        """The validation pass (cirs_dice_validate) of the LIVE parameters over a cirs_hip.userval.ValSet -> (pred or None, sums or None)."""
        from .userval import dice_validate
        return dice_validate(self.cfg, self.flat, valset, want_pred, want_sums)

    def step(self, x, y, score):
        """One optimiser step on the batch x [n,16], y, score [n] or [n,1] (a pass of one batch over these rows).  Returns the device loss
        vector {loss, loss_y, bpr_click, bpr_con, bpr_int, reg}."""
        cols = split_columns(x, y, score, self.device)
        self._check_ids(cols)
        n = cols[0].numel()
        self.loss.copy_(self._run_epoch(cols, n, None, n, n)[0])
        return self.loss

    def load(self, x, y, score):
        """Make the data set resident on the device in the column form of the kernels (the split runs once); epoch() trains on it."""
        cols = split_columns(x, y, score, self.device)
        self._check_ids(cols)
        self._data = cols
        return cols[0].numel()

    def epoch(self, order, batch_size, check=True):
        """One pass over the loaded data set from one call: batch b is the rows order[b * batch_size : (b + 1) * batch_size] (int64 indices
        into the data set; None = every row in file order), the last batch short.  Returns the [steps, 6] device tensor of per-step
        {loss, loss_y, bpr_click, bpr_con, bpr_int, reg}.  check=False skips the range check of `order` (one read-back in front of the
        pass) for a caller that built the permutation itself; the kernel answers an index outside the data set with a NaN loss, not a
        read."""
        assert self._data is not None, "call load(x, y, score) first"
        n_rows = self._data[0].numel()
        if order is None:
            return self._run_epoch(self._data, n_rows, None, n_rows, batch_size)
        order = torch.as_tensor(order).to(self.device, torch.int64).reshape(-1).contiguous()
        if check and order.numel():
            lo, hi = torch.aminmax(order)
            if int(lo) < 0 or int(hi) >= n_rows:
                raise IndexError(f"order holds row indices outside [0, {n_rows})")
        return self._run_epoch(self._data, n_rows, order, order.numel(), batch_size)


class DeviceDice:
    """UserModel_DICE.forward on the device: the interface of cirs_hip.deepfm.DeviceDeepFM that UserModel.recommend_k_item,
    evaluation.interactive_evaluation and KuaishouEnv.compute_normed_reward call."""
    PAIRS_PER_CALL = 1 << 22

    def __init__(self, state_dict, device="cuda"):
        self.device = torch.device(device)
        self._lib = abi.lib()
        self.cfg, self.flat, self.views = _flatten(state_dict, self.device)

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
