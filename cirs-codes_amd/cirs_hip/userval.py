"""Validation pass of the Kuaishou user models on the device (csrc/userval.hip: cirs_deepfm_validate, cirs_dice_validate).

Counterpart of evaluate_data / predict_data (reference core/user_model.py:351-399): the validation set is made resident once in the
column form of the kernels (ValSet), one call scores every row and reduces the errors against y to {sum |e|, sum e^2} in float64.
DeviceDeepFM.validate / DeviceDice.validate run it over a model's weights, DeepFMTrainer.validate / DiceTrainer.validate over a
trainer's live parameters (no publish needed for the numbers)."""
import ctypes as C

import numpy as np
import torch

from . import abi

DEVICE_METRICS = ("mae", "mse")      # index into the fused sums: sums[i] / n


class ValSet:
    """x [n,7] = [user_id, photo_id, feat0..3, photo_duration], y [n] or [n,1] -> device columns (uid, pid int64; feats [n,4] int32;
    dur fp32; y float64).  Every id column is checked against its vocabulary of `cfg` (abi.DeepFMCfg / abi.DiceCfg) once, on the host,
    before anything is copied or launched: the kernel indexes the tables with the ids as they are."""

    def __init__(self, x, y, cfg, device="cuda"):
        x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
        if x.ndim != 2 or x.shape[1] != 7:
            raise ValueError("x must have the 7 columns [user_id, photo_id, feat0..3, photo_duration]")
        n = x.shape[0]
        if n < 1:
            raise ValueError("empty validation set")
        ids = x[:, :6].astype(np.int64)
        for what, cols, hi in (("user", ids[:, 0:1], cfg.n_user_vocab), ("photo", ids[:, 1:2], cfg.n_item_vocab), ("feat", ids[:, 2:6], cfg.n_feat_vocab)):
            if int(cols.min()) < 0 or int(cols.max()) >= hi:
                raise IndexError(f"{what} ids outside [0, {hi})")
        self.n = n
        self.vocab = (cfg.n_user_vocab, cfg.n_item_vocab, cfg.n_feat_vocab)
        self.device = torch.device(device)
        dev = self.device
        self.uid = torch.as_tensor(np.ascontiguousarray(ids[:, 0])).to(dev)
        self.pid = torch.as_tensor(np.ascontiguousarray(ids[:, 1])).to(dev)
        self.feats = torch.as_tensor(np.ascontiguousarray(ids[:, 2:6].astype(np.int32))).to(dev)
        self.dur = torch.as_tensor(np.ascontiguousarray(x[:, 6].astype(np.float32))).to(dev)
        self.y = None
        if y is not None:
            y = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, dtype=np.float64).reshape(-1)
            if y.shape[0] != n:
                raise ValueError("x and y must have one row per sample")
            self.y = torch.as_tensor(np.ascontiguousarray(y)).to(dev)
        self._ws = None

    def check_vocab(self, cfg):
        if (cfg.n_user_vocab, cfg.n_item_vocab, cfg.n_feat_vocab) != self.vocab:
            raise ValueError("the validation set was checked against other vocabulary sizes than this model's")


def run(entry, ws_entry, cfg, weights_arg, vs: ValSet, want_pred, want_sums=True):
    """One call of cirs_deepfm_validate / cirs_dice_validate -> (pred [n] fp32 or None, sums float64 [2] on the device or None)."""
    lib = abi.lib()
    vs.check_vocab(cfg)
    if not (want_pred or want_sums):
        raise ValueError("ask for the predictions, the sums or both")
    if want_sums and vs.y is None:
        raise ValueError("the error sums need a validation set with y")
    dev = vs.device
    pred = torch.empty(vs.n, dtype=torch.float32, device=dev) if want_pred else None
    sums = torch.empty(2, dtype=torch.float64, device=dev) if want_sums else None
    if want_sums and vs._ws is None:
        vs._ws = torch.empty(getattr(lib, ws_entry)(C.byref(cfg), vs.n), dtype=torch.uint8, device=dev)
    ws = vs._ws if want_sums else None
    abi.check(getattr(lib, entry)(C.byref(cfg), weights_arg, vs.uid.data_ptr(), vs.pid.data_ptr(), vs.feats.data_ptr(), vs.dur.data_ptr(),
                                  abi.ptr(vs.y) if want_sums else None, vs.n, abi.ptr(pred), abi.ptr(sums), abi.ptr(ws),
                                  ws.numel() if ws is not None else 0, torch.cuda.current_stream(dev).cuda_stream), entry)
    return pred, sums


def deepfm_validate(cfg, w, vs, want_pred=False, want_sums=True):
    return run("cirs_deepfm_validate", "cirs_deepfm_validate_workspace_bytes", cfg, C.byref(w), vs, want_pred, want_sums)


def dice_validate(cfg, flat, vs, want_pred=False, want_sums=True):
    return run("cirs_dice_validate", "cirs_dice_validate_workspace_bytes", cfg, flat.data_ptr(), vs, want_pred, want_sums)
