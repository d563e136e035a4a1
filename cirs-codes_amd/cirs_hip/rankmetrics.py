"""Ranking and list-diversity metrics of top-k lists on the device (csrc/rankmetrics.hip: cirs_rows_topk, cirs_rank_metrics).

The ground truth is a fully observed user x item matrix (KuaishouEnv.mat, DeviceEnvTables.mat); a list comes from the RL policy
(DevicePolicy.topk) or from a score table of a static model (DeviceDeepFM.sweep / DeviceDice.sweep -> RankMetrics.topk_rows).  No reference
counterpart.  cirs_hip/rankmetrics_host.py restates every number in float64 numpy, in the same summation orders."""
import ctypes as C

import numpy as np
import torch

from . import abi
from .evalmetrics import CoverageCounter
from .rankmetrics_host import discounts

METRIC_NAMES = ("Precision", "Recall", "HR", "MRR", "NDCG", "ILD")       # sums[2:8]


def check_k(k):
    if not isinstance(k, (int, np.integer)) or not 1 <= k <= abi.TOPK_MAX:
        raise ValueError(f"k must lie in 1..{abi.TOPK_MAX}, got {k!r}")
    return int(k)


def _rows(n, **named):
    for name, t in named.items():
        if t is not None and t.shape[0] != n:
            raise ValueError(f"{name} has {t.shape[0]} rows, expected {n}")


class RankMetrics:
    """rel: float64 [U, I] relevance (a DeviceEnvTables.mat tensor is used as it is, without a copy); item_cats: the packed uint32 categories
    (DeviceEnvTables.item_cats) or an [I, 4] int table (-1 = none).  rel_threshold: an item is relevant iff rel >= rel_threshold."""

    def __init__(self, rel, item_cats, *, rel_threshold=None, device="cuda"):
        if rel_threshold is None:       # no default on purpose: the caller says what counts as relevant
            raise ValueError("rel_threshold is required: an item is relevant iff rel >= rel_threshold")
        self.device = torch.device(device)
        self.rel_threshold = float(rel_threshold)
        if isinstance(rel, torch.Tensor) and rel.dtype == torch.float64 and rel.device.type == self.device.type and rel.dim() == 2 \
                and rel.stride(1) == 1:
            self.rel = rel
        else:
            self.rel = torch.as_tensor(np.ascontiguousarray(np.asarray(rel.cpu() if isinstance(rel, torch.Tensor) else rel, np.float64))).to(self.device)
        self.n_users, self.n_items = self.rel.shape
        if isinstance(item_cats, torch.Tensor) and item_cats.dim() == 1:
            cats = item_cats.to(self.device, torch.int32).contiguous()
        else:
            from .synthetic import pack_item_cats
            c = np.asarray(item_cats.cpu() if isinstance(item_cats, torch.Tensor) else item_cats)
            cats = torch.as_tensor(np.ascontiguousarray(c if c.ndim == 1 else pack_item_cats(c)).view(np.int32)).to(self.device)
        if cats.numel() != self.n_items:
            raise ValueError(f"item_cats has {cats.numel()} items, rel has {self.n_items} columns")
        self.item_cats = cats
        self._disc = discounts(abi.TOPK_MAX)
        self._scratch = {}          # n -> (sums, workspace)
        self._coverage = None
        self._lib = abi.lib()

    @classmethod
    def for_env(cls, env, *, rel_threshold=None, device="cuda"):
        """Against the ground truth of a KuaishouEnv: its mat and item categories, resident once per table set (KuaishouEnv.device_tables)."""
        if rel_threshold is None:
            raise ValueError("rel_threshold is required: an item is relevant iff rel >= rel_threshold")
        tab = env.device_tables(device=device)
        return cls(tab.mat, tab.item_cats, rel_threshold=rel_threshold, device=device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _mask_args(self, n, visited, env_ids, skip):
        dev = self.device
        if visited is not None:
            visited = visited.to(dev).contiguous()
            if visited.dim() != 2 or visited.shape[1] != (self.n_items + 31) // 32 or visited.element_size() != 4:
                raise ValueError("visited must be a 32-bit bitmap [rows, ceil(n_items / 32)]")
            if env_ids is None and visited.shape[0] < n:
                raise ValueError(f"visited has {visited.shape[0]} rows, expected {n}")
        env_ids = None if env_ids is None or visited is None else torch.as_tensor(env_ids).to(dev, torch.int32).contiguous()
        skip = None if skip is None else torch.as_tensor(skip).to(dev, torch.uint8).contiguous()
        _rows(n, env_ids=env_ids, skip=skip)
        return visited, env_ids, skip

    def topk_rows(self, scores, k, visited=None, env_ids=None, skip=None):
        """scores: fp32 [n, >= n_items] on the device, rows contiguous (a column slice of a wider table is read in place) -> (ids [n, k] int64,
        vals [n, k] fp32): value descending, ties to the lower id; -inf, NaN and masked entries are never listed; fills are -1 / -inf."""
        k = check_k(k)
        if scores.dim() != 2 or scores.dtype != torch.float32 or scores.shape[1] < self.n_items:
            raise ValueError(f"scores must be float32 [n, >= {self.n_items}], got {tuple(scores.shape)} {scores.dtype}")
        scores = scores.to(self.device)
        if scores.stride(1) != 1:
            scores = scores.contiguous()
        n = scores.shape[0]
        visited, env_ids, skip = self._mask_args(n, visited, env_ids, skip)
        ids = torch.empty((n, k), dtype=torch.int64, device=self.device)
        vals = torch.empty((n, k), dtype=torch.float32, device=self.device)
        abi.check(self._lib.cirs_rows_topk(scores.data_ptr(), n, self.n_items, scores.stride(0) if n > 1 else scores.shape[1], k, abi.ptr(env_ids),
                                           abi.ptr(visited), abi.ptr(skip), ids.data_ptr(), vals.data_ptr(), self._stream()), "cirs_rows_topk")
        return ids, vals

    def evaluate(self, ids, users, visited=None, env_ids=None, skip=None, k=None):
        """ids int64 [n, >= k] (-1 = fill), users [n] rows of rel -> {"Precision@k", "Recall@k", "HR@k", "MRR@k", "NDCG@k", "ILD@k": means over the
        rows not skipped, "CV@k": share of the catalogue in any scored list, "n": rows not skipped, "per_row": float64 [n, 11] device tensor in
        abi.RANK_COLUMNS order}.  k defaults to ids.shape[1]; a smaller k scores the prefix of every list in place.  One read-back."""
        if ids.dim() != 2 or ids.dtype != torch.int64:
            raise ValueError("ids must be int64 [n, k]")
        k = check_k(ids.shape[1] if k is None else k)
        if k > ids.shape[1]:
            raise ValueError(f"k = {k} exceeds the list length {ids.shape[1]}")
        ids = ids.to(self.device)
        if ids.stride(1) != 1:
            ids = ids.contiguous()
        n = ids.shape[0]
        users = torch.as_tensor(users).to(self.device, torch.int32).contiguous().reshape(-1)
        _rows(n, users=users)
        visited, env_ids, skip = self._mask_args(n, visited, env_ids, skip)
        per_row = torch.empty((n, abi.RANK_NCOL), dtype=torch.float64, device=self.device)
        if n == 0:
            return dict({f"{m}@{k}": 0.0 for m in METRIC_NAMES}, **{f"CV@{k}": 0.0, "n": 0, "per_row": per_row})
        if n not in self._scratch:
            self._scratch[n] = (torch.empty(abi.RANK_NSUM, dtype=torch.float64, device=self.device),
                                torch.empty(self._lib.cirs_rank_metrics_workspace_bytes(n), dtype=torch.uint8, device=self.device))
        sums, ws = self._scratch[n]
        cfg = abi.RankCfg(n_users=self.n_users, n_items=self.n_items, k=k, rel_threshold=self.rel_threshold,
                          discount=(C.c_double * abi.TOPK_MAX)(*self._disc.tolist()))
        abi.check(self._lib.cirs_rank_metrics(C.byref(cfg), ids.data_ptr(), ids.stride(0) if n > 1 else ids.shape[1], users.data_ptr(), n,
                                              self.rel.data_ptr(), self.rel.stride(0), self.item_cats.data_ptr(), abi.ptr(env_ids), abi.ptr(visited),
                                              abi.ptr(skip), per_row.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                  "cirs_rank_metrics")
        # CV@k: the existing coverage count over the scored prefixes (ids out of range and the lists of skipped rows do not count)
        if self._coverage is None:
            self._coverage = CoverageCounter(self.n_items, device=self.device)
        cc = self._coverage
        lists = ids[:, :k] if skip is None else ids[:, :k].masked_fill(skip.bool()[:, None], -1)
        lists = lists.contiguous()
        abi.check(self._lib.cirs_eval_coverage(lists.data_ptr(), lists.numel(), self.n_items, None, cc.bitmap.data_ptr(), cc.out.data_ptr(),
                                               self._stream()), "cirs_eval_coverage")
        host = torch.cat([sums, cc.out.double()]).cpu().numpy()          # the one read-back
        word = int(host[1])
        if word:
            what = [s for bit, s in ((abi.RANK_ERR_ID, f"a list id outside [-1, {self.n_items})"),
                                     (abi.RANK_ERR_USER, f"a user outside [0, {self.n_users})")) if word & bit]
            exc = ValueError("cirs_rank_metrics: " + " and ".join(what) + " (such rows are zero in per_row)")
            exc.per_row = per_row
            raise exc
        out = {f"{m}@{k}": float(host[2 + q]) for q, m in enumerate(METRIC_NAMES)}
        out[f"CV@{k}"] = float(host[abi.RANK_NSUM]) / self.n_items
        out["n"] = int(host[0])
        out["per_row"] = per_row
        return out
