"""Dataset preparation of the user-model training on the device (csrc/dataprep.hip).

Host-side counterpart of reference core/util.py:56-76,135-196 (compute_exposure_effect_kuaishouRec / compute_exposure_each_user,
negative_sampling / find_negative) and of the score columns of the two debiasing baselines (compute_IPS_kuaishouRec,
DeepFM-IPS-pairwise.py:79-86; compute_popularity_kuaishouRec_pairwise, PD-pairwise.py:76-108)."""
from typing import Optional

import numpy as np
import torch

from . import abi
from .synthetic import pack_item_cats


def exposure_history(user_id, photo_id, timestamp, tau: float, *, dist: Optional[np.ndarray] = None, list_feat=None, device="cuda"):
    """exposure_pos [n_rows] float64 of every logged interaction (rows in file order, a user's rows contiguous).
    Pass either the distance table `dist` (1 / similarity, [n_items, n_items]) or `list_feat` (category lists per item id)."""
    user_id = np.asarray(user_id); n = len(user_id)
    # first row of each row's user (df_user.index[0], util.py:158): rows of a user are contiguous in the log
    change = np.r_[True, user_id[1:] != user_id[:-1]]
    start = np.maximum.accumulate(np.where(change, np.arange(n), 0)).astype(np.int64)
    dev = torch.device(device)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dev, dt).contiguous()
    start_d, photo_d, ts_d = t(start, torch.int64), t(np.asarray(photo_id), torch.int32), t(np.asarray(timestamp, np.float64), torch.float64)
    out = torch.zeros(n, dtype=torch.float64, device=dev)
    dist_d = cats_d = None
    if dist is not None:
        dist_d = t(np.asarray(dist, np.float64), torch.float64)
        n_items = dist_d.shape[0]
    else:
        cats = np.full((len(list_feat), 4), -1, np.int32)
        for i, f in enumerate(list_feat):
            cats[i, :len(f)] = sorted(set(int(c) for c in f))
        cats_d = torch.as_tensor(np.ascontiguousarray(pack_item_cats(cats)).view(np.int32)).to(dev)
        n_items = len(list_feat)
    abi.check(abi.lib().cirs_exposure_history(start_d.data_ptr(), photo_d.data_ptr(), ts_d.data_ptr(), n, abi.ptr(dist_d), abi.ptr(cats_d),
                                              n_items, float(tau), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
              "cirs_exposure_history")
    return out


def bitmap_rows(mat_bool: np.ndarray) -> np.ndarray:
    """[n_users, n_items] bool -> [n_users, ceil(n_items/32)] uint32 (bit i of word i>>5)"""
    n_u, n_i = mat_bool.shape
    padded = np.zeros((n_u, ((n_i + 31) // 32) * 32), dtype=bool)
    padded[:, :n_i] = mat_bool
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32)


def find_negative(user_ids, photo_ids, seen_small_bits, seen_big_bits, n_items: int, absent_id: int = 1225, device="cuda"):
    """negative item per (user, positive item) row; seen_*_bits: bitmap_rows() of the two interaction matrices."""
    dev = torch.device(device)
    u = torch.as_tensor(np.asarray(user_ids)).to(dev, torch.int64).contiguous()
    p = torch.as_tensor(np.asarray(photo_ids)).to(dev, torch.int64).contiguous()
    a = torch.as_tensor(np.ascontiguousarray(seen_small_bits).view(np.int32)).to(dev).contiguous()
    b = torch.as_tensor(np.ascontiguousarray(seen_big_bits).view(np.int32)).to(dev).contiguous()
    out = torch.empty_like(u)
    abi.check(abi.lib().cirs_find_negative(u.data_ptr(), p.data_ptr(), u.numel(), a.data_ptr(), b.data_ptr(), int(n_items), int(absent_id),
                                           out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cirs_find_negative")
    return out


# ---- score columns of the debiasing baselines: item counts per time bin on the device, the float arithmetic on the host ----------
def time_bin_bounds(time_min, time_max, num_bin):
    """The num_bin + 1 bin bounds in the reference's own float64 expression `interval * i + time_min` (PD-pairwise.py:82-84)."""
    time_min, time_max = np.float64(time_min), np.float64(time_max)
    interval = (time_max - time_min) / num_bin
    return np.array([interval * i + time_min for i in range(num_bin + 1)], dtype=np.float64)


def ips_table(counts):
    """counts [1, n_items] -> the inverse-propensity weight of every item: 1.0 / max(count, 1) (DeepFM-IPS-pairwise.py:82-83)."""
    c = np.asarray(counts, np.int64).copy()
    c[c < 1] = 1
    return 1.0 / c


def popularity_table(counts, gamma):
    """counts [num_bin, n_items] -> (count / total of the bin) ** gamma (PD-pairwise.py:100-106); an empty bin keeps 0."""
    c = np.asarray(counts, np.int64)
    total = c.sum(axis=1, keepdims=True)
    pop = np.zeros(c.shape, np.float64)
    np.divide(c, total, out=pop, where=total > 0)
    return pop ** gamma


def item_bin_counts(photo_id, timestamp=None, bounds=None, n_items=None, device="cuda"):
    """-> (photo [n] int32, bin [n] int32, counts [num_bin, n_items] int32), all on the device (cirs_item_bin_counts)."""
    dev = torch.device(device)
    photo = torch.as_tensor(np.ascontiguousarray(np.asarray(photo_id))).to(dev, torch.int32).reshape(-1).contiguous()
    n = photo.numel()
    n_items = (int(photo.max()) + 1 if n else 1) if n_items is None else int(n_items)
    ts_d = bounds_d = None
    num_bin = 1
    if timestamp is not None:
        ts_d = torch.as_tensor(np.ascontiguousarray(np.asarray(timestamp, np.float64))).to(dev).reshape(-1).contiguous()
        assert ts_d.numel() == n, "one timestamp per row"
        bounds_d = torch.as_tensor(np.ascontiguousarray(np.asarray(bounds, np.float64))).to(dev).contiguous()
        num_bin = bounds_d.numel() - 1
    bins = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(num_bin, n_items, dtype=torch.int32, device=dev)
    abi.check(abi.lib().cirs_item_bin_counts(photo.data_ptr(), abi.ptr(ts_d), n, abi.ptr(bounds_d), num_bin, n_items, bins.data_ptr(),
                                             counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cirs_item_bin_counts")
    return photo, bins, counts


def item_bin_gather(photo, bins, table):
    """out[r] = table[bins[r], photo[r]] in float64, 0 where bins[r] < 0 (cirs_item_bin_gather); photo / bins from item_bin_counts."""
    dev = photo.device
    table_d = torch.as_tensor(np.ascontiguousarray(np.asarray(table, np.float64))).to(dev).contiguous()
    out = torch.empty(photo.numel(), dtype=torch.float64, device=dev)
    abi.check(abi.lib().cirs_item_bin_gather(photo.data_ptr(), bins.data_ptr(), photo.numel(), table_d.data_ptr(), table_d.shape[0],
                                             table_d.shape[1], out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cirs_item_bin_gather")
    return out


def ips_scores(photo_id, device="cuda"):
    """compute_IPS_kuaishouRec: 1 / (number of log rows with this row's item) per row -> [n, 1] float64 numpy."""
    photo, bins, counts = item_bin_counts(photo_id, device=device)
    return item_bin_gather(photo, bins, ips_table(counts.cpu().numpy())).cpu().numpy().reshape(-1, 1)


def popularity_scores(photo_id, timestamp, gamma, num_bin=5, device="cuda"):
    """compute_popularity_kuaishouRec_pairwise: (share of this row's item among the log rows of this row's time bin) ** gamma per row
    -> [n, 1] float64 numpy; a row that no bin takes (rounding at time_max) keeps the reference's 0 ** gamma."""
    ts = np.asarray(timestamp, np.float64).reshape(-1)
    bounds = time_bin_bounds(ts.min(), ts.max(), num_bin)
    photo, bins, counts = item_bin_counts(photo_id, ts, bounds, device=device)
    out = item_bin_gather(photo, bins, popularity_table(counts.cpu().numpy(), gamma)).cpu().numpy().reshape(-1, 1)
    if gamma == 0:      # 0 ** 0 == 1 in the reference for a row outside every bin
        out[bins.cpu().numpy() < 0] = 1.0
    return out
