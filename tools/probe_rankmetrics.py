"""Time of one evaluate_ranking-shaped pass, in three parts: a score table already on the device -> RankMetrics.topk_rows (cirs_rows_topk),
RankMetrics.evaluate (cirs_rank_metrics + the coverage count), and the read-back; k = 10 at 1411 x 3327 (all users of the small matrix) and at
7176 x 10728.    python tools/probe_rankmetrics.py [--reps 50] [--shapes small large] [--no-compare]

Timed with device events around `reps` repetitions after a warm-up of the same shape (the read-back: a host clock around the copy that ends in a
synchronise).  In the same call and alternating with them: the same metrics written with torch ops on the same GPU (torch.topk + gathers +
torch.sort for the ideal list) and, once, the numpy restatement (cirs_hip/rankmetrics_host.py) on 16 host threads.  Per kernel the bytes it must
read from shapes (n * I * 4 for the selection, n * I * 8 for the relevance pass) and, over the event time, their share of the 8 TB/s HBM peak --
an upper bound of the kernel's share, since the event window also holds the launch gaps.  Kernel times proper come from a run of their own:
    rocprofv3 --kernel-trace --stats -d <out> -- python tools/probe_rankmetrics.py --no-compare --reps 20
One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cirs_hip import abi, rankmetrics_host as host  # noqa: E402
from cirs_hip.rankmetrics import RankMetrics  # noqa: E402

SHAPES = {"small": (1411, 3327), "large": (7176, 10728)}
HBM_PEAK, CACHE_BYTES = 8.0e12, 256 << 20      # spec peak; the die-level cache (Infinity Cache) holds tables up to 256 MiB
K, REL_THRESHOLD, N_CATS = 10, 3.0, 31


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def torch_metrics(scores, rel, onehot, disc, k, thr):
    """The same metrics with torch ops (users = all rows in order): -> the six means."""
    ids = torch.topk(scores, k, dim=1).indices
    x = rel.gather(1, ids)
    hit = x >= thr
    hits = hit.sum(1).double()
    n_rel = (rel >= thr).sum(1).double()
    dcg = (x.clamp_min(0) * disc).sum(1)
    idcg = (torch.sort(rel.clamp_min(0), dim=1, descending=True).values[:, :k] * disc).sum(1)
    first = torch.where(hit.any(1), hit.double().argmax(1) + 1, torch.ones_like(ids[:, 0])).double()
    a = onehot[ids]                                        # [n, k, C]
    inter = a @ a.transpose(1, 2)
    size = a.sum(2)
    union = size[:, :, None] + size[:, None, :] - inter
    sim = torch.where(union > 0, inter / union.clamp_min(1), torch.zeros_like(inter))
    pair_sum = (sim.sum((1, 2)) - sim.diagonal(dim1=1, dim2=2).sum(1)) / 2
    cols = [hits / k, torch.where(n_rel > 0, hits / n_rel.clamp_min(1), n_rel * 0), hit.any(1).double(),
            torch.where(hit.any(1), 1.0 / first, first * 0), torch.where(idcg > 0, dcg / idcg.clamp_min(1e-300), idcg * 0),
            1.0 - pair_sum / (k * (k - 1) / 2)]
    return torch.stack([c.mean() for c in cols])


def numpy_metrics(scores, rel, packed, k, thr, threads=16):
    n = len(scores)
    blocks = [slice(s, min(n, s + (n + threads - 1) // threads)) for s in range(0, n, (n + threads - 1) // threads)]

    def one(b):
        ids, _ = host.topk_rows64(scores[b], k)
        return host.rank_metrics64(ids, np.arange(b.start, b.stop), rel, packed, k, thr)[0]
    with ThreadPoolExecutor(threads) as pool:
        return host.reduce64(np.concatenate(list(pool.map(one, blocks))))


def probe(name, reps, compare):
    n, I = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(11)
    scores = torch.randn((n, I), generator=g, device=dev)
    rel = torch.rand((n, I), generator=g, device=dev, dtype=torch.float64) * 5.0
    rng = np.random.RandomState(3)
    cats = np.where(np.arange(4)[None, :] < rng.randint(1, 5, I)[:, None], np.argsort(rng.uniform(size=(I, N_CATS)), axis=1)[:, :4], -1)
    rm = RankMetrics(rel, cats, rel_threshold=REL_THRESHOLD, device=dev)
    users = torch.arange(n, dtype=torch.int32, device=dev)
    lib, stream = abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    ids, _ = rm.topk_rows(scores, K)
    res = rm.evaluate(ids, users)                          # warm-up of the shape; allocates the scratch
    sums, ws = rm._scratch[n]
    per_row = res["per_row"]
    cfg = abi.RankCfg(n_users=n, n_items=I, k=K, rel_threshold=REL_THRESHOLD, discount=(C.c_double * abi.TOPK_MAX)(*host.discounts().tolist()))

    def rank_kernels():
        abi.check(lib.cirs_rank_metrics(C.byref(cfg), ids.data_ptr(), K, users.data_ptr(), n, rel.data_ptr(), I, rm.item_cats.data_ptr(), None, None,
                                        None, per_row.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), stream), "cirs_rank_metrics")

    def readback():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sums.cpu()
        return (time.perf_counter() - t0) * 1e3
    onehot = torch.zeros((I, N_CATS), dtype=torch.float64, device=dev)
    for q in range(4):
        ok = cats[:, q] >= 0
        onehot[torch.as_tensor(np.flatnonzero(ok)).to(dev), torch.as_tensor(cats[ok, q]).to(dev)] = 1.0
    disc = torch.as_tensor(host.discounts(K)).to(dev)
    out = {"shape": name, "n": n, "n_items": I, "k": K, "reps": reps}
    rounds = {"topk_rows_ms": [], "rank_metrics_ms": [], "evaluate_ms": [], "torch_ops_ms": []}
    if compare:
        torch_metrics(scores, rel, onehot, disc, K, REL_THRESHOLD)       # warm-up
    for _ in range(2):                                      # alternating: ours, torch, ours, torch
        rounds["topk_rows_ms"].append(events_ms(lambda: rm.topk_rows(scores, K), reps))
        rounds["rank_metrics_ms"].append(events_ms(rank_kernels, reps))
        rounds["evaluate_ms"].append(events_ms(lambda: rm.evaluate(ids, users), reps))
        if compare:
            rounds["torch_ops_ms"].append(events_ms(lambda: torch_metrics(scores, rel, onehot, disc, K, REL_THRESHOLD), max(3, reps // 10)))
    for key, v in rounds.items():
        if v:
            out[key] = [round(x, 4) for x in v]
    out["readback_ms"] = round(min(readback() for _ in range(reps)), 4)
    sel_bytes, rel_bytes = n * I * 4, n * I * 8
    out["selection_bytes"], out["relevance_bytes"] = sel_bytes, rel_bytes
    out["selection_share_of_hbm_peak"] = round(sel_bytes / (min(rounds["topk_rows_ms"]) * 1e-3) / HBM_PEAK, 4)
    out["relevance_share_of_hbm_peak"] = round(rel_bytes / (min(rounds["rank_metrics_ms"]) * 1e-3) / HBM_PEAK, 4)
    out["tables_fit_the_die_level_cache"] = bool(sel_bytes + rel_bytes <= CACHE_BYTES)
    if out["tables_fit_the_die_level_cache"]:
        out["note"] = "score and relevance tables sit in L2 / Infinity Cache between repetitions: the shares are not HBM traffic"
    if compare:
        t0 = time.perf_counter()
        want = numpy_metrics(scores.cpu().numpy(), rel.cpu().numpy(), rm.item_cats.cpu().numpy(), K, REL_THRESHOLD)
        out["numpy_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        got = np.array([res[f"{m}@{K}"] for m in ("Precision", "Recall", "HR", "MRR", "NDCG", "ILD")])
        out["means_match_numpy_restatement"] = bool(np.allclose(got, want[2:], rtol=1e-12, atol=0))
        out["means_close_to_torch_ops"] = bool(np.allclose(got, torch_metrics(scores, rel, onehot, disc, K, REL_THRESHOLD).cpu().numpy(), rtol=1e-9))
    out["metrics"] = {key: v for key, v in res.items() if key != "per_row"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-compare", action="store_true", help="skip the torch-op and numpy comparisons (for a profiler run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_rankmetrics needs the GPU: nothing is measured without one")
    for name in args.shapes:
        probe(name, args.reps, not args.no_compare)


if __name__ == "__main__":
    main()
