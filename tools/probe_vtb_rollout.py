"""Wall time of one VirtualTaobao PPO collect, `collect(n_episode=n_env)`, in the script's shape (max_turn 50, D = 27, nhead 3, d_hid 128,
2 layers, dim_state 20, Net (64, 64), dropout 0.1), both env kinds.

    python tools/probe_vtb_rollout.py [--device-sizes 4,100,1024] [--host-sizes 4,100] [--loop-sizes 4] [--reps 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -- python tools/probe_vtb_rollout.py --kernels-only

One JSON line per (path, kind, n_env):
  device   Collector(..., rollout="device") with a training buffer: collect_ms = the whole collect (device rollout + host rebuild of the
           states with autograd + buffer fill), rollout_ms = cirs_vtb_rollout_collect alone (two launches per vector step, one sync)
  hostdev  HostCollector on DummyVectorEnv(..., device="cuda"): the per-step host loop over the device env
  host     HostCollector on the host-mode DummyVectorEnv (no device)
--kernels-only runs only device rollouts at the largest size, so that the kernel trace holds nothing else."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cirs-codes_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtbrolloutcase as case  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N, THR, T = 5, 3.0, 50           # CIRS-RL-taobao.py defaults


def _setup(n, simulated, device, rollout):
    from core.collector import Collector
    from tianshou.data import VectorReplayBuffer
    env, base = case.venv(GOLDEN, n, simulated, T, device=device, n_leave=N, thr=THR)
    tracker, actor, critic, policy = case.stack(base, n, T, dropout=0.1)
    env.seed(1)
    kw = dict(rollout="device") if rollout else {}
    return Collector(policy, env, VectorReplayBuffer(n * T, n), preprocess_fn=tracker.build_state, **kw)


def _time(fn, reps):
    fn()      # warm-up (first launch, pinned buffers, allocator)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-sizes", default="4,100,1024")
    ap.add_argument("--host-sizes", default="4,100")
    ap.add_argument("--loop-sizes", default="4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(x) for x in a.device_sizes.split(",") if x]
    rows = []
    for simulated in (True, False):
        kind = "simulated" if simulated else "raw"
        for n in sizes[-1:] if a.kernels_only else sizes:
            c = _setup(n, simulated, "cuda", True)
            res = {}

            def one():
                res.update(c.collect(n_episode=n))
            ms = _time(one, a.reps)
            ro = c.rollout()
            rms = _time(lambda: ro.collect(*c.keys(0)[:1], 0, dropout_seed=c.keys(0)[1]), a.reps)
            rows.append(dict(path="device", kind=kind, n_env=n, collect_ms=round(ms, 3), rollout_ms=round(rms, 3), steps=int(res["n/st"]),
                             max_len=int(res["lens"].max())))
            print(json.dumps(rows[-1]), flush=True)
        if a.kernels_only:
            continue
        for path, dev, ns in (("hostdev", "cuda", a.host_sizes), ("host", None, a.loop_sizes)):
            for n in [int(x) for x in ns.split(",") if x]:
                c = _setup(n, simulated, dev, False)
                res = {}

                def one():
                    res.update(c.collect(n_episode=n))
                ms = _time(one, 1)
                rows.append(dict(path=path, kind=kind, n_env=n, collect_ms=round(ms, 3), steps=int(res["n/st"]), max_len=int(res["lens"].max())))
                print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
