"""Wall time of one VirtualTaobao PPO collect + update under the exact-redraw tracker dropout (dropout_redraw=True) in the script's shape
(max_turn 50, D 27, 3 heads, d_hid 128, 2 layers, Net (64, 64), dropout 0.1, batch 2048, repeat 2), in one process against the two paths
it sits between: the position-keyed device mode and the host path (HostCollector + HostPPOPolicy over the device env, which redraws
with torch's generator).

    python tools/probe_vtb_redraw.py [--sizes 100,1024] [--host-sizes 100] [--kinds simulated,raw] [--reps 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -- python tools/probe_vtb_redraw.py --kernels-only

One JSON line per (mode, kind, n_env): median collect_ms and update_ms of `reps` rounds after one warm-up round, with a device sync
around each timed call.  --kernels-only runs redraw rounds at the largest size only."""
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
N, THR, T, BATCH, REPEAT = 5, 3.0, 50, 2048, 2


def _setup(n, simulated, mode):
    from core.collector import Collector
    from core.policy.ppo import PPOPolicy
    from tianshou.data import VectorReplayBuffer
    from torch.distributions import Independent, Normal
    env, base = case.venv(GOLDEN, n, simulated, T, n_leave=N, thr=THR)
    tracker, actor, critic, policy = case.stack(base, n, T, dropout=0.1)
    kw = {}
    if mode != "host":
        policy = PPOPolicy(actor, critic, policy.optim, lambda *lg: Independent(Normal(*lg), 1), discount_factor=0.95, max_grad_norm=0.5,
                           eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, reward_normalization=1, advantage_normalization=1, value_clip=1,
                           gae_lambda=0.95, action_space=base.action_space, learner="device")
        kw = dict(rollout="device", dropout_redraw=mode == "redraw")
    env.seed(1)
    return Collector(policy, env, VectorReplayBuffer(n * T, n), preprocess_fn=tracker.build_state, **kw), policy


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def probe(n, simulated, mode, reps):
    c, policy = _setup(n, simulated, mode)
    col, upd = [], []
    for r in range(reps + 1):
        res, tc = _timed(lambda: c.collect(n_episode=n))
        _, tu = _timed(lambda: policy.update(0, c.buffer, batch_size=BATCH, repeat=REPEAT))
        if r:
            col.append(tc)
            upd.append(tu)
    return dict(mode=mode, kind="simulated" if simulated else "raw", n_env=n, rows=int(res["n/st"]), collect_ms=float(np.median(col)),
                update_ms=float(np.median(upd)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1024")
    ap.add_argument("--host-sizes", default="100")
    ap.add_argument("--kinds", default="simulated,raw")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    plan = [("redraw", sizes[-1:])] if a.kernels_only else [("redraw", sizes), ("keyed", sizes),
                                                            ("host", [int(x) for x in a.host_sizes.split(",") if x])]
    lines = []
    for kind in a.kinds.split(","):
        for mode, ns in plan:
            for n in ns:
                lines.append(probe(n, kind == "simulated", mode, a.reps))
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
