"""Wall time of one VirtualTaobao PPO collect + update in the script's shape (max_turn 50, batch 2048, repeat 2, dropout 0.1), both env
kinds, for the host learner (HostPPOPolicy over DeviceVtbCollector's torch rebuild) and the device learner (learner="device").

    python tools/probe_vtb_learn.py [--device-sizes 100,1024] [--host-sizes 100] [--reps 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -- python tools/probe_vtb_learn.py --kernels-only

One JSON line per (learner, kind, n_env): median collect_ms and update_ms of `reps` rounds after one warm-up round, with a device sync
around each timed call.  --kernels-only runs device-learner rounds at the largest size only."""
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


def _setup(n, simulated, learner):
    from core.collector import Collector
    from core.policy.ppo import PPOPolicy
    from tianshou.data import VectorReplayBuffer
    from torch.distributions import Independent, Normal
    env, base = case.venv(GOLDEN, n, simulated, T, n_leave=N, thr=THR)
    tracker, actor, critic, host = case.stack(base, n, T, dropout=0.1)
    policy = host
    if learner == "device":
        policy = PPOPolicy(actor, critic, host.optim, lambda *lg: Independent(Normal(*lg), 1), discount_factor=0.95, max_grad_norm=0.5,
                           eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, reward_normalization=1, advantage_normalization=1, value_clip=1,
                           gae_lambda=0.95, action_space=base.action_space, learner="device")
    env.seed(1)
    return Collector(policy, env, VectorReplayBuffer(n * T, n), preprocess_fn=tracker.build_state, rollout="device"), policy


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def probe(n, simulated, learner, reps):
    c, policy = _setup(n, simulated, learner)
    col, upd = [], []
    for r in range(reps + 1):
        res, tc = _timed(lambda: c.collect(n_episode=n))
        _, tu = _timed(lambda: policy.update(0, c.buffer, batch_size=BATCH, repeat=REPEAT))
        if r:
            col.append(tc)
            upd.append(tu)
    return dict(learner=learner, kind="simulated" if simulated else "raw", n_env=n, rows=int(res["n/st"]),
                collect_ms=float(np.median(col)), update_ms=float(np.median(upd)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-sizes", default="100,1024")
    ap.add_argument("--host-sizes", default="100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = [int(x) for x in a.device_sizes.split(",") if x]
    host = [] if a.kernels_only else [int(x) for x in a.host_sizes.split(",") if x]
    if a.kernels_only:
        dev = dev[-1:]
    lines = []
    for simulated in (True, False):
        for n in dev:
            lines.append(probe(n, simulated, "device", a.reps))
            print(json.dumps(lines[-1]), flush=True)
        for n in host:
            lines.append(probe(n, simulated, "host", a.reps))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
