"""Timing of the batched device VirtualTaobao env (cirs_hip/virtualtb.py) against the host-mode loop, both env kinds.

    python tools/probe_vtb.py [--sizes 4,100,1024,8192] [--steps 50] [--host-cap 100] [--out FILE]

Per n_env and kind it prints one JSON line:
  plugin_us      wall time of one DummyVectorEnv(..., device="cuda").step, numpy in and out (one H2D, one launch, one packed D2H)
  engine_us      DeviceVirtualTB.step alone, timed with device events over `steps` back-to-back launches
  host_us        the host-mode loop (DummyVectorEnv without device) at the same n_env, only for n_env <= --host-cap
  speedup        host_us / plugin_us
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/probe_vtb.py --kernels-only` run; --kernels-only
runs the engine steps alone so that the trace holds nothing else.  FLOP counts are from the layer shapes, not measured:
~180 kFLOP per env-step (action model and MMoE) plus ~55 kFLOP per user redraw."""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cirs-codes_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N, THR, T = 5, 3.0, 50           # CIRS-RL-taobao.py defaults


def _register():
    from cirs_hip import gymlite
    gymlite.install()
    from gym.envs.registration import register
    import vtbcase
    model, _ = vtbcase.golden_mmoe(GOLDEN)
    register(id="VirtualTB-v0", entry_point="environments.VirtualTaobao.virtualTB.envs.virtualTB:VirtualTB",
             kwargs=dict(num_leave_compute=N, leave_threshold=THR, max_turn=T, data_dir=os.path.join(GOLDEN, "virtualtb")))
    register(id="SimulatedEnv-v0", entry_point="core.env.simulatedEnv.simulated_env:SimulatedEnv",
             kwargs=dict(user_model=model, task_name="VirtualTB-v0", version="v1", tau=10.0, gamma_exposure=3.0))


def _venv(name, n, device):
    import gym
    from tianshou.env import DummyVectorEnv
    return DummyVectorEnv([lambda: gym.make(name) for _ in range(n)], device=device)


def _time_vector(venv, n, steps, sim):
    """mean seconds per vector step; envs are reset every T - 1 steps so that the simulated kind never passes max_turn."""
    rng = np.random.RandomState(0)
    acts = rng.uniform(-1, 1, (steps, n, 27)).astype(np.float32)
    ids = np.arange(n)
    venv.reset()
    tot = 0.0
    for k in range(steps):
        if k and k % (T - 1) == 0:
            venv.reset()
        t0 = time.perf_counter()
        venv.step(acts[k], ids)
        tot += time.perf_counter() - t0
    return tot / steps


def _time_engine(eng, n, steps):
    acts = torch.rand((steps, n, 27), device=eng.device) * 2 - 1
    ids = torch.arange(n, dtype=torch.int32)
    eng.reset()
    for k in range(3):
        eng.step(acts[k], ids)
    eng.reset()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    tot = 0.0
    for k in range(steps):
        if k and k % (T - 1) == 0:
            torch.cuda.synchronize()
            eng.reset()
        ev[0].record()
        eng.step(acts[k], ids)
        ev[1].record()
        ev[1].synchronize()
        tot += ev[0].elapsed_time(ev[1]) * 1e-3
    return tot / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4,100,1024,8192")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--host-cap", type=int, default=100)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _register()
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        for name, sim in (("SimulatedEnv-v0", True), ("VirtualTB-v0", False)):
            dev = _venv(name, n, "cuda")
            dev.seed(1)
            eng = dev.vtb_env()
            row = collections.OrderedDict(kind="simulated" if sim else "raw", n_env=n)
            row["engine_us"] = 1e6 * _time_engine(eng, n, a.steps)
            if not a.kernels_only:
                row["plugin_us"] = 1e6 * _time_vector(dev, n, a.steps, sim)
                if n <= a.host_cap:
                    row["host_us"] = 1e6 * _time_vector(_venv(name, n, None), n, min(a.steps, 20), sim)
                    row["speedup"] = row["host_us"] / row["plugin_us"]
                else:
                    row["host_us"] = "not measured (n_env > host cap)"
            row["env_steps_per_s_plugin"] = n / (row.get("plugin_us", row["engine_us"]) * 1e-6)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
