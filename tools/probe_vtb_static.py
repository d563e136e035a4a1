"""Timing of evaluation.test_taobao: the one-launch device path (cirs_hip/vtb_static.py) against the reference's host procedure.

    python tools/probe_vtb_static.py [--traj 100] [--max-turn 50] [--thr 0.4] [--reps 3] [--host-traj 100] [--out FILE]

The script's shape (dnn 256 x 256, 4 experts of dim 8) with weights scaled up as the tests scale them (the reference's init would make
every prediction round-off and every trajectory 2 turns long), max_turn 50, epsilon 0 and 0.3.  Per epsilon one JSON line:
  device_wall_ms   median of `reps` DeviceVtbStaticEval.run calls after a warm-up, wall clock, the read-back of metrics and lengths included
  device_event_ms  the same calls between two device events (launch + reduction, buffers' allocation and zeroing included)
  entry_wall_ms    median of `reps` evaluation.test_taobao(model, env, epsilon, device="cuda") calls: what an epoch end pays, the evaluator's
                   construction (weight upload, buffers) included
  turns            env steps the evaluation played; longest: the longest trajectory (the kernel's critical path)
  host_ms          median of `reps` test_taobao(device=None) calls on this machine (the reference's procedure)
  factor           host_ms / device_wall_ms (factor_entry: host_ms / entry_wall_ms), and the per-step times of both
--kernels-only runs the device calls alone, for a `rocprofv3 --kernel-trace --stats -- python tools/probe_vtb_static.py --kernels-only`
run of its own."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cirs-codes_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=100)
    ap.add_argument("--max-turn", type=int, default=50)
    ap.add_argument("--thr", type=float, default=0.4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-traj", type=int, default=100)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import evaluation
    import vtbcase
    import vtbstaticcase as case
    from cirs_hip.vtb_static import DeviceVtbStaticEval
    model = case.two_task_model((256, 256))
    env = vtbcase.base_vtb(GOLDEN, 5, a.thr, a.max_turn)
    env.set_state_mode(True)
    ev = DeviceVtbStaticEval(env, model, a.traj, seed=1, device="cuda")
    rows = []
    for eps in (0.0, 0.3):
        ev.run(eps)                                   # warm-up
        torch.cuda.synchronize()
        wall, evt = [], []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            e0.record()
            ev.run(eps)
            e1.record()
            wall.append(time.perf_counter() - t0)
            e1.synchronize()
            evt.append(e0.elapsed_time(e1))
        row = collections.OrderedDict(epsilon=eps, n_traj=a.traj, max_turn=a.max_turn, device_wall_ms=1e3 * statistics.median(wall),
                                      device_event_ms=statistics.median(evt), turns=int(ev.lengths.sum()), longest=int(ev.lengths.max()))
        row["device_us_per_step"] = 1e3 * row["device_wall_ms"] / row["turns"]
        if not a.kernels_only:
            entry = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                evaluation.test_taobao(model, env, eps, device="cuda", num_trajectory=a.traj, seed=1)
                entry.append(time.perf_counter() - t0)
            row["entry_wall_ms"] = 1e3 * statistics.median(entry[1:])
            host, steps = [], []
            for r in range(a.reps):
                torch.manual_seed(r)
                np.random.seed(r)
                rec = case.Recorder(model, env)
                rec.env.static = True
                t0 = time.perf_counter()
                evaluation.test_taobao(rec, rec.env, eps, num_trajectory=a.host_traj)
                host.append(time.perf_counter() - t0)
                steps.append(len(rec.rows))
            k = int(np.argsort(host)[len(host) // 2])
            row["host_ms"], row["host_turns"] = 1e3 * host[k] * a.traj / a.host_traj, steps[k] * a.traj // a.host_traj
            row["host_us_per_step"] = 1e6 * host[k] / steps[k]
            row["factor"] = row["host_ms"] / row["device_wall_ms"]
            row["factor_entry"] = row["host_ms"] / row["entry_wall_ms"]
            row["factor_per_step"] = row["host_us_per_step"] / row["device_us_per_step"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
