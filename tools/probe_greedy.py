"""Per-vector-step time of the greedy (no-noise) head launch against the sampled one at the benchmark shape, and of a whole greedy collect
against a sampled one:  python tools/probe_greedy.py [--workload c3|c2]
The head launch is timed by the library's own event pairs around it (cirs_prof_start / cirs_prof_stop, kernel id 3); a collect by HIP events."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
from cirs_hip import abi  # noqa: E402


def head_launch_us(eng, lib, **kw):
    abi.check(lib.cirs_prof_start(3, 64), "cirs_prof_start")
    eng.collect(**kw)
    torch.cuda.synchronize()
    tot, cnt = C.c_double(0.0), C.c_int32(0)
    abi.check(lib.cirs_prof_stop(C.byref(tot), C.byref(cnt)), "cirs_prof_stop")
    return tot.value / max(cnt.value, 1) * 1e6


def collect_ms(eng, reps=20, **kw):
    for _ in range(3):
        eng.collect(**kw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        eng.collect(**kw)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3", choices=sorted(bench.WORKLOADS))
    args = ap.parse_args()
    wl = bench.WORKLOADS[args.workload]
    eng, _ = bench.build_engine(wl, 0, 1, torch.device("cuda:0"))
    lib = abi.lib()
    eng.collect(); eng.collect(greedy=True)
    out = {"workload": args.workload, "n_env": wl["B"], "n_items": wl["I"], "max_turn": wl["T"],
           "head_launch_us_sampled": round(head_launch_us(eng, lib), 2), "head_launch_us_greedy": round(head_launch_us(eng, lib, greedy=True), 2),
           "collect_ms_sampled": round(collect_ms(eng), 3), "collect_ms_greedy": round(collect_ms(eng, greedy=True), 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
