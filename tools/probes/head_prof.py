"""Per-tile stage timestamps of head_bwd_fused_kernel (probe build: tools/probes/build_prof_lib.sh), C3 minibatch of 1024 rows.
    python tools/probes/head_prof.py"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))
import numpy as np
import torch
from cirs_hip import abi

abi.LIB_PATH = os.path.join(ROOT, "tools", "probes", "libcirs_prof.so")
import bench

wl = bench.WORKLOADS["c3"]
eng, _ = bench.build_engine(wl, 0, 1, torch.device("cuda:0"))
eng.collect(); eng.update(1024, 1)
lib = C.CDLL(abi.LIB_PATH)
# the two-role form (the default): role A = wave 0, role B = wave 4 one iteration later, both at the workgroup's third tile
names = {0: "A: tile start", 1: "A: slab values -> acc, next tile requested", 2: "A: C-plane operand reads", 3: "A: dZ (exp2, coefficients, action, mask)",
         4: "A: dZ^T -> LDS (+ high-side clamp correction)", 5: "A: split + dH2 MFMAs (12)", 10: "A: the tile's one barrier",
         11: "B: iteration start (one iteration later)", 12: "B: plane request, dZ^T read, partial tiles of the tile before", 13: "B: db, split + dWa MFMAs (12)",
         14: "B: plane commit, wave-order sum + slab stores", 15: "B: partial-tile writes"}
acc = None
for rep in range(8):
    bench.hip_event_kernel_time(eng, wl, reps=2)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * 64)()
    assert lib.cirs_debug_head_prof(buf) == 0
    t = np.array(buf[:], dtype=np.float64)
    if rep >= 2:
        acc = t if acc is None else acc + t
t = acc / 6
prev = t[0]
print("head_bwd_fused_kernel, workgroup (0,0) wave 0, third tile (raw s_memtime ticks):")
for k in sorted(names):
    print(f"  {names[k]:36s} {t[k] - prev:9.0f}   (cum {t[k] - t[0]:9.0f})")
    prev = t[k]

ks = {30: "kernel entry", 31: "row coefficients (merge prologue)", 32: "barrier (first planes tile staged by role B)", 33: "all tiles",
      35: "dH2 / entropy partial stores"}
print("head_bwd_fused_kernel, workgroup (0,0) thread 0, whole kernel:")
prev = t[30]
for k in sorted(ks):
    print(f"  {ks[k]:52s} {t[k] - prev:9.0f}   (cum {t[k] - t[30]:9.0f})")
    prev = t[k]
tb = {16: "row workgroup 0: entry", 17: "W2/W1 columns requested, 31 dh2 slabs summed, da2 written", 18: "barrier", 19: "da1 tile (32 MFMAs), relu gate, stores", 20: "barrier",
      21: "dW1 tile (wave 0)"}
print("trunk_bwd_kernel (raw ticks; the stamps of thread 0 = wave 0):")
prev = t[16]
for k in sorted(tb):
    print(f"  {tb[k]:64s} {t[k] - prev:9.0f}   (cum {t[k] - t[16]:9.0f})")
    prev = t[k]
print(f"  first wa|ba slab-sum workgroup: entry at {t[24] - t[16]:+.0f} relative to row workgroup 0, its sums + reduction take {t[25] - t[24]:.0f}")

hs = {40: "head_stats workgroup (0,0): entry", 41: "H2 tile coalesced -> LDS -> split into bf16 planes", 42: "first planes tile staged, barrier",
      43: "(tiles 0, 1)", 44: "tile 2: next tile requested, LDS operand reads, bias init", 45: "tile 2: 24 MFMAs", 46: "tile 2: mask, max, 16 exp, running sums",
      47: "tile 2: commit next + barrier", 48: "remaining tiles"}
print("head_stats_kernel (raw ticks; two workgroups per CU share the SIMDs):")
prev = t[40]
for k in sorted(hs):
    print(f"  {hs[k]:64s} {t[k] - prev:9.0f}   (cum {t[k] - t[40]:9.0f})")
    prev = t[k]
