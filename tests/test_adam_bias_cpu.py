"""adam_bias (csrc/optim.h), the one place where the library forms the bias corrections of torch.optim.Adam, against torch's own
computation of them: step_size = lr / (1 - beta1^t), bc2s = sqrt(1 - beta2^t) and its reciprocal in Python floats (fp64), rounded to
float32.  A stand-alone host program includes the header and prints the bit patterns; no GPU is touched.

The C ABI hands the hyper-parameters over as float32, so the Python side starts from the same float32 values (0.9f is
0.899999976..., not 0.9).  With the float64 literals instead, the values differ from the library's, today as before this header, by up to
3 units in the last place of step_size and 107 of rbc2s at t <= 3 and by at most 1 from t = 9999 on.

The VirtualTaobao learner reads its hyper-parameters from the optimiser it is given, and a default torch.optim.Adam has the triple of the
first case: the two cases the work item names coincide today (the second follows the learner's defaults should they move).  The third
case has other bases for both powers."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cirs-codes_amd", "csrc")
STEPS = (1, 2, 3, 1000, 9999, 10000, 20001)

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "optim.h"
static unsigned bits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
int main(int argc, char** argv) {
    const float lr = strtof(argv[1], nullptr), b1 = strtof(argv[2], nullptr), b2 = strtof(argv[3], nullptr);
    for (int i = 4; i < argc; ++i) {
        const cirs::AdamBias b = cirs::adam_bias(lr, b1, b2, atoll(argv[i]));
        printf("%s %08x %08x %08x\n", argv[i], bits(b.step_size), bits(b.bc2s), bits(b.rbc2s));
    }
    return 0;
}
"""


def _learner_defaults():
    from cirs_hip.vtb_learn import _hyper
    return _hyper(torch.optim.Adam([torch.zeros(1, requires_grad=True)]))[:3]   # what learner="device" reads from a default optim_RL


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no host compiler for HIP headers")
    d = tmp_path_factory.mktemp("adam_bias")
    src, exe = str(d / "adam_bias_main.hip"), str(d / "adam_bias_main")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, src, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("hyper", [(1e-3, 0.9, 0.999), "virtualtaobao-learner", (3e-4, 0.8, 0.99)],
                         ids=["1e-3_0.9_0.999", "virtualtaobao-learner", "3e-4_0.8_0.99"])
def test_adam_bias_bits(program, hyper):
    lr, b1, b2 = (float(np.float32(x)) for x in (_learner_defaults() if isinstance(hyper, str) else hyper))
    out = subprocess.run([program, repr(lr), repr(b1), repr(b2)] + [str(t) for t in STEPS], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    assert [int(r[0]) for r in rows] == list(STEPS)
    for r, t in zip(rows, STEPS):
        want = (np.float32(lr / (1 - b1 ** t)), np.float32(math.sqrt(1 - b2 ** t)), np.float32(1 / math.sqrt(1 - b2 ** t)))
        got = tuple(int(h, 16) for h in r[1:])
        print(t, r[1:], [f"{int(w.view(np.uint32)):08x}" for w in want])
        assert got == tuple(int(w.view(np.uint32)) for w in want), f"t = {t}"
