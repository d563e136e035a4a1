"""GPU: gradient and Adam parity of the two VirtualTaobao trainers (csrc/mmoe_train.hip, csrc/mlp_train.hip, grad_adam_kernel of
csrc/train_step.hip) -- after each device step the gradient buffer against float64 autograd of the host restatement, the entries without
a data gradient against 2 c p exactly, both loss columns, and the moments / parameters against the float64 Adam recurrence fed the
device's own gradient (tests/vtbgradcase.py).  The shapes are the smallest that cross each boundary of the kernels: see
vtbgradcase.CASES."""
import pytest
import torch

import vtbgradcase as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(V.CASES))
def test_gradients_and_adam_against_float64(name):
    """Three consecutive steps on different rows (a gradient entry that is not rewritten shows as a stale one), then one step at
    t = 10000 (the bias corrections far from their first values)."""
    c = V.build(name)
    tr = V.make_trainer(c)
    cursor = 0
    for st in range(3):
        cursor, _ = V.check_step(tr, c, cursor, what=f"{name} step {st + 1}")
    tr.step_count = 9999
    V.check_step(tr, c, cursor, what=f"{name} step 10000")
    assert tr.step_count == 10000


@pytest.mark.parametrize("name", ["mmoe-128x128-n129", "mlp-40x72x24-n33"])
def test_two_identical_runs_leave_identical_gradient_bits(name):
    c = V.build(name)
    n = c["spec"]["n"]
    out = []
    for _ in range(2):
        tr = V.make_trainer(c)
        for st in range(2):
            tr.step(*(col[st * n:(st + 1) * n] for col in c["pool"]))
        out.append((tr.grads.clone(), tr.flat.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][0].abs().max()) > 0
