"""GPU: gradient and Adam parity of the Kuaishou trainers (csrc/deepfm_train.hip, csrc/dice_train.hip, csrc/table_step.h, launch_dw_gemm) --
after each device step the gradient buffer against float64 autograd of the host restatement, the entries without a data gradient
against 2 c p exactly, the loss columns, and the moments / parameters against the float64 Adam recurrence fed the device's own gradient
(tests/gradcase.py).  The shapes are the smallest that cross each boundary of the kernels: see gradcase.CASES."""
import numpy as np
import pytest
import torch

import gradcase as G

pytestmark = pytest.mark.gpu


def _first_linear_model_offset(tr):
    name = next(k for k in tr.views if k.startswith("linear_model."))
    return (tr.views[name].data_ptr() - tr.flat.data_ptr()) // 4


@pytest.mark.parametrize("name", list(G.CASES))
def test_gradients_and_adam_against_float64(name):
    """Three consecutive steps on batches with different ids (a gradient row that is not cleared shows as a non-zero untouched row), then
    one step at t = 10000 (the bias corrections far from their first values)."""
    c = G.build(name)
    tr, host = G.make_trainer(c), G.host_module(c["spec"])
    if name.endswith("bigtables"):       # a second trip of the Adam kernel's grid (1024 x 256 elements), with a regulariser segment starting inside it
        assert tr.flat.numel() > 262144 and _first_linear_model_offset(tr) > 262144
    if name.endswith("slabcap"):
        rows = (2 if c["spec"]["trainer"] == "deepfm" else 4) * c["spec"]["n"]
        assert rows == 16400 > 256 * 64
    for b in range(3):
        G.check_step(tr, host, c["batches"][b], c["hyper"], what=f"{name} step {b + 1}")
    tr.step_count = 9999
    G.check_step(tr, host, c["batches"][3], c["hyper"], what=f"{name} step 10000")
    assert tr.step_count == 10000


@pytest.mark.parametrize("name", ["deepfm-pd-segments", "dice-segments"])
def test_two_identical_runs_leave_identical_gradient_bits(name):
    c = G.build(name)
    out = []
    for _ in range(2):
        tr = G.make_trainer(c)
        for b in range(2):
            tr.step(*c["batches"][b])
        out.append((tr.grads.clone(), tr.flat.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][0].abs().max()) > 0


def test_dice_step_and_epoch_leave_equal_gradients():
    c = G.build("dice-E16")
    x, y, s = c["batches"][0]
    a, b = G.make_trainer(c), G.make_trainer(c)
    la = a.step(x, y, s).clone()
    assert b.load(x, y, s) == len(x)
    lb = b.epoch(None, len(x))
    assert torch.equal(a.grads, b.grads) and torch.equal(a.flat, b.flat) and torch.equal(la, lb[0])
    assert float(a.grads.abs().max()) > 0
