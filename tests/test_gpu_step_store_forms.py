"""GPU: the minibatch step's slabs leave as 16-byte write-through units (the dWa row-block slabs, the logit slab, the optimiser launch's p / m / v,
fp16 planes and next-step tiles, the flat Wa gradient, the 8-row slabs of the trunk backward).  A store form changes no value, so every comparison
is torch.equal; what 16-byte units add is a way to be wrong at the END of an array -- a unit that straddles it, a last unit that is dropped -- and a
step that reads what the step before wrote through.  So:

  catalogue sizes   I = 21, 101, 182 (I mod 4 = 1, 2, 3: wa_len = 65 I ends in 1, 2 or 3 elements after the last whole float4 of the flat gradient,
                    and the last item tile is partial), 100 and 224 (whole float4s; 224: whole tiles)
  minibatch sizes   32 rows (one live wave pair), 70 (padding rows inside a tile), 200 (a second row block)
  head kernels      the hand-over step (CIRS_PPO_HEAD_RECOMPUTE=0: logit slab + two-role backward, written through) against the recompute step
                    (=1: the plain-store kernels), steps of 32, 70 and 200 rows in a row
  chain of steps    cirs_ppo_learn's loop (step k + 1 reads the planes, p / m / v and H2 tiles that step k's optimiser launch wrote through) against
                    one cirs_ppo_minibatch call per step (each call forms them again with plain stores), at least three consecutive steps

Every byte of the workspace is 0xff before every call.  The helpers of test_gpu_learn.py fix the state width at 20 (S % 4 == 0), so the trunk
backward's scalar form for other widths is not reached from here; its condition is `(S & 3) == 0` on the kernel argument."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_head_bwd_roles import _case, _run
from test_gpu_learn import make_learner, upload_traj

pytestmark = pytest.mark.gpu

SIZES = (21, 101, 182, 100, 224)
ROWS = (32, 70, 200)
NAMES = ("losses", "params", "adam_m", "adam_v", "dobs")


@functools.lru_cache(maxsize=None)
def _shared_case(I):
    return _case(I)


def _ent(I):
    return 0.01 if I % 2 else 0.0      # both dZ instantiations over the sizes


def _same(a, b):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} of {x.numel()} elements differ, max |d| = {float((x - y).abs().max()):.3e}"
        assert bool(torch.isfinite(x).all()), name


@pytest.mark.parametrize("I", SIZES)
def test_written_through_head_slabs_give_the_bits_of_the_recompute_step(I, monkeypatch):
    monkeypatch.setenv("CIRS_PPO_MERGE_KERNEL", "0")
    case = _shared_case(I)
    assert (65 * I) % 4 == I % 4 and (I % 32 != 0) == (I != 224)
    a, b = (_run(monkeypatch, recompute, case, I, _ent(I)) for recompute in (False, True))
    _same(a, b)


def _learner(case, I, bs, rep):
    from cirs_hip.rollout import Trajectory
    B, T, pp, lens, acts, rews, dones, obs, n, value, logp, rows = case
    traj = Trajectory(B, T, 20, "cuda")
    upload_traj(traj, acts, rews, dones, lens, obs, value, logp)
    ln, _ = make_learner(pp, I, B, T, [0.95, 0.95, 0.2, 0.25, _ent(I), 0.5, 1e-3, bs, rep])
    assert ln.prepare(traj, lens) == n
    ln.dobs.fill_(7.0)
    return ln


@pytest.mark.parametrize("bs", ROWS)
@pytest.mark.parametrize("I", SIZES)
def test_steps_that_read_the_written_through_state_of_the_step_before(I, bs, monkeypatch):
    from cirs_hip import abi
    from cirs_hip.learner import minibatch_slices
    monkeypatch.setenv("CIRS_PPO_HEAD_RECOMPUTE", "0")
    monkeypatch.setenv("CIRS_PPO_LEARN_PREFETCH", "1")
    case = _shared_case(I)
    n, rows = case[8], case[11]
    rep = 2
    perms = [rows, rows[::-1].copy()]
    slices = minibatch_slices(n, bs)
    assert rep * len(slices) >= 3
    max_mb = max(e - s for s, e in slices)
    # the loop: one call, the optimiser launch of step k runs the head of step k + 1
    ln = _learner(case, I, bs, rep)
    ln.workspace(max_mb).fill_(255)
    la = ln.learn(bs, rep, perms=perms)
    torch.cuda.synchronize()
    a = (la.clone(), ln.params.clone(), ln.adam_m.clone(), ln.adam_v.clone(), ln.dobs.clone())
    # one call per step
    ln = _learner(case, I, bs, rep)
    lb = torch.zeros((rep * len(slices), 4), dtype=torch.float32, device="cuda")
    perm_d = torch.as_tensor(np.stack(perms).astype(np.int32)).cuda()
    k = 0
    for r in range(rep):
        last = r == rep - 1
        if last:
            ln.dobs.zero_()
        for s0, e0 in slices:
            ws = ln.workspace(max_mb)
            ws.fill_(255)
            abi.check(ln._lib.cirs_ppo_minibatch(C.byref(ln.cfg), ln.params.data_ptr(), ln.grads.data_ptr(), ln.adam_m.data_ptr(), ln.adam_v.data_ptr(),
                                                 ln.opt_step, C.byref(ln.batch), perm_d[r].data_ptr() + 4 * s0, e0 - s0,
                                                 ln.dobs.data_ptr() if last else None, ln.n_env, lb[k].data_ptr(), ws.data_ptr(), ws.numel(),
                                                 ln._stream()), "cirs_ppo_minibatch")
            ln.opt_step += 1
            k += 1
    torch.cuda.synchronize()
    b = (lb.clone(), ln.params.clone(), ln.adam_m.clone(), ln.adam_v.clone(), ln.dobs.clone())
    _same(a, b)
