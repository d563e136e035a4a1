"""GPU: the linear-recurrence state tracker (csrc/lru_tracker.hip) against the float64 restatement (cirs_hip/lru_host.py): every state of
every live (env, position) through reset / init / step in both replay modes, every gradient tensor of the backward against float64 autograd.
The checks are tests/test_gpu_slot_tracker.py's, the same for every slot tracker; this file binds them to its tracker's record
(tests/lrucase.py) and adds one for what this model alone carries per env: the complex state as h_re and h_im.
The model is smooth: no case and no element is skipped or masked."""
import numpy as np
import pytest
import torch

import test_gpu_slot_tracker as checks
from lrucase import SLOT
from slotcase import backward_args, reference, replayed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_lru_states_match_float64_restatement(ci, mode):
    checks.states_match_float64_restatement(SLOT, ci, mode)


@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_lru_backward_matches_float64_autograd(ci):
    checks.backward_matches_float64_autograd(SLOT, ci)


def test_lru_backward_refuses_a_short_workspace():
    checks.backward_refuses_a_short_workspace(SLOT)


def test_lru_states_when_a_workgroup_walks_several_envs():
    checks.states_when_a_launch_walks_several_env_groups(SLOT, SLOT.walk[0])


def test_lru_carried_state_matches_float64_and_a_second_backward_gives_the_same_bits():
    """After the teacher-forced replay of case 0: the carried h_re[0, b] / h_im[0, b] of every env are the restatement's hidden state at the
    env's last live position; then two backward calls on a NaN-filled flat_grad leave the same bits and no NaN."""
    from cirs_hip import lru_host
    case, ci = SLOT.case, 0
    (U, I, B, T, S, hot), model = SLOT.split(SLOT.CASES[ci])
    ref = reference(SLOT, ci)
    trk, _ = replayed(SLOT, ci)
    lens = ref["lens"]
    kept = {}
    for dtype in (torch.float64, torch.float32):
        kept[dtype] = {}
        lru_host.states(lru_host.cast_params(ref["p"], dtype), ref["users"], ref["acts"], ref["rews"], model, kept[dtype])
    b = np.arange(B)
    for name in ("h_re", "h_im"):
        want = kept[torch.float64][name].numpy()[b, lens - 1]
        want32 = kept[torch.float32][name].numpy()[b, lens - 1]
        have = getattr(trk, name).cpu().numpy().astype(np.float64)
        assert have.shape == (1, B, 32) and want.shape == (B, 32)
        scale = np.abs(want).max()
        err = np.abs(have[0] - want).max() / scale
        err32 = np.abs(want32 - want).max() / scale
        bar = case.bar_for(case.STATE_BAR, err32)
        print(f"carried {name} lru {SLOT.IDS[ci]}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar, name
    args = backward_args(ref, T, B, S)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    assert torch.equal(trk.flat_grad, first)
