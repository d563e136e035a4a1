"""GPU: the GRU-with-attention state tracker (csrc/narm_tracker.hip) against the float64 restatement (cirs_hip/narm_host.py): every state of
every live (env, position) through reset / init / step in both replay modes, every gradient tensor of the backward against float64 autograd.
The checks are tests/test_gpu_slot_tracker.py's, the same for every slot tracker; this file binds them to its tracker's record
(tests/narmcase.py) and adds one for what this model alone keeps per env: the histories of its hidden states and of their A2 projections.
The model is smooth: no case and no element is skipped or masked."""
import numpy as np
import pytest
import torch

import test_gpu_slot_tracker as checks
from narmcase import SLOT
from slotcase import backward_args, reference, replayed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_narm_states_match_float64_restatement(ci, mode):
    checks.states_match_float64_restatement(SLOT, ci, mode)


@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_narm_backward_matches_float64_autograd(ci):
    checks.backward_matches_float64_autograd(SLOT, ci)


def test_narm_backward_refuses_a_short_workspace():
    checks.backward_refuses_a_short_workspace(SLOT)


def test_narm_states_when_a_workgroup_walks_several_envs():
    checks.states_when_a_launch_walks_several_env_groups(SLOT, SLOT.walk[0])


def test_narm_histories_match_float64_and_a_second_backward_gives_the_same_bits():
    """After the teacher-forced replay of case 0: h_hist[b, p] is the restatement's hidden state and q_hist[b, p] its A2 projection at every
    live (b, p); then two backward calls on the same inputs leave the same bits in flat_grad."""
    from cirs_hip import narm_host
    case, ci = SLOT.case, 0
    (U, I, B, T, S, hot), model = SLOT.split(SLOT.CASES[ci])
    ref = reference(SLOT, ci)
    trk, _ = replayed(SLOT, ci)
    live = ref["live"]
    kept = {}
    for dtype in (torch.float64, torch.float32):
        kept[dtype] = {}
        narm_host.states(narm_host.cast_params(ref["p"], dtype), ref["users"], ref["acts"], ref["rews"], model, kept[dtype])
    h64 = kept[torch.float64]["h"].numpy()
    a2 = ref["p"]["attn.a2.weight"].double().numpy()
    want = {"h_hist": h64, "q_hist": h64 @ a2.T}
    np.testing.assert_allclose(kept[torch.float64]["q"].numpy(), want["q_hist"], rtol=0, atol=1e-13)
    for name, key in (("h_hist", "h"), ("q_hist", "q")):
        have = getattr(trk, name).cpu().numpy().astype(np.float64)
        assert have.shape == want[name].shape == (B, T + 1, 32)
        scale = np.abs(want[name][live]).max()
        err = np.abs(have[live] - want[name][live]).max() / scale
        err32 = np.abs(kept[torch.float32][key].numpy()[live] - want[name][live]).max() / scale
        bar = case.bar_for(case.STATE_BAR, err32)
        print(f"{name} narm {SLOT.IDS[ci]}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar, name
    args = backward_args(ref, T, B, S)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    assert torch.equal(trk.flat_grad, first)
