"""GPU: the GRU state tracker (csrc/gru_tracker.hip) against the float64 restatement (cirs_hip/gru_host.py).
The checks are tests/test_gpu_slot_tracker.py's, the same for the four slot trackers; this file binds them to its tracker's record."""
import pytest

import test_gpu_slot_tracker as checks
from slotcase import GRU as SLOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_gru_states_match_float64_restatement(ci, mode):
    checks.states_match_float64_restatement(SLOT, ci, mode)


@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_gru_backward_matches_float64_autograd(ci):
    checks.backward_matches_float64_autograd(SLOT, ci)


def test_gru_backward_refuses_a_short_workspace():
    checks.backward_refuses_a_short_workspace(SLOT)


@pytest.mark.parametrize("walk", SLOT.walk, ids=[f"{w[0]}-{w[2]}" for w in SLOT.walk])
def test_gru_states_when_a_wavefront_walks_several_envs(walk):
    checks.states_when_a_launch_walks_several_env_groups(SLOT, walk)
