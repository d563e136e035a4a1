"""GPU: the filter-MLP state tracker (csrc/fmlp_tracker.hip) against the float64 restatement (cirs_hip/fmlp_host.py): every state of every
live (env, position) through reset / init / step in both replay modes, every gradient tensor of the backward against float64 autograd.  The
restatement filters in the frequency domain (rfft / irfft), the device in the time domain: the check is between two formulations.
The checks are tests/test_gpu_slot_tracker.py's, the same for every slot tracker; this file binds them to its tracker's record
(tests/fmlpcase.py).  The model is smooth: no case and no element is skipped or masked."""
import pytest

import test_gpu_slot_tracker as checks
from fmlpcase import SLOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_fmlp_states_match_float64_restatement(ci, mode):
    checks.states_match_float64_restatement(SLOT, ci, mode)


@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_fmlp_backward_matches_float64_autograd(ci):
    checks.backward_matches_float64_autograd(SLOT, ci)


def test_fmlp_backward_refuses_a_short_workspace():
    checks.backward_refuses_a_short_workspace(SLOT)


def test_fmlp_states_when_a_workgroup_walks_several_envs():
    checks.states_when_a_launch_walks_several_env_groups(SLOT, SLOT.walk[0])
