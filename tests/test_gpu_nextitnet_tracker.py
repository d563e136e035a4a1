"""GPU: the dilated-convolution state tracker (csrc/nextitnet_tracker.hip) against the float64 restatement (cirs_hip/nextitnet_host.py): the
device computes every position from the cone of its last slots, the restatement the whole history at once.
The checks are tests/test_gpu_slot_tracker.py's, the same for every slot tracker; this file binds them to its tracker's record
(tests/nextitnetcase.py).  The cases' inputs are ones where float64 itself is unambiguous at every ReLU (tests/test_nextitnet_host_cpu.py
checks that on the CPU): no case and no element is skipped or masked."""
import pytest

import test_gpu_slot_tracker as checks
from nextitnetcase import SLOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_nextitnet_states_match_float64_restatement(ci, mode):
    checks.states_match_float64_restatement(SLOT, ci, mode)


@pytest.mark.parametrize("ci", range(len(SLOT.CASES)), ids=SLOT.IDS)
def test_nextitnet_backward_matches_float64_autograd(ci):
    checks.backward_matches_float64_autograd(SLOT, ci)


def test_nextitnet_backward_refuses_a_short_workspace():
    checks.backward_refuses_a_short_workspace(SLOT)


def test_nextitnet_states_when_a_workgroup_walks_several_envs():
    checks.states_when_a_launch_walks_several_env_groups(SLOT, SLOT.walk[0])
