"""GPU: DeviceRollout.collect with the filter-MLP tracker (cirs_rollout_collect_fmlp).  The rollout model is W = 3, L = 2 at T = 8: the tile
slides from position 4 on, and up to position 2 it holds padded rows that layer 0's filter writes into and layer 1 reads.
The checks are tests/test_gpu_slot_rollout.py's, the same for every slot tracker; this file binds them to its tracker's record."""
import pytest

import test_gpu_slot_rollout as checks
from fmlpcase import SLOT
from test_gpu_slot_rollout import tables  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [6, 70])
@pytest.mark.parametrize("mode", ["sampled", "greedy", "remove", "force"])
def test_collect_equals_the_steps_issued_one_at_a_time(tables, B, mode):  # noqa: F811
    checks.collect_equals_the_steps_issued_one_at_a_time(tables, SLOT, B, mode)


def test_harness_noise_is_the_sampler_with_that_noise(tables):  # noqa: F811
    checks.harness_noise_is_the_sampler_with_that_noise(tables, SLOT)


def test_what_is_not_built_is_refused(tables):  # noqa: F811
    checks.what_is_not_built_is_refused(tables, SLOT)
