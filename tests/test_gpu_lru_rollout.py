"""GPU: DeviceRollout.collect with the linear-recurrence tracker (cirs_rollout_collect_lru).  T = 8: an env carries its complex state through
up to nine steps of the collect's own launch sequence.
The checks are tests/test_gpu_slot_rollout.py's, the same for every slot tracker; this file binds them to its tracker's record."""
import pytest

import test_gpu_slot_rollout as checks
from lrucase import SLOT
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
