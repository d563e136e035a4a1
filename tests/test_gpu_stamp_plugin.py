"""GPU: StateTrackerSTAMP behind the plugin objects (Collector / PPOPolicy / CollectorSet / the example script).
The tests are tests/test_gpu_slot_plugin.py's, called through the module (importing them by name would collect them twice); this file
defines their `wired` fixture for its one record."""
import pytest

import test_gpu_slot_plugin as checks
from slotcase import load_example
from stampcase import SLOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wired():
    ex = load_example()
    args = ex.get_args(checks.argv(SLOT))
    tab, train_envs, st, policy, coll = ex.build(args)
    return SLOT, ex, args, st, policy, coll


def test_collect_and_update_through_the_plugin_objects(wired):
    checks.test_collect_and_update_through_the_plugin_objects(wired)


def test_state_dict_round_trip_gives_the_same_greedy_collect(wired):
    checks.test_state_dict_round_trip_gives_the_same_greedy_collect(wired)


def test_collector_set_over_the_tracker(wired):
    checks.test_collector_set_over_the_tracker(wired)


def test_example_runs_with_the_tracker(tmp_path, monkeypatch):
    checks.test_example_runs_with_the_tracker(SLOT, tmp_path, monkeypatch)
