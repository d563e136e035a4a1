"""GPU: StateTrackerLRU behind the plugin objects (Collector / PPOPolicy / CollectorSet / the example script).
The tests are tests/test_gpu_slot_plugin.py's, called through the module (importing them by name would collect them twice); this file
defines their `wired` fixture for its one record."""
import pytest

import test_gpu_slot_plugin as checks
from slotcase import load_example
from lrucase import SLOT

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


def test_entry_point_walk_takes_the_tracker(tmp_path, monkeypatch):
    """examples/cirs_rl_kuaishou.py --tracker lru: the step-for-step walk of the reference's entry point, on a synthetic KuaiRec-format
    workspace, builds StateTrackerLRU, trains it and saves its 23 tensors in the checkpoint."""
    import importlib.util
    import os

    import torch
    from slotcase import ROOT
    spec = importlib.util.spec_from_file_location("cirs_rl_kuaishou_entry", os.path.join(ROOT, "examples", "cirs_rl_kuaishou.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    monkeypatch.setenv("CIRS_DATAPATH", os.environ.get("CIRS_DATAPATH", ""))      # the example sets it: restored after the test
    ws = str(tmp_path / "ws")
    out = ex.run(["--workspace", ws, "--tracker", "lru", "--epoch", "1", "--step-per-epoch", "120", "--training-num", "16", "--test-num", "8",
                  "--episode-per-collect", "16", "--batch-size", "64", "--max_turn", "8", "--leave_threshold", "1", "--num_leave_compute", "3",
                  "--force_length", "5", "--tau", "10"])
    st = out["state_tracker"]
    assert type(st).__name__ == "StateTrackerLRU" and st.adam_steps >= 1
    ckpt = torch.load(os.path.join(ws, out["model_save_path"]), map_location="cpu", weights_only=False)
    assert list(ckpt["state_tracker"]) == list(SLOT.param_shapes(st.n_users, st.n_items, 20, 1))
    assert all(torch.isfinite(v).all() for v in ckpt["state_tracker"].values())
