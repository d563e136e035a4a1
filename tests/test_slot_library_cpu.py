"""CPU: the six slot trackers' entry points (csrc/slot_tracker.h under gru / lstm / avg / caser / nextitnet / stamp _tracker.hip) answer what
the six hand-written copies answered before they shared one scaffold.  tests/golden/slot_workspace_bytes.json was recorded from that earlier
library by tools/gen_golden_slot_workspace.py; tests/slotlibcase.py makes the calls, none of which reaches a launch.
  workspace sizes   equal to the byte, for every recorded cfg and n_rows
  refusals          return code and message of init / step / backward equal for every refused cfg: one common field bad, and several at once
                    (the order of the reports)
  refused cfgs      cirs_X_tracker_backward_workspace_bytes is 0 for every cfg the tracker's validation refuses -- the rule caser, nextitnet
                    and stamp followed; avg, gru and lstm answered a size for some of them (workspace_bytes_recorded keeps what)
  entry checks      a valid cfg through init, step and the head of backward, one refusal at a time, in the recorded order"""
import json
import os

import pytest

import slotlibcase as sc
from cirs_hip import abi

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slot_workspace_bytes.json")) as _fh:
    GOLDEN = json.load(_fh)
NAMES = list(sc.TRACKERS)


def test_golden_file_covers_the_cases():
    assert list(GOLDEN) == NAMES
    for name in NAMES:
        g = GOLDEN[name]
        assert [e["cfg"] for e in g["workspace"]] == list(sc.workspace_cfgs(name)) and all(e["n_rows"] == sc.N_ROWS for e in g["workspace"])
        assert [e["bad"] for e in g["refused"]] == sc.BAD_FIELDS and [e["cfg"] for e in g["refused"]] == [sc.cfg_fields(name, **b) for b in sc.BAD_FIELDS]
        assert g["entry"]["cfg"] == sc.cfg_fields(name)
        assert all(b > 0 for e in g["workspace"] for b in e["bytes"])
    # what the earlier library answered on refused cfgs: nothing for the three trackers whose rule is kept, a size from the other three
    for name in ("caser", "nextitnet", "stamp"):
        assert all(e["workspace_bytes_recorded"] == 0 for e in GOLDEN[name]["refused"])
    for name in ("avg", "gru", "lstm"):
        assert any(e["workspace_bytes_recorded"] > 0 for e in GOLDEN[name]["refused"])


@pytest.mark.parametrize("name", NAMES)
def test_workspace_bytes_equal_the_recorded_sizes(name):
    lib = abi.lib()
    for e in GOLDEN[name]["workspace"]:
        cfg = sc.make_cfg(name, e["cfg"])
        got = [sc.workspace_bytes(lib, name, cfg, r) for r in e["n_rows"]]
        assert got == e["bytes"], (e["cfg"], got)
        assert sc.workspace_bytes(lib, name, cfg, 0) == 0 and sc.workspace_bytes(lib, name, cfg, -3) == 0


@pytest.mark.parametrize("name", NAMES)
def test_refused_cfgs_keep_code_message_and_order_and_size_zero(name):
    lib = abi.lib()
    for e in GOLDEN[name]["refused"]:
        cfg = sc.make_cfg(name, e["cfg"])
        got = sc.refused_calls(lib, name, cfg)
        assert got == e["calls"], (e["bad"], got)
        assert all(rc != 0 for calls in got.values() for rc, _ in calls)
        for n_rows in (1, sc.REFUSED_N_ROWS, 16385):
            assert sc.workspace_bytes(lib, name, cfg, n_rows) == 0, e["bad"]
    assert sc.workspace_bytes(lib, name, None, 7) == 0


@pytest.mark.parametrize("name", NAMES)
def test_entry_checks_keep_their_order_and_messages(name):
    lib = abi.lib()
    e = GOLDEN[name]["entry"]
    cfg = sc.make_cfg(name, e["cfg"])
    got = sc.entry_sequence(lib, name, cfg)
    assert got == e["calls"], got
    by = {label: (rc, msg) for label, rc, msg in got}
    for call in ("init", "step", "backward"):      # a valid cfg with null weights, with null weight pointers: refused by all three
        assert by[f"{call} weights null"][0] != 0 and "null" in by[f"{call} weights null"][1]
        assert by[f"{call} weight pointers null"] == (-1, f"{name} tracker: weight pointer null")
    assert by["init n = 0"] == (0, "") and by["step n = 0"] == (0, "")
    assert sc.workspace_bytes(lib, name, cfg, 0) == 0 and sc.workspace_bytes(lib, name, cfg, 4) > 0
