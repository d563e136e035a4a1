"""Record tests/golden/slot_workspace_bytes.json from the built library: what the six slot trackers' entry points answer without a GPU.

Run as `python tools/gen_golden_slot_workspace.py` from the repository root, on a build of the commit whose answers are to be kept -- the
file in the repository was recorded from the commit BEFORE the trackers' host code moved into csrc/slot_tracker.h, so that
tests/test_slot_library_cpu.py compares the shared scaffold with the six hand-written copies it replaced.  No test calls this.

Per tracker (tests/slotlibcase.py has the cases and the calls):
  workspace   cirs_X_tracker_backward_workspace_bytes for every cfg of the tracker's variants x n_env x dim_state, at each n_rows
  refused     a valid cfg with one common field made bad: return code and cirs_last_error() of init, step and backward with null weights and
              with a weights struct of null pointers; workspace_bytes_recorded is what workspace_bytes answered for that cfg on the recorded
              build (non-zero for avg, gru and lstm there: the test asserts 0, the rule the other three already followed)
  entry       a valid cfg walked through the checks of init, step and the head of backward one refusal at a time"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cirs-codes_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import slotlibcase as sc  # noqa: E402
from cirs_hip import abi  # noqa: E402


def main():
    lib = abi.lib()
    out = {}
    for name in sc.TRACKERS:
        ws = [dict(cfg=f, n_rows=sc.N_ROWS, bytes=[sc.workspace_bytes(lib, name, sc.make_cfg(name, f), r) for r in sc.N_ROWS])
              for f in sc.workspace_cfgs(name)]
        refused = []
        for bad in sc.BAD_FIELDS:
            f = sc.cfg_fields(name, **bad)
            cfg = sc.make_cfg(name, f)
            refused.append(dict(cfg=f, bad=bad, calls=sc.refused_calls(lib, name, cfg),
                                workspace_bytes_recorded=sc.workspace_bytes(lib, name, cfg, sc.REFUSED_N_ROWS)))
        f = sc.cfg_fields(name)
        out[name] = dict(workspace=ws, refused=refused, entry=dict(cfg=f, calls=sc.entry_sequence(lib, name, sc.make_cfg(name, f))))
    path = os.path.join(ROOT, "tests", "golden", "slot_workspace_bytes.json")
    with open(path, "w") as fh:      # one case per line: readable diffs, a few KB
        fh.write("{\n" + ",\n".join(
            f' "{name}": {{\n' + ",\n".join(
                f'  "{key}": ' + ("[\n" + ",\n".join("   " + json.dumps(e) for e in val) + "\n  ]" if isinstance(val, list)
                                  else "{\n" + f'   "cfg": {json.dumps(val["cfg"])},\n   "calls": [\n'
                                  + ",\n".join("    " + json.dumps(c) for c in val["calls"]) + "\n   ]\n  }")
                for key, val in t.items()) + "\n }" for name, t in out.items()) + "\n}\n")
    json.load(open(path))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
