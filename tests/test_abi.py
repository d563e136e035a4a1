"""CPU: libcirs_hip.so loads without a GPU and exports exactly the entry points include/cirs_hip.h declares."""
import ctypes as C
import os
import re

from cirs_hip import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "cirs_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cirs_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = abi.lib()  # raises if the .so is missing or a bound symbol is absent
    syms = header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/cirs_hip.h but not exported"
        assert s in abi.SIGNATURES, f"{s} has no ctypes signature in cirs_hip/abi.py"
    for s in abi.SIGNATURES:
        assert s in syms, f"{s} bound in abi.py but not declared in the header"


def test_version_and_error_plumbing():
    lib = abi.lib()
    assert lib.cirs_version() >= 100
    # argument validation happens on the host before any launch: safe without a GPU
    rc = lib.cirs_env_step(None, None, None, None, None, 0, None, None, None, None, None, None)
    assert rc == -1 and b"cfg" in lib.cirs_last_error()
    cfg = abi.EnvCfg(n_users=3, n_items=4, max_turn=5, num_leave_compute=1, leave_threshold=0, version=3, dist_mode=0, simulated=1)
    assert lib.cirs_env_step(C.byref(cfg), None, None, None, None, 1, None, None, None, None, None, None) == -1
    assert b"version" in lib.cirs_last_error()
    cfg.version = 1
    assert lib.cirs_env_step(C.byref(cfg), None, None, None, None, 0, None, None, None, None, None, None) == 0  # empty batch


def test_struct_sizes_match_header_layout():
    assert C.sizeof(abi.EnvCfg) == 10 * 4 + 3 * 8
    assert C.sizeof(abi.TrackerWeights) == 8 * (7 + 12 * abi.MAX_TRACKER_LAYERS + 2)
    assert C.sizeof(abi.PpoCfg) == 17 * 4
    assert C.sizeof(abi.Traj) == 7 * 8
    # int32s incl. hidden[] | max_action, dropout_p | drop_env_base | padding to the 8-byte aligned dropout_seed | dropout_seed
    model = (7 + abi.VTB_RO_MAX_HIDDEN + 2) * 4 + 2 * 4 + 4 + 4 + 8
    assert C.sizeof(abi.VtbModelCfg) == model
    assert C.sizeof(abi.VtbRolloutCfg) == 5 * 4 + 4 + model + 8      # 4: padding in front of the 8-byte aligned model
    assert C.sizeof(abi.VtbLearnCfg) == 2 * 4 + model + 7 * 4 + 5 * 4 + 3 * 8 + 8 * 4


def _vtb_model(**kw):
    m = abi.VtbModelCfg(dim_model=27, nhead=3, d_hid=128, nlayers=2, dim_state=20, max_len=51, n_hidden=2,
                        hidden=(C.c_int32 * abi.VTB_RO_MAX_HIDDEN)(64, 64, 0), max_action=1.0)
    for k, v in kw.items():
        setattr(m, k, (C.c_int32 * abi.VTB_RO_MAX_HIDDEN)(*v) if k == "hidden" else v)
    return m


def _vtb_rollout_rc(model):
    """cirs_vtb_rollout_collect with every pointer null: argument validation ends it before any launch."""
    lib = abi.lib()
    cfg = abi.VtbRolloutCfg(n_env=4, max_turn=50, model=model)
    vc = abi.VtbCfg(n_env=4, max_turn=50, simulated=1)
    rc = lib.cirs_vtb_rollout_collect(C.byref(cfg), C.byref(abi.VtbPolicyWeights()), C.byref(vc), None, None, C.byref(abi.VtbTraj()), 0, 0, None)
    return rc, lib.cirs_last_error()


def _vtb_learn_rc(model):
    lib = abi.lib()
    cfg = abi.VtbLearnCfg(n_env=4, max_turn=50, n_rows=8, n_seg=1, model=model)
    out = (C.c_int64 * 5)()
    rc = lib.cirs_vtb_learn_sizes(C.byref(cfg), C.cast(out, C.c_void_p))
    return rc, lib.cirs_last_error()


def test_vtb_model_rules_are_checked_once_for_both_stages():
    # the model both stages accept: the learner sizes it, the rollout gets as far as its (null) weight pointers
    assert _vtb_learn_rc(_vtb_model())[0] == 0
    rc, msg = _vtb_rollout_rc(_vtb_model())
    assert rc == -1 and b"weight is null" in msg
    shared = [(dict(dim_model=24), b"dim_model must be 27"), (dict(nhead=4), b"nhead"), (dict(nhead=0), b"nhead"), (dict(nlayers=0), b"nlayers"),
              (dict(nlayers=5), b"nlayers"), (dict(max_len=50), b"max_turn"), (dict(n_hidden=0), b"hidden layers"),
              (dict(n_hidden=4), b"hidden layers"), (dict(hidden=(64, 129, 0)), b"widths"), (dict(hidden=(0, 64, 0)), b"widths"),
              (dict(dropout_p=1.0), b"dropout_p"), (dict(dropout_p=-0.1), b"dropout_p"), (dict(drop_env_base=-1), b"drop_env_base")]
    for kw, name in shared:
        for stage in (_vtb_rollout_rc, _vtb_learn_rc):
            rc, msg = stage(_vtb_model(**kw))
            assert rc == -1 and name in msg, (stage.__name__, kw, msg)
    # the capacity limits stay per stage: the rollout's are the tighter ones
    for kw, name in [(dict(d_hid=257), b"d_hid"), (dict(dim_state=65), b"dim_state"), (dict(max_len=683), b"nhead * max_len")]:
        rc, msg = _vtb_rollout_rc(_vtb_model(**kw))
        assert rc == -1 and name in msg, (kw, msg)
        assert _vtb_learn_rc(_vtb_model(**kw))[0] == 0, kw
    for kw, name in [(dict(d_hid=256), b"weight is null"), (dict(dim_state=64), b"weight is null"), (dict(max_len=682), b"weight is null")]:
        rc, msg = _vtb_rollout_rc(_vtb_model(**kw))
        assert rc == -1 and name in msg, (kw, msg)
    for kw, name in [(dict(d_hid=1025), b"d_hid"), (dict(d_hid=0), b"d_hid"), (dict(dim_state=129), b"dim_state"), (dict(dim_state=0), b"dim_state")]:
        rc, msg = _vtb_learn_rc(_vtb_model(**kw))
        assert rc == -1 and name in msg, (kw, msg)
    assert _vtb_learn_rc(_vtb_model(d_hid=1024, dim_state=128))[0] == 0
