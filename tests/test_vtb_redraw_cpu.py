"""CPU: the host side of the exact-redraw tracker dropout of the device VirtualTaobao path (dropout_redraw=True).  (a) The keyword is routed:
Collector(..., rollout="device", dropout_redraw=True) builds a DeviceVtbCollector with the option on, and it is refused without
rollout="device" or with a non-bool value.  (b) vtb_host.redraw_states -- one causal pass per call with that call's masks -- equals
tracker_states without dropout, and a call's masks change that call's state only.  (c) The new entry points validate on the host."""
import ctypes as C

import pytest
import torch

import vtbrolloutcase as case
from test_vtb_rollout_cpu import _tracker


def _taobao(golden_dir, device, n=3, T=5):
    env, base = case.venv(golden_dir, n, True, T, device=device)
    tracker, actor, critic, policy = case.stack(base, n, T, dropout=0.1)
    return env, tracker, policy


def test_redraw_collector_is_selected_by_the_keyword(golden_dir):
    from core.collector import Collector
    from core.vtb_collector import DeviceVtbCollector
    env, tracker, policy = _taobao(golden_dir, "cuda")
    c = Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="device", dropout_redraw=True)
    assert isinstance(c, DeviceVtbCollector) and c.dropout_redraw is True
    assert c._rollout is None                      # nothing touches the GPU before collect
    off = Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="device")
    assert off.dropout_redraw is False
    with pytest.raises(TypeError, match="dropout_redraw must be a bool"):
        Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="device", dropout_redraw="yes")
    with pytest.raises(TypeError, match="dropout_redraw must be a bool"):
        Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="device", dropout_redraw=1)


def test_redraw_without_the_device_rollout_is_refused(golden_dir):
    from core.collector import Collector
    from core.host_rl import HostCollector
    env, tracker, policy = _taobao(golden_dir, None)
    with pytest.raises(ValueError, match="rollout='device'"):
        Collector(policy, env, None, preprocess_fn=tracker.build_state, dropout_redraw=True)
    assert type(Collector(policy, env, None, preprocess_fn=tracker.build_state, dropout_redraw=False)) is HostCollector


def _ones(B, n_pos):
    from cirs_hip import vtb_host
    m = {"pos": torch.ones(B, n_pos, 27)}
    for l in range(2):
        m.update({(l, vtb_host.DROP_ATTN): torch.ones(B, n_pos, n_pos * 3), (l, vtb_host.DROP_RES1): torch.ones(B, n_pos, 27),
                  (l, vtb_host.DROP_FF): torch.ones(B, n_pos, 128), (l, vtb_host.DROP_RES2): torch.ones(B, n_pos, 27)})
    return m


def _inputs(T, B):
    g = torch.Generator().manual_seed(0)
    return (torch.rand(B, 88, generator=g) < 0.1).float(), torch.rand(T, B, generator=g) * 3, torch.randn(T, B, 27, generator=g)


def test_redraw_states_with_unit_masks_equal_tracker_states():
    from cirs_hip import vtb_host
    T, B = 12, 5
    tr = _tracker(T)
    user, rew, act = _inputs(T, B)
    with torch.no_grad():
        want = vtb_host.tracker_states(tr, user, rew, act)
        got = vtb_host.redraw_states(tr, user, rew, act, lambda c: _ones(B, c + 1))
        plain = vtb_host.redraw_states(tr, user, rew, act)
    assert got.shape == (T + 1, B, 20)
    torch.testing.assert_close(got, want, rtol=0, atol=0)
    torch.testing.assert_close(plain, want, rtol=0, atol=0)


def test_redraw_states_masks_of_a_call_touch_that_call_only():
    from cirs_hip import vtb_host
    T, B = 6, 3
    tr = _tracker(T)
    user, rew, act = _inputs(T, B)

    def masks(variant):
        def of_call(c):
            m = _ones(B, c + 1)
            if c == 3:                                  # call 3 drops one element of position 1's feed-forward, another per variant
                m[(0, vtb_host.DROP_FF)][:, 1, 7 + variant] = 0.0
            return m
        return of_call

    with torch.no_grad():
        a = vtb_host.redraw_states(tr, user, rew, act, masks(0))
        b = vtb_host.redraw_states(tr, user, rew, act, masks(1))
        base = vtb_host.tracker_states(tr, user, rew, act)
    torch.testing.assert_close(a[:3], b[:3], rtol=0, atol=0)
    torch.testing.assert_close(a[4:], b[4:], rtol=0, atol=0)       # later calls run the prefix again with masks of their own
    torch.testing.assert_close(a[4:], base[4:], rtol=0, atol=0)
    assert float((a[3] - b[3]).abs().max()) > 1e-6
    assert float((a[3] - base[3]).abs().max()) > 1e-6


def test_redraw_states_keep_a_graph_per_call():
    from cirs_hip import vtb_host
    T, B = 4, 2
    tr = _tracker(T)
    user, rew, act = _inputs(T, B)
    st = vtb_host.redraw_states(tr, user, rew, act, lambda c: _ones(B, c + 1))
    st[2].sum().backward()
    for name in ("ffn_user", "fnn_gate", "decoder"):
        assert float(getattr(tr, name).weight.grad.abs().sum()) > 0, name


# ---- entry points -----------------------------------------------------------------------------------------------------------------
def _model(abi, **kw):
    m = abi.VtbModelCfg(dim_model=27, nhead=3, d_hid=128, nlayers=2, dim_state=20, max_len=51, n_hidden=2,
                        hidden=(C.c_int32 * abi.VTB_RO_MAX_HIDDEN)(64, 64, 0), max_action=1.0, dropout_p=0.1)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_redraw_entry_points_reject_bad_arguments():
    from cirs_hip import abi
    lib = abi.lib()
    err = lambda: lib.cirs_last_error().decode()
    fake = 0x2000            # never dereferenced: validation ends every call below before a launch
    pw = abi.VtbPolicyWeights()
    tr = abi.VtbTraj()
    vc = abi.VtbCfg(n_env=4, max_turn=50, simulated=1)

    def collect(cfg, ws=fake, w=pw, traj=tr):
        return lib.cirs_vtb_rollout_collect_redraw(cfg and C.byref(cfg), C.byref(w), C.byref(vc), None, None, C.byref(traj), ws, 0, 0, None)

    assert collect(None) == -1 and "null" in err()
    assert collect(abi.VtbRolloutCfg(n_env=4, max_turn=50, model=_model(abi))) == -1 and "weight is null" in err()
    big = abi.VtbRolloutCfg(n_env=4, max_turn=50, model=_model(abi, drop_env_base=2 ** 31 - 51 * 4))
    assert collect(big) == -1 and "2^31" in err()
    ok = abi.VtbRolloutCfg(n_env=4, max_turn=50, model=_model(abi, drop_env_base=2 ** 31 - 51 * 4 - 1))
    assert collect(ok) == -1 and "weight is null" in err()
    assert collect(abi.VtbRolloutCfg(n_env=4, max_turn=362, model=_model(abi, max_len=363))) == -1 and "1088" in err()
    # every weight and buffer present, the workspace missing
    full_w = abi.VtbPolicyWeights()
    for k, _ in abi.VtbPolicyWeights._fields_:
        if k == "layer":
            for l in range(abi.VTB_RO_MAX_LAYERS):
                for f in abi.VTB_LAYER_FIELDS:
                    setattr(full_w.layer[l], f, fake)
        elif k.startswith("trunk"):
            for i in range(abi.VTB_RO_MAX_HIDDEN):
                getattr(full_w, k)[i] = fake
        else:
            setattr(full_w, k, fake)
    full_tr = abi.VtbTraj(**{k: fake for k in abi.VTB_TRAJ_FIELDS})
    cfg = abi.VtbRolloutCfg(n_env=4, max_turn=50, model=_model(abi))
    assert collect(cfg, w=full_w, traj=full_tr) == -1 and "env weights" in err()
    rc = lib.cirs_vtb_rollout_collect_redraw(C.byref(cfg), C.byref(full_w), C.byref(vc), C.byref(abi.VtbWeights()), C.byref(abi.VtbState()),
                                             C.byref(full_tr), None, 0, 0, None)
    assert rc == -1 and "null workspace" in err()

    # learner
    out = (C.c_int64 * 5)()
    lc = lambda **kw: abi.VtbLearnCfg(n_env=4, max_turn=50, n_rows=8, n_seg=1, model=_model(abi, **kw))
    assert lib.cirs_vtb_learn_redraw_sizes(None, C.cast(out, C.c_void_p)) == -1 and "null learn cfg" in err()
    assert lib.cirs_vtb_learn_redraw_sizes(C.byref(lc()), None) == -1 and "null output" in err()
    assert lib.cirs_vtb_learn_redraw_sizes(C.byref(lc(drop_env_base=2 ** 31 - 51 * 4)), C.cast(out, C.c_void_p)) == -1 and "2^31" in err()
    assert lib.cirs_vtb_learn_redraw_sizes(C.byref(lc()), C.cast(out, C.c_void_p)) == 0
    redraw_ws = out[2]
    plain = (C.c_int64 * 5)()
    assert lib.cirs_vtb_learn_sizes(C.byref(lc()), C.cast(plain, C.c_void_p)) == 0
    assert list(out[:2]) == list(plain[:2]) and redraw_ws > plain[2]          # same images, one workspace and slab per tracker workgroup
    assert lib.cirs_vtb_learn_redraw_sizes(C.byref(lc(dropout_p=0.0)), C.cast(out, C.c_void_p)) == 0 and list(out) == list(plain)
    for fn in (lib.cirs_vtb_learn_prepare_redraw,
               lambda c, b, s: lib.cirs_vtb_learn_update_redraw(c, b, None, 1, 8, 0, 0, 0, s)):
        assert fn(None, C.byref(abi.VtbLearnBufs()), None) == -1 and "null learn cfg" in err()
        assert fn(C.byref(lc()), None, None) == -1 and "null learn buffer" in err()
        assert fn(C.byref(lc()), C.byref(abi.VtbLearnBufs()), None) == -1 and "null learn buffer" in err()
        assert fn(C.byref(lc(drop_env_base=2 ** 31 - 51 * 4)), C.byref(abi.VtbLearnBufs()), None) == -1 and "2^31" in err()
    bufs = abi.VtbLearnBufs(**{k: fake for k in abi.VTB_LEARN_BUF_FIELDS if k != "losses"})
    assert lib.cirs_vtb_learn_update_redraw(C.byref(lc()), C.byref(bufs), None, 1, 8, 0, 0, 0, None) == -1 and "permutations" in err()
