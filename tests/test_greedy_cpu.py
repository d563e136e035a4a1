"""CPU: argument validation of the deterministic-evaluation entry points (no launch), and the float64 restatement the GPU tests compare
against, on hand-made cases."""
import ctypes as C

import numpy as np
import pytest

import greedycase
from cirs_hip import abi, policy_host


def _policy(n_items=130, **kw):
    cfg = abi.PolicyCfg(n_items=n_items, dim_state=20, hidden=64)
    for k, v in kw.items():
        setattr(cfg, k, v)
    w = abi.PolicyWeights(**{k: 8 for k in ("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc")})   # non-null, never dereferenced on the host
    return cfg, w


def _err():
    return abi.lib().cirs_last_error()


def test_actor_greedy_validates_before_any_launch():
    lib = abi.lib()
    cfg, w = _policy()
    assert lib.cirs_actor_greedy(None, None, 8, 20, 4, None, None, None, 8, None, None, 8, 1 << 30, None) == -1 and b"null" in _err()
    assert lib.cirs_actor_greedy(C.byref(cfg), C.byref(abi.PolicyWeights()), 8, 20, 4, None, None, None, 8, None, None, 8, 1 << 30, None) == -1
    assert b"weight pointer null" in _err()
    assert lib.cirs_actor_greedy(C.byref(cfg), C.byref(w), None, 20, 4, None, None, None, 8, None, None, 8, 1 << 30, None) == -1 and b"null" in _err()
    assert lib.cirs_actor_greedy(C.byref(cfg), C.byref(w), 8, 20, 4, None, None, None, None, None, None, 8, 1 << 30, None) == -1 and b"null" in _err()
    assert lib.cirs_actor_greedy(C.byref(cfg), C.byref(w), 8, 19, 4, None, None, None, 8, None, None, 8, 1 << 30, None) == -1 and b"state_stride" in _err()
    need = lib.cirs_policy_workspace_bytes(C.byref(cfg), 4)
    assert lib.cirs_actor_greedy(C.byref(cfg), C.byref(w), 8, 20, 4, None, None, None, 8, None, None, 8, need - 1, None) == -1
    assert b"workspace too small" in _err()
    bad, _ = _policy(hidden=32)
    assert lib.cirs_actor_greedy(C.byref(bad), C.byref(w), 8, 20, 4, None, None, None, 8, None, None, 8, 1 << 30, None) != 0
    assert lib.cirs_actor_greedy(C.byref(cfg), C.byref(w), None, 20, 0, None, None, None, None, None, None, None, 0, None) == 0     # empty batch


def test_actor_topk_validates_before_any_launch():
    lib = abi.lib()
    cfg, w = _policy(300)
    call = lambda k, ws_bytes, state=8, ids=8, ws=8, n=5: lib.cirs_actor_topk(C.byref(cfg), C.byref(w), state, 20, n, k, None, None, None, ids, None,
                                                                              ws, ws_bytes, None)      # noqa: E731
    for k in (0, 33, -1):
        assert call(k, 1 << 30) == -1 and b"k must lie in 1..32" in _err(), k
        assert lib.cirs_actor_topk_workspace_bytes(C.byref(cfg), 5, k) == 0
    need = lib.cirs_actor_topk_workspace_bytes(C.byref(cfg), 5, 7)
    # the greedy scratch plus one float per (item of a whole 32-item tile, padded row)
    assert need >= lib.cirs_policy_workspace_bytes(C.byref(cfg), 5) + 10 * 32 * 32 * 4
    assert call(7, need - 1) == -1 and b"workspace too small" in _err()
    assert call(7, need, state=None) == -1 and b"null" in _err()
    assert call(7, need, ids=None) == -1 and b"null" in _err()
    assert call(7, need, ws=None) == -1 and b"null" in _err()
    assert lib.cirs_actor_topk(None, None, 8, 20, 5, 7, None, None, None, 8, None, 8, need, None) == -1
    assert call(7, 0, n=0) == 0
    assert lib.cirs_actor_topk_workspace_bytes(None, 5, 7) == 0 and lib.cirs_actor_topk_workspace_bytes(C.byref(cfg), 0, 7) == 0


def test_greedy_rollouts_validate_before_any_launch():
    lib = abi.lib()
    ecfg = abi.EnvCfg(n_users=3, n_items=130, max_turn=5, num_leave_compute=1, leave_threshold=0, version=1, simulated=1)
    assert lib.cirs_rollout_steps_greedy(C.byref(ecfg), None, None, None, None, None, None, None, None, 4, 0, 5, None, 0, None, 0, None) == -1
    assert b"null" in _err()
    assert lib.cirs_rollout_collect_greedy(C.byref(ecfg), None, None, None, None, None, None, None, None, 4, None, None, 0, None, 0, None) == -1
    assert b"null" in _err()
    # tables set up for the online-reward loop are refused with a message
    tab = abi.EnvTables(pred_online=8)
    assert lib.cirs_rollout_steps_greedy(C.byref(ecfg), C.byref(tab), None, None, None, None, None, None, None, 4, 0, 5, None, 0, None, 0, None) == -1
    assert b"online-reward loop has no greedy mode" in _err()
    st = abi.EnvState()
    assert lib.cirs_rollout_collect_greedy(C.byref(ecfg), C.byref(tab), C.byref(st), None, None, None, None, None, None, 4, 8, None, 0, 8, 1 << 20,
                                           None) == -1
    assert b"online-reward loop has no greedy mode" in _err()
    # a bad step range, as in the sampled rollout
    tab = abi.EnvTables()
    args = [C.byref(x) for x in (abi.EnvState(), abi.TrackerCfg(), abi.TrackerWeights(), abi.TrackerState(), abi.PolicyCfg(), abi.PolicyWeights())]
    traj = abi.Traj(**{k: 8 for k in ("obs", "act", "rew", "done", "logp", "value", "ctr")})
    assert lib.cirs_rollout_steps_greedy(C.byref(ecfg), C.byref(tab), *args, C.byref(traj), 4, 0, 6, None, 0, 8, 1 << 20, None) == -1
    assert b"bad step range" in _err()


def test_vtb_greedy_collect_validates_before_any_launch():
    lib = abi.lib()
    model = abi.VtbModelCfg(dim_model=27, nhead=3, d_hid=128, nlayers=2, dim_state=20, max_len=51, n_hidden=2,
                            hidden=(C.c_int32 * abi.VTB_RO_MAX_HIDDEN)(64, 64, 0), max_action=1.0)
    cfg = abi.VtbRolloutCfg(n_env=4, max_turn=50, model=model)
    vc = abi.VtbCfg(n_env=4, max_turn=50, simulated=1)
    assert lib.cirs_vtb_rollout_collect_greedy(None, None, None, None, None, None, None, None) == -1 and b"null" in _err()
    rc = lib.cirs_vtb_rollout_collect_greedy(C.byref(cfg), C.byref(abi.VtbPolicyWeights()), C.byref(vc), None, None, C.byref(abi.VtbTraj()), None, None)
    assert rc == -1 and b"weight is null" in _err()
    cfg.model.max_len = 2000                                   # the exact-redraw limits apply when its workspace is given
    rc = lib.cirs_vtb_rollout_collect_greedy(C.byref(cfg), C.byref(abi.VtbPolicyWeights()), C.byref(vc), None, None, C.byref(abi.VtbTraj()), 8, None)
    assert rc == -1 and b"dropout_redraw" in _err()


def test_python_layer_refuses_what_is_out_of_scope():
    from cirs_hip.engine import CirsEngine
    from cirs_hip.rollout import DeviceRollout
    ro = object.__new__(DeviceRollout)
    ro.online = None
    with pytest.raises(ValueError, match="gumbel"):
        ro._check_greedy(np.zeros(3, np.float32))
    ro.online = object()
    with pytest.raises(NotImplementedError, match="online-reward"):
        ro._check_greedy(None)
    eng = object.__new__(CirsEngine)
    eng.world, eng.dropout_redraw, eng.rollout = 2, False, ro
    with pytest.raises(NotImplementedError, match="one rank"):
        eng.collect(greedy=True)
    eng.world, eng.dropout_redraw = 1, True
    with pytest.raises(NotImplementedError, match="exact-redraw"):
        eng.collect(greedy=True)
    eng.dropout_redraw = False
    with pytest.raises(NotImplementedError, match="online-reward"):
        eng.collect(greedy=True)
    from cirs_hip.policy import DevicePolicy
    pol = object.__new__(DevicePolicy)
    for k in (0, 33):
        with pytest.raises(ValueError, match="1..32"):
            pol.topk(None, k)


# ---- the float64 restatement on hand-made cases --------------------------------------------------------------------------------
def test_restatement_ties_go_to_the_lowest_id():
    z = np.array([[0.5, 2.0, 2.0, -1.0, 2.0], [1.0, 1.0, 1.0, 1.0, 1.0]])
    ids, logp, gaps = policy_host.topk_from_logits(z, 3)
    assert ids.tolist() == [[1, 2, 4], [0, 1, 2]]
    assert gaps[0].tolist() == [0.0, 0.0, 1.5] and gaps[1].tolist() == [0.0, 0.0, 0.0]
    np.testing.assert_allclose(logp[1], np.log(0.2), rtol=1e-12)
    np.testing.assert_allclose(np.exp(logp[0]), np.exp(2.0) / np.exp(z[0]).sum(), rtol=1e-12)


def test_restatement_excludes_masked_items_and_fills_short_lists():
    z = np.array([[3.0, 2.0, 1.0, 0.0, -1.0, 5.0]] * 3)
    masked = np.zeros((3, 6), bool)
    masked[0, [0, 5]] = True                    # the two best are gone
    masked[1, [0, 1, 2, 5]] = True              # two items left
    ids, logp, gaps = policy_host.topk_from_logits(z, 4, masked, skip=np.array([0, 0, 1]))
    assert ids[0].tolist() == [1, 2, 3, 4]
    np.testing.assert_allclose(np.exp(logp[0]).sum(), 1.0, rtol=1e-12)      # the soft-max runs over the unmasked items only
    assert ids[1].tolist() == [3, 4, -1, -1] and np.isneginf(logp[1, 2:]).all() and np.isfinite(logp[1, :2]).all()
    assert gaps[1, 0] == 1.0 and np.isinf(gaps[1, 1:]).all()
    assert ids[2].tolist() == [-1] * 4 and np.isneginf(logp[2]).all()       # skipped row
    # the clamp of torch's probs_to_logits
    ids, logp, _ = policy_host.topk_from_logits(np.array([[0.0, 100.0]]), 2)
    np.testing.assert_allclose(logp[0], [np.log(1 - policy_host.EPS32), np.log(policy_host.EPS32)], rtol=1e-12)


def test_restatement_reads_the_bitmap_by_env_id():
    bm = np.zeros((3, 2), np.uint32)
    bm[2, 0] = 1 << 5
    bm[0, 1] = 1 << 1
    m = policy_host.mask_from_bitmap(bm, np.array([2, 0]), 2, 40)
    assert np.flatnonzero(m[0]).tolist() == [5] and np.flatnonzero(m[1]).tolist() == [33]


@pytest.mark.parametrize("masked", [False, True])
def test_the_gpu_cases_have_no_row_inside_the_margin(masked):
    """The share of rows whose float64 top-2 gap is inside the margin is a condition on the inputs: none on the seeds the GPU tests use."""
    for n in greedycase.ROWS:
        for I in greedycase.CATALOGUES:
            c = greedycase.case(n, I, masked)
            act, logp, value, gap, ru = policy_host.greedy64(c["arrs"], c["state"], c["env_ids"], c["visited"], c["skip"])
            z, _ = policy_host.forward64(c["arrs"], c["state"])
            live = act >= 0
            assert live.sum() == n - (0 if c["skip"] is None else int(c["skip"].sum()))
            assert (gap[live] > greedycase.margin_of(z[np.flatnonzero(live), act[live]])).all(), (n, I, masked, gap[live].min())
            if masked:
                mk = policy_host.mask_from_bitmap(c["visited"], c["env_ids"], n, I)
                assert 0.25 < mk[:-1].mean() < 0.35 if n > 1 else True
                assert (~mk[n - 1]).sum() == 3 and not mk[np.flatnonzero(live), act[live]].any()
