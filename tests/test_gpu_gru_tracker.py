"""GPU: the GRU state tracker (csrc/gru_tracker.hip) against the float64 restatement (cirs_hip/gru_host.py): every state of every live
(env, position) through reset / init / step, every gradient tensor of the back-propagation through time against float64 autograd."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grucase
from cirs_hip import gru_host

pytestmark = pytest.mark.gpu
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-L{c[4]}-S{c[5]}" + ("-hot" if c[6] else "") for c in grucase.CASES]


@functools.lru_cache(maxsize=None)
def reference(ci):
    """Computed once per case and shared: parameters, inputs, the float64 states / gradients and the float32 restatement's own error."""
    U, I, B, T, L, S, hot = grucase.CASES[ci]
    p = grucase.gru_param_dict(U, I, seed=3, S=S, nlayers=L)
    users, acts, rews, lens, rng = grucase.teacher_inputs(U, I, B, T, hot)
    G = rng.normal(size=(T + 1, B, S)).astype(np.float32)
    s64 = gru_host.states(gru_host.cast_params(p, torch.float64), users, acts, rews, L).numpy()
    s32 = gru_host.states(gru_host.cast_params(p, torch.float32), users, acts, rews, L).numpy()
    live = np.arange(T + 1)[None, :] < lens[:, None]
    s_scale = np.abs(s64[live]).max()
    s_err32 = np.abs(s32[live] - s64[live]).max() / s_scale
    g64 = gru_host.grads(p, users, acts, rews, lens, G, L, torch.float64)
    g32 = gru_host.grads(p, users, acts, rews, lens, G, L, torch.float32)
    g_err32 = {k: float(np.abs(g32[k] - g64[k]).max() / (np.abs(g64[k]).max() + 1e-300)) for k in g64}
    return dict(p=p, users=users, acts=acts, rews=rews, lens=lens, G=G, s64=s64, live=live, s_scale=s_scale, s_err32=float(s_err32), g64=g64,
                g_err32=g_err32)


def replay(trk, users, acts, rews, lens, mode):
    """reset / init / step, teacher-forced: env b gets positions 0 .. lens[b] - 1.  Finished envs are dropped through env_ids (the live rows
    only, in descending env order) or kept in the batch and marked (skip on even steps, item -1 on odd ones).  Returns states [B, T+1, S],
    NaN where no state was produced."""
    B, T = acts.shape
    S = trk.dim_state
    out = np.full((B, T + 1, S), np.nan, np.float32)
    trk.reset()
    out[:, 0] = trk.init(torch.as_tensor(users)).cpu().numpy()
    for t in range(T):
        live = np.where(lens > t + 1)[0]
        if len(live) == 0:
            break
        if mode == "env_ids":
            ids = live[::-1].copy()
            buf = torch.full((len(ids), S), float("nan"), device="cuda")
            trk.step(torch.as_tensor(acts[ids, t]), torch.as_tensor(rews[ids, t]), env_ids=torch.as_tensor(ids.astype(np.int32)).cuda(), out=buf,
                     out_stride=S)
            out[ids, t + 1] = buf.cpu().numpy()
        else:
            dead = lens <= t + 1
            buf = torch.full((B, S), float("nan"), device="cuda")      # the sentinel: rows of finished envs must keep it
            if t % 2 == 0:
                trk.step(torch.as_tensor(acts[:, t]), torch.as_tensor(rews[:, t]), skip=torch.as_tensor(dead.astype(np.uint8)).cuda(), out=buf, out_stride=S)
            else:
                trk.step(torch.as_tensor(np.where(dead, -1, acts[:, t])), torch.as_tensor(rews[:, t]), out=buf, out_stride=S)
            got = buf.cpu().numpy()
            assert np.isnan(got[dead]).all(), "a finished env's row of state_out was written"
            out[:, t + 1] = got
    return out


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(grucase.CASES)), ids=IDS)
def test_gru_states_match_float64_restatement(ci, mode):
    U, I, B, T, L, S, hot = grucase.CASES[ci]
    ref = reference(ci)
    trk, _ = grucase.device_gru_trainable(ref["p"], U, I, B, T, L, S)
    got = replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], mode)
    live = ref["live"]
    assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
    np.testing.assert_array_equal(trk.len.cpu().numpy(), ref["lens"])
    err = np.abs(got[live] - ref["s64"][live]).max() / ref["s_scale"]
    bar = grucase.bar_for(grucase.STATE_BAR, ref["s_err32"])
    print(f"states {IDS[ci]} {mode}: device {err:.3e}  float32 restatement {ref['s_err32']:.3e}  bar {bar:.3e}")
    assert err <= bar


def _backward(trk, ref, T, B, S):
    from cirs_hip.rollout import Trajectory
    lens, acts, rews = ref["lens"], ref["acts"], ref["rews"]
    traj = Trajectory(B, T, S, "cuda")
    a = np.where(np.arange(T)[None, :] < lens[:, None] - 1, acts, -1)      # position p reads action p - 1: lens - 1 actions per env
    traj.act.copy_(torch.as_tensor(a.T.copy())); traj.rew.copy_(torch.as_tensor(rews.T.copy()))
    offsets, row_env, row_t = grucase.rows_of(lens)
    d = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    args = (torch.as_tensor(ref["users"]), traj, d(row_env), d(row_t), d(offsets), d(lens.astype(np.int32)), int(lens.sum()), d(ref["G"]))
    return args


@pytest.mark.parametrize("ci", range(len(grucase.CASES)), ids=IDS)
def test_gru_backward_matches_float64_autograd(ci):
    U, I, B, T, L, S, hot = grucase.CASES[ci]
    ref = reference(ci)
    trk, _ = grucase.device_gru_trainable(ref["p"], U, I, B, T, L, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    args = _backward(trk, ref, T, B, S)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    lens, acts = ref["lens"], ref["acts"]
    touched_items = np.unique(np.concatenate([acts[b, :lens[b] - 1] for b in range(B)]))
    touched_users = np.unique(ref["users"])
    for k, gv in trk.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), ref["g64"][k]
        scale = np.abs(want).max() + 1e-300
        err = np.abs(got - want).max() / scale
        bar = grucase.bar_for(grucase.GRAD_BAR, ref["g_err32"][k])
        print(f"grad {IDS[ci]} {k}: device {err:.3e}  float32 restatement {ref['g_err32'][k]:.3e}  bar {bar:.3e}")
        assert err <= bar, k
    gi = trk.grad_views["embedding_dict.feat_item.weight"].cpu().numpy()
    gu = trk.grad_views["embedding_dict.feat_user.weight"].cpu().numpy()
    assert (np.delete(gi, touched_items, axis=0) == 0).all() and (np.delete(gu, touched_users, axis=0) == 0).all()
    # a second call: the same bits (fixed reduction orders, no atomics)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    assert torch.equal(trk.flat_grad, first)


def test_gru_backward_refuses_a_short_workspace():
    from cirs_hip import abi
    U, I, B, T, L, S, hot = grucase.CASES[0]
    ref = reference(0)
    trk, _ = grucase.device_gru_trainable(ref["p"], U, I, B, T, L, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    users, traj, row_env, row_t, offsets, lens, n_rows, G = _backward(trk, ref, T, B, S)
    users = users.to("cuda", torch.int32)
    lib = abi.lib()
    need = lib.cirs_gru_tracker_backward_workspace_bytes(C.byref(trk.cfg), n_rows)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    trk.flat_grad.fill_(float("nan"))
    rc = lib.cirs_gru_tracker_backward(C.byref(trk.cfg), C.byref(trk.w), C.byref(trk.st), users.data_ptr(), traj.act.data_ptr(), traj.rew.data_ptr(),
                                       row_env.data_ptr(), row_t.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n_rows, G.data_ptr(), C.byref(trk.g),
                                       ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc != 0 and b"workspace too small" in lib.cirs_last_error()
    assert torch.isnan(trk.flat_grad).all(), "a refused call launched something"
    rc = lib.cirs_gru_tracker_backward(C.byref(trk.cfg), C.byref(trk.w), C.byref(trk.st), users.data_ptr(), traj.act.data_ptr(), traj.rew.data_ptr(),
                                       row_env.data_ptr(), row_t.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n_rows, G.data_ptr(), C.byref(trk.g),
                                       ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and not torch.isnan(trk.flat_grad).any()


@pytest.mark.parametrize("B,L", [(4100, 1), (2060, 2)])
def test_gru_states_when_a_wavefront_walks_several_envs(B, L):
    """More envs than 4 x workgroups-per-CU x CUs of a 256-CU part (4096 with one layer, 2048 with two): the launch then gives every wavefront
    two envs, the last workgroups a ragged tail.  Same bar as above."""
    U, I, T, S = 50, 80, 3, 20
    p = grucase.gru_param_dict(U, I, seed=5, S=S, nlayers=L)
    users, acts, rews, lens, _ = grucase.teacher_inputs(U, I, B, T)
    s64 = gru_host.states(gru_host.cast_params(p, torch.float64), users, acts, rews, L).numpy()
    s32 = gru_host.states(gru_host.cast_params(p, torch.float32), users, acts, rews, L).numpy()
    live = np.arange(T + 1)[None, :] < lens[:, None]
    scale = np.abs(s64[live]).max()
    trk, _ = grucase.device_gru_trainable(p, U, I, B, T, L, S)
    for mode in ("env_ids", "skip"):
        got = replay(trk, users, acts, rews, lens, mode)
        assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
        err, err32 = np.abs(got[live] - s64[live]).max() / scale, np.abs(s32[live] - s64[live]).max() / scale
        bar = grucase.bar_for(grucase.STATE_BAR, err32)
        print(f"states B={B} L={L} {mode}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar
