"""GPU: the pooled-window state tracker (csrc/avg_tracker.hip) against the float64 restatement (cirs_hip/avg_host.py): every state of every
live (env, position) through reset / init / step, every gradient tensor of the backward against float64 autograd.  The replay (env_ids in
descending order; skip on even steps, item -1 on odd ones) is the GRU tracker's test's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import avgcase
from cirs_hip import avg_host
from test_gpu_gru_tracker import _backward, replay

pytestmark = pytest.mark.gpu
IDS = avgcase.IDS


def errors32(p, users, acts, rews, lens, W, T):
    """float64 states, the live mask, their scale and the float32 restatement's own error"""
    s64 = avg_host.states(avg_host.cast_params(p, torch.float64), users, acts, rews, W).numpy()
    s32 = avg_host.states(avg_host.cast_params(p, torch.float32), users, acts, rews, W).numpy()
    live = np.arange(T + 1)[None, :] < lens[:, None]
    scale = np.abs(s64[live]).max()
    return s64, live, scale, float(np.abs(s32[live] - s64[live]).max() / scale)


@functools.lru_cache(maxsize=None)
def reference(ci):
    """Computed once per case and shared: parameters, inputs, the float64 states / gradients and the float32 restatement's own error."""
    U, I, B, T, W, S, hot = avgcase.CASES[ci]
    p = avgcase.avg_param_dict(U, I, seed=3, S=S)
    users, acts, rews, lens, rng = avgcase.teacher_inputs(U, I, B, T, hot)
    G = rng.normal(size=(T + 1, B, S)).astype(np.float32)
    s64, live, s_scale, s_err32 = errors32(p, users, acts, rews, lens, W, T)
    g64 = avg_host.grads(p, users, acts, rews, lens, G, W, torch.float64)
    g32 = avg_host.grads(p, users, acts, rews, lens, G, W, torch.float32)
    g_err32 = {k: float(np.abs(g32[k] - g64[k]).max() / (np.abs(g64[k]).max() + 1e-300)) for k in g64}
    return dict(p=p, users=users, acts=acts, rews=rews, lens=lens, G=G, s64=s64, live=live, s_scale=s_scale, s_err32=s_err32, g64=g64, g_err32=g_err32)


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(avgcase.CASES)), ids=IDS)
def test_avg_states_match_float64_restatement(ci, mode):
    U, I, B, T, W, S, hot = avgcase.CASES[ci]
    ref = reference(ci)
    trk, _ = avgcase.device_avg_trainable(ref["p"], U, I, B, T, W, S)
    got = replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], mode)
    live = ref["live"]
    assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
    np.testing.assert_array_equal(trk.len.cpu().numpy(), ref["lens"])
    err = np.abs(got[live] - ref["s64"][live]).max() / ref["s_scale"]
    bar = avgcase.bar_for(avgcase.STATE_BAR, ref["s_err32"])
    print(f"states {IDS[ci]} {mode}: device {err:.3e}  float32 restatement {ref['s_err32']:.3e}  bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("ci", range(len(avgcase.CASES)), ids=IDS)
def test_avg_backward_matches_float64_autograd(ci):
    U, I, B, T, W, S, hot = avgcase.CASES[ci]
    ref = reference(ci)
    trk, _ = avgcase.device_avg_trainable(ref["p"], U, I, B, T, W, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    args = _backward(trk, ref, T, B, S)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    lens, acts = ref["lens"], ref["acts"]
    touched_items = np.unique(np.concatenate([acts[b, :lens[b] - 1] for b in range(B)]))
    touched_users = np.unique(ref["users"])
    assert set(trk.grad_views) == set(ref["g64"]) and len(trk.grad_views) == 8
    for k, gv in trk.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), ref["g64"][k]
        scale = np.abs(want).max() + 1e-300
        err = np.abs(got - want).max() / scale
        bar = avgcase.bar_for(avgcase.GRAD_BAR, ref["g_err32"][k])
        print(f"grad {IDS[ci]} {k}: device {err:.3e}  float32 restatement {ref['g_err32'][k]:.3e}  bar {bar:.3e}")
        assert err <= bar, k
    gi = trk.grad_views["embedding_dict.feat_item.weight"].cpu().numpy()
    gu = trk.grad_views["embedding_dict.feat_user.weight"].cpu().numpy()
    assert (np.delete(gi, touched_items, axis=0) == 0).all() and (np.delete(gu, touched_users, axis=0) == 0).all()
    # a second call: the same bits (fixed reduction orders, no atomics)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    assert torch.equal(trk.flat_grad, first)


def test_avg_backward_refuses_a_short_workspace():
    from cirs_hip import abi
    U, I, B, T, W, S, hot = avgcase.CASES[0]
    ref = reference(0)
    trk, _ = avgcase.device_avg_trainable(ref["p"], U, I, B, T, W, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    users, traj, row_env, row_t, offsets, lens, n_rows, G = _backward(trk, ref, T, B, S)
    users = users.to("cuda", torch.int32)
    lib = abi.lib()
    need = lib.cirs_avg_tracker_backward_workspace_bytes(C.byref(trk.cfg), n_rows)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(nbytes, stream):
        rc = lib.cirs_avg_tracker_backward(C.byref(trk.cfg), C.byref(trk.w), C.byref(trk.st), users.data_ptr(), traj.act.data_ptr(), traj.rew.data_ptr(),
                                           row_env.data_ptr(), row_t.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n_rows, G.data_ptr(), C.byref(trk.g),
                                           ws.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        return rc
    trk.flat_grad.fill_(float("nan"))
    assert call(need - 1, None) == -1 and b"workspace too small" in lib.cirs_last_error()
    assert torch.isnan(trk.flat_grad).all(), "a refused call launched something"
    assert call(need, torch.cuda.current_stream().cuda_stream) == 0 and not torch.isnan(trk.flat_grad).any()


def test_avg_states_when_a_workgroup_walks_several_envs():
    """More envs than 8 x workgroups-per-CU x CUs of a 256-CU part (4 per CU: 8192): the launch then gives every workgroup two groups of
    eight envs, the last workgroup a ragged tail.  T = 4 with W = 3: windows of one, two and three slots (the sliding is the cases' business
    above).  Same bar as above."""
    U, I, B, T, W, S = 50, 80, 8200, 4, 3, 20
    p = avgcase.avg_param_dict(U, I, seed=5, S=S)
    users, acts, rews, lens, _ = avgcase.teacher_inputs(U, I, B, T)
    s64, live, scale, err32 = errors32(p, users, acts, rews, lens, W, T)
    trk, _ = avgcase.device_avg_trainable(p, U, I, B, T, W, S)
    for mode in ("env_ids", "skip"):
        got = replay(trk, users, acts, rews, lens, mode)
        assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
        np.testing.assert_array_equal(trk.len.cpu().numpy(), lens)
        err = np.abs(got[live] - s64[live]).max() / scale
        bar = avgcase.bar_for(avgcase.STATE_BAR, err32)
        print(f"states B={B} W={W} {mode}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar
