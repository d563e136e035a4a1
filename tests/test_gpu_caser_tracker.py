"""GPU: the convolutional window state tracker (csrc/caser_tracker.hip) against the float64 restatement (cirs_hip/caser_host.py): every state of
every live (env, position) through reset / init / step, every gradient tensor of the backward against float64 autograd.  The replay (env_ids
in descending order; skip on even steps, item -1 on odd ones) is the GRU tracker's test's.  The cases' inputs are ones where float64 itself is
unambiguous at every max and ReLU (tests/test_caser_host_cpu.py checks that on the CPU): no case and no element is skipped or masked here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import casercase
from cirs_hip import caser_host
from test_gpu_gru_tracker import _backward, replay

pytestmark = pytest.mark.gpu
IDS = casercase.IDS
WALK_SEED = 5      # parameter seed of the many-env test


def errors32(p, users, acts, rews, lens, W, T):
    """float64 states, the live mask, their scale and the float32 restatement's own error"""
    s64 = caser_host.states(caser_host.cast_params(p, torch.float64), users, acts, rews, W).numpy()
    s32 = caser_host.states(caser_host.cast_params(p, torch.float32), users, acts, rews, W).numpy()
    live = np.arange(T + 1)[None, :] < lens[:, None]
    scale = np.abs(s64[live]).max()
    return s64, live, scale, float(np.abs(s32[live] - s64[live]).max() / scale)


@functools.lru_cache(maxsize=None)
def reference(ci):
    """Computed once per case and shared: parameters, inputs, the float64 states / gradients and the float32 restatement's own error."""
    U, I, B, T, W, heights, S, hot = casercase.CASES[ci]
    p = casercase.case_params(ci)
    users, acts, rews, lens, rng = casercase.teacher_inputs(U, I, B, T, hot)
    G = rng.normal(size=(T + 1, B, S)).astype(np.float32)
    s64, live, s_scale, s_err32 = errors32(p, users, acts, rews, lens, W, T)
    g64 = caser_host.grads(p, users, acts, rews, lens, G, W, torch.float64)
    g32 = caser_host.grads(p, users, acts, rews, lens, G, W, torch.float32)
    g_err32 = {k: float(np.abs(g32[k] - g64[k]).max() / (np.abs(g64[k]).max() + 1e-300)) for k in g64}
    return dict(p=p, users=users, acts=acts, rews=rews, lens=lens, G=G, s64=s64, live=live, s_scale=s_scale, s_err32=s_err32, g64=g64, g_err32=g_err32)


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(casercase.CASES)), ids=IDS)
def test_caser_states_match_float64_restatement(ci, mode):
    U, I, B, T, W, heights, S, hot = casercase.CASES[ci]
    ref = reference(ci)
    trk, _ = casercase.device_caser_trainable(ref["p"], U, I, B, T, W, heights, S)
    got = replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], mode)
    live = ref["live"]
    assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
    np.testing.assert_array_equal(trk.len.cpu().numpy(), ref["lens"])
    err = np.abs(got[live] - ref["s64"][live]).max() / ref["s_scale"]
    bar = casercase.bar_for(casercase.STATE_BAR, ref["s_err32"])
    print(f"states {IDS[ci]} {mode}: device {err:.3e}  float32 restatement {ref['s_err32']:.3e}  bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("ci", range(len(casercase.CASES)), ids=IDS)
def test_caser_backward_matches_float64_autograd(ci):
    U, I, B, T, W, heights, S, hot = casercase.CASES[ci]
    ref = reference(ci)
    trk, _ = casercase.device_caser_trainable(ref["p"], U, I, B, T, W, heights, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    args = _backward(trk, ref, T, B, S)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    lens, acts = ref["lens"], ref["acts"]
    touched_items = np.unique(np.concatenate([acts[b, :lens[b] - 1] for b in range(B)]))
    touched_users = np.unique(ref["users"])
    assert set(trk.grad_views) == set(ref["g64"]) and len(trk.grad_views) == 12 + 2 * len(heights)
    for k, gv in trk.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), ref["g64"][k]
        scale = np.abs(want).max() + 1e-300
        err = np.abs(got - want).max() / scale
        bar = casercase.bar_for(casercase.GRAD_BAR, ref["g_err32"][k])
        print(f"grad {IDS[ci]} {k}: device {err:.3e}  float32 restatement {ref['g_err32'][k]:.3e}  bar {bar:.3e}")
        assert err <= bar, k
    gi = trk.grad_views["embedding_dict.feat_item.weight"].cpu().numpy()
    gu = trk.grad_views["embedding_dict.feat_user.weight"].cpu().numpy()
    assert (np.delete(gi, touched_items, axis=0) == 0).all() and (np.delete(gu, touched_users, axis=0) == 0).all()
    # a second call: the same bits (fixed reduction orders, no atomics)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    assert torch.equal(trk.flat_grad, first)


def test_caser_backward_refuses_a_short_workspace():
    from cirs_hip import abi
    U, I, B, T, W, heights, S, hot = casercase.CASES[0]
    ref = reference(0)
    trk, _ = casercase.device_caser_trainable(ref["p"], U, I, B, T, W, heights, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    users, traj, row_env, row_t, offsets, lens, n_rows, G = _backward(trk, ref, T, B, S)
    users = users.to("cuda", torch.int32)
    lib = abi.lib()
    need = lib.cirs_caser_tracker_backward_workspace_bytes(C.byref(trk.cfg), n_rows)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(nbytes, stream):
        rc = lib.cirs_caser_tracker_backward(C.byref(trk.cfg), C.byref(trk.w), C.byref(trk.st), users.data_ptr(), traj.act.data_ptr(), traj.rew.data_ptr(),
                                           row_env.data_ptr(), row_t.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n_rows, G.data_ptr(), C.byref(trk.g),
                                           ws.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        return rc
    trk.flat_grad.fill_(float("nan"))
    assert call(need - 1, None) == -1 and b"workspace too small" in lib.cirs_last_error()
    assert torch.isnan(trk.flat_grad).all(), "a refused call launched something"
    assert call(need, torch.cuda.current_stream().cuda_stream) == 0 and not torch.isnan(trk.flat_grad).any()


def test_caser_states_when_a_workgroup_walks_several_envs():
    """More envs than 4 x workgroups-per-CU x CUs of a 256-CU part (2 per CU: 2048): the launch then gives every workgroup two groups of four
    envs, the last workgroup a ragged tail.  T = 4 with W = 3 and heights (1, 3): windows with three, two, one and no zero rows (the sliding
    is the cases' business above).  Same bar as above.  States only: they are continuous at every max and ReLU, so the near-tie condition of
    the gradient tests is not needed here."""
    U, I, B, T, W, heights, S = 50, 80, 2056, 4, 3, (1, 3), 20
    p = casercase.caser_param_dict(U, I, WALK_SEED, W, heights, S=S)
    users, acts, rews, lens, _ = casercase.teacher_inputs(U, I, B, T)
    s64, live, scale, err32 = errors32(p, users, acts, rews, lens, W, T)
    trk, _ = casercase.device_caser_trainable(p, U, I, B, T, W, heights, S)
    for mode in ("env_ids", "skip"):
        got = replay(trk, users, acts, rews, lens, mode)
        assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
        np.testing.assert_array_equal(trk.len.cpu().numpy(), lens)
        err = np.abs(got[live] - s64[live]).max() / scale
        bar = casercase.bar_for(casercase.STATE_BAR, err32)
        print(f"states B={B} W={W} {mode}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar
