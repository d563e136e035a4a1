"""GPU: the LSTM state tracker (csrc/lstm_tracker.hip) against the float64 restatement (cirs_hip/lstm_host.py): every state of every live
(env, position) through reset / init / step, the carried h and c, every gradient tensor of the back-propagation through time against
float64 autograd.  The replay (env_ids in descending order; skip on even steps, item -1 on odd ones) is the GRU tracker's test's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lstmcase
from cirs_hip import lstm_host
from test_gpu_gru_tracker import _backward, replay

pytestmark = pytest.mark.gpu
IDS = lstmcase.IDS


def host_states(p, users, acts, rews, lens, L, dtype):
    """states [B, T+1, S] and the carried (h, c) [L, B, D] of every env's last position, at `dtype`"""
    carried = {}
    s = lstm_host.states(lstm_host.cast_params(p, dtype), users, acts, rews, L, carried).numpy()
    b = np.arange(len(lens))
    return s, carried["h"].numpy()[:, b, lens - 1], carried["c"].numpy()[:, b, lens - 1]


@functools.lru_cache(maxsize=None)
def reference(ci):
    """Computed once per case and shared: parameters, inputs, the float64 states / carried tensors / gradients and the float32
    restatement's own error."""
    U, I, B, T, L, S, hot = lstmcase.CASES[ci]
    p = lstmcase.lstm_param_dict(U, I, seed=3, S=S, nlayers=L)
    users, acts, rews, lens, rng = lstmcase.teacher_inputs(U, I, B, T, hot)
    G = rng.normal(size=(T + 1, B, S)).astype(np.float32)
    s64, h64, c64 = host_states(p, users, acts, rews, lens, L, torch.float64)
    s32, h32, c32 = host_states(p, users, acts, rews, lens, L, torch.float32)
    live = np.arange(T + 1)[None, :] < lens[:, None]
    s_scale = np.abs(s64[live]).max()
    s_err32 = np.abs(s32[live] - s64[live]).max() / s_scale
    hc_err32 = {"h": float(np.abs(h32 - h64).max() / np.abs(h64).max()), "c": float(np.abs(c32 - c64).max() / np.abs(c64).max())}
    g64 = lstm_host.grads(p, users, acts, rews, lens, G, L, torch.float64)
    g32 = lstm_host.grads(p, users, acts, rews, lens, G, L, torch.float32)
    g_err32 = {k: float(np.abs(g32[k] - g64[k]).max() / (np.abs(g64[k]).max() + 1e-300)) for k in g64}
    return dict(p=p, users=users, acts=acts, rews=rews, lens=lens, G=G, s64=s64, h64=h64, c64=c64, live=live, s_scale=s_scale,
                s_err32=float(s_err32), hc_err32=hc_err32, g64=g64, g_err32=g_err32)


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("ci", range(len(lstmcase.CASES)), ids=IDS)
def test_lstm_states_match_float64_restatement(ci, mode):
    U, I, B, T, L, S, hot = lstmcase.CASES[ci]
    ref = reference(ci)
    trk, _ = lstmcase.device_lstm_trainable(ref["p"], U, I, B, T, L, S)
    got = replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], mode)
    live = ref["live"]
    assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
    np.testing.assert_array_equal(trk.len.cpu().numpy(), ref["lens"])
    err = np.abs(got[live] - ref["s64"][live]).max() / ref["s_scale"]
    bar = lstmcase.bar_for(lstmcase.STATE_BAR, ref["s_err32"])
    print(f"states {IDS[ci]} {mode}: device {err:.3e}  float32 restatement {ref['s_err32']:.3e}  bar {bar:.3e}")
    assert err <= bar
    # what every (layer, env) carries after the replay: the restatement's h and c of that env's last position
    for name in ("h", "c"):
        have, want = getattr(trk, name).cpu().numpy().astype(np.float64), ref[name + "64"]
        assert have.shape == want.shape == (L, B, 32)
        err = np.abs(have - want).max() / np.abs(want).max()
        bar = lstmcase.bar_for(lstmcase.STATE_BAR, ref["hc_err32"][name])
        print(f"carried {name} {IDS[ci]} {mode}: device {err:.3e}  float32 restatement {ref['hc_err32'][name]:.3e}  bar {bar:.3e}")
        assert err <= bar, name


@pytest.mark.parametrize("ci", range(len(lstmcase.CASES)), ids=IDS)
def test_lstm_backward_matches_float64_autograd(ci):
    U, I, B, T, L, S, hot = lstmcase.CASES[ci]
    ref = reference(ci)
    trk, _ = lstmcase.device_lstm_trainable(ref["p"], U, I, B, T, L, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    args = _backward(trk, ref, T, B, S)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    lens, acts = ref["lens"], ref["acts"]
    touched_items = np.unique(np.concatenate([acts[b, :lens[b] - 1] for b in range(B)]))
    touched_users = np.unique(ref["users"])
    assert {f"lstm.bias_{s}_l{l}" for s in ("ih", "hh") for l in range(L)} <= set(trk.grad_views)
    for k, gv in trk.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), ref["g64"][k]
        scale = np.abs(want).max() + 1e-300
        err = np.abs(got - want).max() / scale
        bar = lstmcase.bar_for(lstmcase.GRAD_BAR, ref["g_err32"][k])
        print(f"grad {IDS[ci]} {k}: device {err:.3e}  float32 restatement {ref['g_err32'][k]:.3e}  bar {bar:.3e}")
        assert err <= bar, k
    gi = trk.grad_views["embedding_dict.feat_item.weight"].cpu().numpy()
    gu = trk.grad_views["embedding_dict.feat_user.weight"].cpu().numpy()
    assert (np.delete(gi, touched_items, axis=0) == 0).all() and (np.delete(gu, touched_users, axis=0) == 0).all()
    # a second call: the same bits (fixed reduction orders, no atomics)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    assert torch.equal(trk.flat_grad, first)


def test_lstm_backward_refuses_a_short_workspace():
    from cirs_hip import abi
    U, I, B, T, L, S, hot = lstmcase.CASES[1]
    ref = reference(1)
    trk, _ = lstmcase.device_lstm_trainable(ref["p"], U, I, B, T, L, S)
    replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    users, traj, row_env, row_t, offsets, lens, n_rows, G = _backward(trk, ref, T, B, S)
    users = users.to("cuda", torch.int32)
    lib = abi.lib()
    need = lib.cirs_lstm_tracker_backward_workspace_bytes(C.byref(trk.cfg), n_rows)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(nbytes, stream):
        rc = lib.cirs_lstm_tracker_backward(C.byref(trk.cfg), C.byref(trk.w), C.byref(trk.st), users.data_ptr(), traj.act.data_ptr(), traj.rew.data_ptr(),
                                            row_env.data_ptr(), row_t.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n_rows, G.data_ptr(), C.byref(trk.g),
                                            ws.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        return rc
    trk.flat_grad.fill_(float("nan"))
    assert call(need - 1, None) != 0 and b"workspace too small" in lib.cirs_last_error()
    assert torch.isnan(trk.flat_grad).all(), "a refused call launched something"
    assert call(need, torch.cuda.current_stream().cuda_stream) == 0 and not torch.isnan(trk.flat_grad).any()


@pytest.mark.parametrize("B,L", [(3073, 1), (2049, 2)])
def test_lstm_states_when_a_wavefront_walks_several_envs(B, L):
    """One env more than 4 x workgroups-per-CU x CUs of a 256-CU part (3 per CU = 3072 with one layer, 2 per CU = 2048 with two): the launch
    then gives every wavefront two envs, and the last workgroup holds a single env.  Same bar as above."""
    U, I, T, S = 50, 80, 3, 20
    p = lstmcase.lstm_param_dict(U, I, seed=5, S=S, nlayers=L)
    users, acts, rews, lens, _ = lstmcase.teacher_inputs(U, I, B, T)
    s64, h64, c64 = host_states(p, users, acts, rews, lens, L, torch.float64)
    s32, _, _ = host_states(p, users, acts, rews, lens, L, torch.float32)
    live = np.arange(T + 1)[None, :] < lens[:, None]
    scale = np.abs(s64[live]).max()
    trk, _ = lstmcase.device_lstm_trainable(p, U, I, B, T, L, S)
    for mode in ("env_ids", "skip"):
        got = replay(trk, users, acts, rews, lens, mode)
        assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
        err, err32 = np.abs(got[live] - s64[live]).max() / scale, np.abs(s32[live] - s64[live]).max() / scale
        bar = lstmcase.bar_for(lstmcase.STATE_BAR, err32)
        print(f"states B={B} L={L} {mode}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar
