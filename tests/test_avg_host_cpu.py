"""CPU: the host restatement of the pooled-window tracker (cirs_hip/avg_host.py) gives the known answers, equals the cumulative-sum
formulation, its autograd equals the closed-form window backward the device kernel implements; StateTrackerAvg and the library refuse
what is not built before they touch a device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import avgcase
from cirs_hip import avg_host
from cirs_hip.avg_tracker import avg_param_shapes, init_avg_tracker_params


@pytest.mark.parametrize("W,want", [(2, [1.0, 3.0, 3.5, 4.5]), (1, [1.0, 3.0, 4.0, 5.0])])
def test_known_answers(W, want):
    B, L, D = 2, 4, 32
    p = {"decoder.weight": torch.eye(D, dtype=torch.float64), "decoder.bias": torch.zeros(D, dtype=torch.float64)}
    X = (torch.arange(L, dtype=torch.float64) + 1)[None, :, None].expand(B, L, D).contiguous()
    s = avg_host.states_from_slots(p, X, W).numpy()
    assert s.shape == (B, L, D)
    for t in range(L):
        assert (s[:, t] == want[t]).all(), (t, s[0, t, 0])


def _case(ci):
    U, I, B, T, W, S, hot = avgcase.CASES[ci]
    p = avg_host.cast_params(avgcase.avg_param_dict(U, I, seed=3, S=S), torch.float64)
    users, acts, rews, lens, rng = avgcase.teacher_inputs(U, I, B, T, hot)
    return p, avg_host.input_slots(p, users, acts, rews), lens, rng


@pytest.mark.parametrize("ci", range(len(avgcase.CASES)), ids=avgcase.IDS)
def test_restatement_equals_the_cumulative_sum_formulation(ci):
    U, I, B, T, W, S, hot = avgcase.CASES[ci]
    p, X, lens, _ = _case(ci)
    got = avg_host.states_from_slots(p, X, W).numpy()
    x = X.numpy()
    c = np.concatenate([np.zeros((B, 1, 32)), np.cumsum(x[:, 1:], axis=1)], axis=1)      # c_p = x_1 + ... + x_p, c_0 = 0
    h = np.empty_like(x)
    for t in range(T + 1):
        n = min(W, t)
        h[:, t] = x[:, 0] + ((c[:, t] - c[:, t - n]) / n if t else 0.0)
    want = h @ p["decoder.weight"].numpy().T + p["decoder.bias"].numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("ci", range(len(avgcase.CASES)), ids=avgcase.IDS)
def test_closed_form_window_backward_equals_autograd(ci):
    """dX[b,0] = sum_p dH[b,p];  dX[b,k] = sum_{p=k}^{min(len-1, k+W-1)} dH[b,p] / n_p -- what avg_window_bwd computes."""
    U, I, B, T, W, S, hot = avgcase.CASES[ci]
    p, X, lens, rng = _case(ci)
    G = rng.normal(size=(T + 1, B, S))
    X = X.detach().clone().requires_grad_(True)
    up = avg_host.upstream(G, lens, B, T + 1, torch.float64)
    (avg_host.states_from_slots(p, X, W) * up).sum().backward()
    dH = up.numpy() @ p["decoder.weight"].numpy()      # [B, T+1, D]; rows p >= len are zero
    want = np.zeros_like(dH)
    for b in range(B):
        for t in range(lens[b]):
            want[b, 0] += dH[b, t]
        for k in range(1, lens[b]):
            for t in range(k, min(lens[b] - 1, k + W - 1) + 1):
                want[b, k] += dH[b, t] / float(min(W, t))
    scale = np.abs(want).max()
    np.testing.assert_allclose(X.grad.numpy() / scale, want / scale, rtol=0, atol=1e-12)


def test_param_shapes_and_init():
    sh = avg_param_shapes(11, 13, 32, 20)
    assert list(sh) == ["embedding_dict.feat_user.weight", "embedding_dict.feat_item.weight", "ffn_user.weight", "ffn_user.bias", "fnn_gate.weight",
                        "fnn_gate.bias", "decoder.weight", "decoder.bias"]
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_avg_tracker_params(11, 13, seed=5)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    # every tensor is drawn as init_tracker_params draws it
    from cirs_hip.engine import init_tracker_params
    ref = init_tracker_params(11, 13, 5, seed=5)
    for k in p:
        assert torch.equal(p[k], ref[k]), k
    assert set(avgcase.avg_param_dict(11, 13, seed=1)) == set(sh)


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_avg_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerAvg, _RecurrentStateTracker

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    assert issubclass(StateTrackerAvg, _RecurrentStateTracker)      # what Collector(dropout_redraw=True) refuses
    uc, ac, fc = _columns()
    for bad in (0, -3):
        with pytest.raises(ValueError, match="window_size"):
            StateTrackerAvg(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, window_size=bad)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerAvg(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerAvg(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="max_len"):
        StateTrackerAvg(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, MAX_TURN=4096)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerAvg(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dataset="VirtualTB-v0")


def test_library_refuses_a_window_below_one_without_a_gpu():
    from cirs_hip import abi
    lib = abi.lib()
    cfg = abi.AvgCfg(n_users=3, n_items=4, dim_model=32, dim_state=20, window=0, max_len=5, n_env=2)
    assert lib.cirs_avg_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None) == -1
    assert b"window" in lib.cirs_last_error()
    assert lib.cirs_avg_tracker_init(C.byref(cfg), None, None, None, None, 2, None, 20, None) == -1 and b"window" in lib.cirs_last_error()
    assert lib.cirs_avg_tracker_backward(C.byref(cfg), None, None, None, None, None, None, None, None, None, 4, None, None, None, 0, None) == -1
    assert b"window" in lib.cirs_last_error()
    cfg.window = 3
    assert lib.cirs_avg_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None) == -1
    assert b"weights null" in lib.cirs_last_error()
    assert lib.cirs_avg_tracker_backward_workspace_bytes(C.byref(cfg), 0) == 0 and lib.cirs_avg_tracker_backward_workspace_bytes(C.byref(cfg), 7) > 0
    assert C.sizeof(abi.AvgCfg) == 7 * 4 and C.sizeof(abi.AvgWeights) == 8 * 8 and C.sizeof(abi.AvgState) == 2 * 8
