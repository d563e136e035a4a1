"""CPU: the host restatement of the LSTM tracker (cirs_hip/lstm_host.py) is torch.nn.LSTM + nn.Linear, the parameter names load into
nn.LSTM, the init is reproducible, and StateTrackerLSTM refuses what is not built before it touches a device."""
import types

import numpy as np
import pytest
import torch

import lstmcase
from cirs_hip import lstm_host
from cirs_hip.lstm_tracker import init_lstm_tracker_params, lstm_param_shapes


@pytest.mark.parametrize("L", [1, 2])
def test_written_out_equations_equal_torch_lstm(L):
    U, I, B, T, S = 30, 40, 5, 11, 20
    p = lstmcase.lstm_param_dict(U, I, seed=3, S=S, nlayers=L)
    users, acts, rews, lens, rng = lstmcase.teacher_inputs(U, I, B, T)
    G = rng.normal(size=(T + 1, B, S))
    # the equations, float64, autograd
    pe = lstm_host.cast_params(p, torch.float64, requires_grad=True)
    s_eq = lstm_host.states(pe, users, acts, rews, L)
    up = lstm_host.upstream(G, lens, B, T + 1, torch.float64)
    (s_eq * up).sum().backward()
    # torch.nn.LSTM + nn.Linear loaded from the same dict by name
    pm = lstm_host.cast_params(p, torch.float64, requires_grad=True)
    lstm, dec = lstm_host.build_modules(pm, L)
    s_mod = lstm_host.module_states(lstm, dec, lstm_host.input_slots(pm, users, acts, rews))
    (s_mod * up).sum().backward()
    np.testing.assert_allclose(s_eq.detach().numpy(), s_mod.detach().numpy(), rtol=0, atol=1e-12)
    mod_grads = {"lstm." + k: v.grad for k, v in lstm.named_parameters()}
    mod_grads.update({"decoder.weight": dec.weight.grad, "decoder.bias": dec.bias.grad})
    assert set(mod_grads) == {k for k in pe if k.startswith(("lstm.", "decoder."))}
    for k, v in pe.items():
        want = mod_grads[k] if k in mod_grads else pm[k].grad
        scale = float(want.abs().max()) + 1e-300
        np.testing.assert_allclose(v.grad.numpy() / scale, want.numpy() / scale, rtol=0, atol=1e-12, err_msg=k)
    for l in range(L):      # both bias vectors are parameters and receive the same gradient
        assert torch.equal(pe[f"lstm.bias_ih_l{l}"].grad, pe[f"lstm.bias_hh_l{l}"].grad) and float(pe[f"lstm.bias_ih_l{l}"].grad.abs().max()) > 0
    # and lstm_host.grads is that autograd
    got = lstm_host.grads(p, users, acts, rews, lens, G, L)
    for k, v in pe.items():
        np.testing.assert_array_equal(got[k], v.grad.numpy(), err_msg=k)


@pytest.mark.parametrize("L", [1, 2])
def test_param_shapes_load_into_nn_lstm(L):
    sh = lstm_param_shapes(11, 13, 32, 20, L)
    lstm = torch.nn.LSTM(32, 32, L)
    sd = {k[len("lstm."):]: torch.zeros(v) for k, v in sh.items() if k.startswith("lstm.")}
    lstm.load_state_dict(sd, strict=True)      # every name and shape, nothing missing, nothing extra
    assert {k: tuple(v.shape) for k, v in lstm.state_dict().items()} == {k[len("lstm."):]: v for k, v in sh.items() if k.startswith("lstm.")}
    assert sh["lstm.weight_ih_l0"] == (128, 32) and sh["lstm.weight_hh_l0"] == (128, 32) and sh["lstm.bias_ih_l0"] == sh["lstm.bias_hh_l0"] == (128,)
    assert list(sh)[:2] == ["embedding_dict.feat_user.weight", "embedding_dict.feat_item.weight"] and list(sh)[-2:] == ["decoder.weight", "decoder.bias"]


@pytest.mark.parametrize("L", [1, 2])
def test_init_is_reproducible_and_leaves_the_global_rng(L):
    sh = lstm_param_shapes(11, 13, 32, 20, L)
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_lstm_tracker_params(11, 13, seed=5, nlayers=L)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    bound = 1 / np.sqrt(32)      # torch.nn.LSTM's default init: U(-1/sqrt(D), 1/sqrt(D))
    for k, v in p.items():
        if k.startswith("lstm."):
            assert v.dtype == torch.float32 and float(v.abs().max()) <= bound and float(v.abs().max()) > 0.5 * bound, k
    again = init_lstm_tracker_params(11, 13, seed=5, nlayers=L)
    assert all(torch.equal(p[k], again[k]) for k in p)
    other = init_lstm_tracker_params(11, 13, seed=6, nlayers=L)
    assert not torch.equal(p["lstm.weight_hh_l0"], other["lstm.weight_hh_l0"])
    # what the trackers share is drawn as init_tracker_params draws it
    from cirs_hip.engine import init_tracker_params
    ref = init_tracker_params(11, 13, 5, seed=5)
    for k in p:
        if not k.startswith("lstm."):
            assert torch.equal(p[k], ref[k]), k


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_lstm_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerLSTM

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    uc, ac, fc = _columns()
    for bad in (0, 3):
        with pytest.raises(ValueError, match="nlayers"):
            StateTrackerLSTM(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, nlayers=bad)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerLSTM(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerLSTM(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="not built"):
        StateTrackerLSTM(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, nlayers=2, dropout=0.1)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerLSTM(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dataset="VirtualTB-v0")


def test_state_tracker_lstm_refuses_inter_layer_dropout_on_train():
    """.train() on a 2-layer tracker with dropout raises too; the object is made without a device (nn.Module state only)."""
    from core.state_tracker import StateTrackerLSTM
    st = StateTrackerLSTM.__new__(StateTrackerLSTM)
    torch.nn.Module.__init__(st)
    st.nlayers, st.dropout_p = 2, 0.1
    st.training = False
    with pytest.raises(ValueError, match="not built"):
        st.train()
    st.nlayers = 1
    assert st.train() is st and st.training
