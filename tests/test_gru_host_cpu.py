"""CPU: the host restatement of the GRU tracker (cirs_hip/gru_host.py) is torch.nn.GRU + nn.Linear, the parameter names load into
nn.GRU, and StateTrackerGRU refuses what is not built before it touches a device."""
import types

import numpy as np
import pytest
import torch

import grucase
from cirs_hip import gru_host
from cirs_hip.gru_tracker import gru_param_shapes, init_gru_tracker_params


@pytest.mark.parametrize("L", [1, 2])
def test_written_out_equations_equal_torch_gru(L):
    U, I, B, T, S = 30, 40, 5, 11, 20
    p = grucase.gru_param_dict(U, I, seed=3, S=S, nlayers=L)
    users, acts, rews, lens, rng = grucase.teacher_inputs(U, I, B, T)
    G = rng.normal(size=(T + 1, B, S))
    # the equations, float64, autograd
    pe = gru_host.cast_params(p, torch.float64, requires_grad=True)
    s_eq = gru_host.states(pe, users, acts, rews, L)
    up = gru_host.upstream(G, lens, B, T + 1, torch.float64)
    (s_eq * up).sum().backward()
    # torch.nn.GRU + nn.Linear loaded from the same dict by name
    pm = gru_host.cast_params(p, torch.float64, requires_grad=True)
    gru, dec = gru_host.build_modules(pm, L)
    s_mod = gru_host.module_states(gru, dec, gru_host.input_slots(pm, users, acts, rews))
    (s_mod * up).sum().backward()
    np.testing.assert_allclose(s_eq.detach().numpy(), s_mod.detach().numpy(), rtol=0, atol=1e-12)
    mod_grads = {"gru." + k: v.grad for k, v in gru.named_parameters()}
    mod_grads.update({"decoder.weight": dec.weight.grad, "decoder.bias": dec.bias.grad})
    for k, v in pe.items():
        want = mod_grads[k] if k in mod_grads else pm[k].grad
        scale = float(want.abs().max()) + 1e-300
        np.testing.assert_allclose(v.grad.numpy() / scale, want.numpy() / scale, rtol=0, atol=1e-12, err_msg=k)
    # and gru_host.grads is that autograd
    got = gru_host.grads(p, users, acts, rews, lens, G, L)
    for k, v in pe.items():
        np.testing.assert_array_equal(got[k], v.grad.numpy(), err_msg=k)


@pytest.mark.parametrize("L", [1, 2])
def test_param_shapes_load_into_nn_gru(L):
    sh = gru_param_shapes(11, 13, 32, 20, L)
    gru = torch.nn.GRU(32, 32, L)
    sd = {k[len("gru."):]: torch.zeros(v) for k, v in sh.items() if k.startswith("gru.")}
    gru.load_state_dict(sd, strict=True)      # every name and shape, nothing missing
    assert {k: tuple(v.shape) for k, v in gru.state_dict().items()} == {k[len("gru."):]: v for k, v in sh.items() if k.startswith("gru.")}
    assert list(sh)[:2] == ["embedding_dict.feat_user.weight", "embedding_dict.feat_item.weight"] and list(sh)[-2:] == ["decoder.weight", "decoder.bias"]
    p = init_gru_tracker_params(11, 13, seed=5, nlayers=L)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh
    bound = 1 / np.sqrt(32)
    for k, v in p.items():
        if k.startswith("gru."):
            assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.5 * bound, k
    again = init_gru_tracker_params(11, 13, seed=5, nlayers=L)
    assert all(torch.equal(p[k], again[k]) for k in p)
    # what both trackers share is drawn as init_tracker_params draws it
    from cirs_hip.engine import init_tracker_params
    ref = init_tracker_params(11, 13, 5, seed=5)
    for k in ("embedding_dict.feat_item.weight", "ffn_user.weight", "fnn_gate.bias", "decoder.weight"):
        assert torch.equal(p[k], ref[k]), k


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_gru_refuses_what_is_not_built():
    from core.state_tracker import StateTrackerGRU
    uc, ac, fc = _columns()
    with pytest.raises(ValueError, match="nlayers"):
        StateTrackerGRU(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, nlayers=3)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerGRU(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    with pytest.raises(ValueError, match="not built"):
        StateTrackerGRU(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, nlayers=2, dropout=0.1)
    with pytest.raises(NotImplementedError):
        StateTrackerGRU(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dataset="VirtualTB-v0")
