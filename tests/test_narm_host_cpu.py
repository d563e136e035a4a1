"""CPU: the host restatement of the GRU-with-attention tracker (cirs_hip/narm_host.py) equals an independent formulation -- torch.nn.GRU
loaded by state_dict name, then the attention in explicit Python loops over p and j -- in its states and, through autograd, in its gradients;
its autograd equals the closed-form backward the device kernels implement (the read-out, the attention once by query row and once by key row,
nothing per pair kept); the parameters carry their names in order and the init shares what it must with the GRU tracker's; StateTrackerNARM,
check_narm_shape and the library refuse what is not built before they touch a device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import narmcase
from cirs_hip import narm_host
from cirs_hip.narm_tracker import check_narm_shape, init_narm_tracker_params, narm_param_shapes
from narmcase import SLOT

D = 32
TWO_CASES = [0, 2]      # ragged lengths at T = 12; lengths 65 and 64


def _case(ci, dtype=torch.float64):
    U, I, B, T, L, S, hot = narmcase.CASES[ci]
    p = narm_host.cast_params(SLOT.params(ci), dtype)
    users, acts, rews, lens, rng = narmcase.teacher_inputs(U, I, B, T, hot)
    return p, (users, acts, rews), lens, rng


def _independent_states(p, X, gru, dec):
    """torch.nn.GRU(32, 32, 1) and the decoder loaded BY NAME (gru_host.build_modules), the attention one (p, j) pair at a time"""
    H, _ = gru(X.transpose(0, 1))
    H = H.transpose(0, 1)                                    # [B, T+1, D]
    A1, A2, v, Bw = p["attn.a1.weight"], p["attn.a2.weight"], p["attn.v.weight"][0], p["bilinear.weight"]
    B, L, _ = H.shape
    rows = []
    for b in range(B):
        out = []
        for q in range(L):
            c = torch.zeros(D, dtype=H.dtype)
            for j in range(q + 1):
                alpha = torch.dot(v, torch.sigmoid(A1 @ H[b, q] + A2 @ H[b, j]))
                c = c + alpha * H[b, j]
            out.append(dec(Bw @ torch.cat([H[b, q], c])))
        rows.append(torch.stack(out))
    return torch.stack(rows)


@pytest.mark.parametrize("ci", TWO_CASES, ids=[narmcase.IDS[c] for c in TWO_CASES])
def test_restatement_equals_nn_gru_and_explicit_attention_loops(ci):
    U, I, B, T, L, S, hot = narmcase.CASES[ci]
    p, inputs, lens, rng = _case(ci)
    live = np.arange(T + 1)[None, :] < lens[:, None]
    assert live[0].sum() == T and (B < 2 or live[1].sum() == T - 1)
    got = narm_host.states(p, *inputs, 1)
    from cirs_hip.gru_host import build_modules
    with torch.no_grad():
        want = _independent_states(p, narm_host.input_slots(p, *inputs), *build_modules(p, 1))
    assert got.shape == want.shape == (B, T + 1, S)
    np.testing.assert_allclose(got.numpy()[live], want.numpy()[live], rtol=0, atol=1e-12)
    # grads(): autograd through the independent formulation, every tensor
    G = rng.normal(size=(T + 1, B, S)).astype(np.float32)
    g = narm_host.grads(p, *inputs, lens, G, 1, torch.float64)
    pi = narm_host.cast_params(p, torch.float64, requires_grad=True)
    up = narm_host.upstream(G, lens, B, T + 1, torch.float64)
    gru, dec = build_modules(pi, 1)      # copies of the gru.* and decoder.* tensors: their gradients arrive in the modules
    (_independent_states(pi, narm_host.input_slots(pi, *inputs), gru, dec) * up).sum().backward()
    assert set(g) == set(pi) and len(g) == 16
    for k, v in pi.items():
        owner = {"gru": gru, "decoder": dec}.get(k.split(".")[0])
        want_g = (getattr(owner, k.split(".", 1)[1]) if owner is not None else v).grad.numpy()
        scale = np.abs(want_g).max()
        assert scale > 0, k
        assert np.abs(g[k] - want_g).max() / scale <= 1e-10, k


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _closed_form_backward(n, H, lens, dM):
    """Stages (E) second half, (F) and (G) of the device backward in numpy, env by env: nothing per (p, j) pair is kept between the two walks."""
    A1, A2, v, Bw = n["attn.a1.weight"], n["attn.a2.weight"], n["attn.v.weight"][0], n["bilinear.weight"]
    g = {k: np.zeros_like(n[k]) for k in narmcase.NEW}
    dH = np.zeros_like(H)
    for b in range(H.shape[0]):
        ln = lens[b]
        h = H[b, :ln]
        a, q = h @ A1.T, h @ A2.T
        c = np.zeros((ln, D))
        for p in range(ln):
            for j in range(p + 1):
                c[p] += (v @ _sig(a[p] + q[j])) * h[j]
        hc = np.concatenate([h, c], 1)
        dhc = dM[b, :ln] @ Bw
        g["bilinear.weight"] += dM[b, :ln].T @ hc
        dc = dhc[:, D:]
        dA, dQ, DV, dHk = (np.zeros((ln, D)) for _ in range(4))
        for p in range(ln):                                  # by query row
            for j in range(p + 1):
                e = _sig(a[p] + q[j])
                dalpha = dc[p] @ h[j]
                dA[p] += dalpha * v * e * (1 - e)
                DV[p] += dalpha * e
        for j in range(ln):                                  # by key row
            for p in range(j, ln):
                e = _sig(a[p] + q[j])
                dalpha = dc[p] @ h[j]
                dQ[j] += dalpha * v * e * (1 - e)
                dHk[j] += (v @ e) * dc[p]
        g["attn.v.weight"] += DV.sum(0)[None, :]
        g["attn.a1.weight"] += dA.T @ h
        g["attn.a2.weight"] += dQ.T @ h
        dH[b, :ln] = dhc[:, :D] + dHk + dA @ A1 + dQ @ A2
    return dH, g


@pytest.mark.parametrize("ci", [0, 5], ids=[narmcase.IDS[c] for c in (0, 5)])
def test_closed_form_attention_backward_equals_autograd(ci):
    U, I, B, T, L, S, hot = narmcase.CASES[ci]
    p, inputs, lens, rng = _case(ci)
    G = rng.normal(size=(T + 1, B, S))
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    H = narm_host.hidden_from_slots(p, narm_host.input_slots(p, *inputs)).detach().clone().requires_grad_(True)
    up = narm_host.upstream(G, lens, B, T + 1, torch.float64)
    (narm_host.states_from_hidden(p, H) * up).sum().backward()
    n = {k: v.detach().numpy() for k, v in p.items()}
    dM = up.numpy() @ n["decoder.weight"]                    # [B, T+1, D]; rows p >= len are zero
    dH, g = _closed_form_backward(n, H.detach().numpy(), lens, dM)

    def close(got, want, what):
        scale = np.abs(want).max()
        assert scale > 0, what
        err = np.abs(got - want).max() / scale
        assert err <= 1e-10, (what, err)
    close(dH, H.grad.numpy(), "dH")
    for k, v in g.items():
        close(v, p[k].grad.numpy(), k)


class _Attn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a1, self.a2, self.v = torch.nn.Linear(D, D, bias=False), torch.nn.Linear(D, D, bias=False), torch.nn.Linear(D, 1, bias=False)


class _Narm(torch.nn.Module):
    """the model's own tensors under their state_dict names"""
    def __init__(self, S):
        super().__init__()
        self.gru, self.attn = torch.nn.GRU(D, D, 1), _Attn()
        self.bilinear, self.decoder = torch.nn.Linear(2 * D, D, bias=False), torch.nn.Linear(D, S)


def test_param_names_order_shapes_and_init():
    sh = narm_param_shapes(11, 13, 32, 20)
    assert list(sh.items()) == [
        ("embedding_dict.feat_user.weight", (11, 32)), ("embedding_dict.feat_item.weight", (13, 32)), ("ffn_user.weight", (32, 32)),
        ("ffn_user.bias", (32,)), ("fnn_gate.weight", (32, 33)), ("fnn_gate.bias", (32,)),
        ("gru.weight_ih_l0", (96, 32)), ("gru.weight_hh_l0", (96, 32)), ("gru.bias_ih_l0", (96,)), ("gru.bias_hh_l0", (96,)),
        ("attn.a1.weight", (32, 32)), ("attn.a2.weight", (32, 32)), ("attn.v.weight", (1, 32)), ("bilinear.weight", (32, 64)),
        ("decoder.weight", (20, 32)), ("decoder.bias", (20,))]
    assert len(sh) == 16 and narm_param_shapes(11, 13, 32, 7)["decoder.weight"] == (7, 32)
    assert [k for k in sh if k.split(".")[0] in ("gru", "attn", "bilinear", "decoder")] == list(_Narm(20).state_dict())
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_narm_tracker_params(11, 13, seed=5)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    # the shared and the gru.* tensors are the GRU tracker's for the same seed
    from cirs_hip.gru_tracker import init_gru_tracker_params
    ref = init_gru_tracker_params(11, 13, seed=5, nlayers=1)
    n_shared = 0
    for k in p:
        if k in ref:
            assert torch.equal(p[k], ref[k]), k
            n_shared += 1
        else:
            assert k in narmcase.NEW and p[k].dtype == torch.float32 and torch.isfinite(p[k]).all(), k
            fan_in = p[k].shape[1]
            assert 0 < p[k].abs().max() <= 1 / np.sqrt(fan_in) + 1e-6, k      # torch's default nn.Linear init
    assert n_shared == 12
    again = init_narm_tracker_params(11, 13, seed=5)
    assert all(torch.equal(again[k], p[k]) for k in p)
    assert not torch.equal(init_narm_tracker_params(11, 13, seed=6)["bilinear.weight"], p["bilinear.weight"])
    # the init's own tensors load by name into the torch modules
    m = _Narm(20)
    m.load_state_dict({k: v for k, v in p.items() if k.split(".")[0] in ("gru", "attn", "bilinear", "decoder")}, strict=True)
    c = narmcase.narm_param_dict(11, 13, 1)
    assert list(c) == list(sh) and {k: tuple(v.shape) for k, v in c.items()} == sh
    for k, fan_in in (("attn.a1.weight", 32), ("attn.a2.weight", 32), ("attn.v.weight", 32), ("bilinear.weight", 64)):
        assert abs(float(c[k].std()) * np.sqrt(fan_in) - 1.0) < 0.35, k
    from grucase import gru_param_dict
    base = gru_param_dict(11, 13, 1, nlayers=1)
    assert all(torch.equal(c[k], base[k]) for k in base)


def test_check_shape_refusals_name_their_member():
    check_narm_shape(32, 20, 1, 101)
    check_narm_shape(32, 32)
    check_narm_shape(32, 1, 1)
    for kw, word in [(dict(dim_model=16), "dim_model"), (dict(dim_state=0), "dim_state"), (dict(dim_state=33), "dim_state"),
                     (dict(nlayers=2), "nlayers"), (dict(nlayers=0), "nlayers"), (dict(max_len=4097), "max_len"), (dict(max_len=0), "max_len")]:
        args = dict(dim_model=32, dim_state=20, nlayers=1, max_len=101)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            check_narm_shape(**args)


def test_slot_record():
    assert (SLOT.name, SLOT.display, SLOT.entry) == ("narm", "NARM", "cirs_narm_tracker")
    assert SLOT.n_grad_tensors(1) == 16 and SLOT.flags(1) == [] and SLOT.plugin_kw(1) == {}
    assert SLOT.split(SLOT.CASES[1]) == ((30, 40, 3, 100, 20, 0.0), 1)
    assert len(SLOT.CASES) == len(SLOT.IDS) == 7 and SLOT.host is narm_host and all(c[4] == 1 for c in SLOT.CASES)
    assert set(narmcase.NEW) | {"gru.weight_ih_l0", "gru.weight_hh_l0", "embedding_dict.feat_item.weight", "decoder.bias"} == set(SLOT.state_names)
    assert set(SLOT.state_names) <= set(narm_param_shapes(5, 6))
    assert type(SLOT).check_unambiguous is type(SLOT).__mro__[1].check_unambiguous      # smooth: the base's no-op
    assert SLOT.walk == ((3074, 3, 1, 5),)
    for ci, (U, I, B, T, L, S, hot) in enumerate(SLOT.CASES):      # the longest session of every case is certain
        lens = narmcase.teacher_inputs(U, I, B, T, hot)[3]
        assert lens[0] == T and (B < 2 or lens[1] == T - 1) and lens.min() >= 2 and lens.max() == T
    refusals = SLOT.engine_refusals({})
    assert len(refusals) == 1
    for exc, pattern, thunk in refusals:      # nlayers = 2: refused before any device use
        with pytest.raises(exc, match=pattern):
            thunk()


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_narm_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerNARM, _RecurrentStateTracker

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    assert issubclass(StateTrackerNARM, _RecurrentStateTracker)      # what Collector(dropout_redraw=True) refuses
    uc, ac, fc = _columns()
    kw = dict(dim_model=32, dim_state=20, dim_max_batch=4)
    for bad in (2, 0, 3):
        with pytest.raises(ValueError, match="nlayers"):
            StateTrackerNARM(uc, ac, fc, nlayers=bad, **kw)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerNARM(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerNARM(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="max_len"):
        StateTrackerNARM(uc, ac, fc, MAX_TURN=4096, **kw)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerNARM(uc, ac, fc, dataset="VirtualTB-v0", **kw)
    with pytest.raises(TypeError):
        StateTrackerNARM(uc, ac, fc, window_size=3, **kw)


def test_plugin_class_keywords_and_attributes_without_a_device(monkeypatch):
    from core.state_tracker import StateTrackerNARM
    monkeypatch.setattr(StateTrackerNARM, "_setup", lambda self, shapes, init, seed: None)      # no device: the flat buffer is not built
    uc, ac, fc = _columns()
    st = StateTrackerNARM(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dropout=0.1, nhead=4, d_hid=64)
    assert st.training      # dropout is accepted and unused: its two sites are not built
    assert st.dropout_p == 0.0 and st.nlayers == 1 and st.CELL == "NARM"
    assert st._model_kw() == {"nlayers": 1} and st._engine_kw() == {"nlayers": 1}
    st.eval(); st.train()
    assert "dropout" in StateTrackerNARM.__doc__ and "not" in StateTrackerNARM.__doc__


def test_library_refuses_the_same_cfgs_without_a_gpu():
    from cirs_hip import abi
    lib = abi.lib()

    def cfg_of(**kw):
        base = dict(n_users=3, n_items=4, dim_model=32, dim_state=20, nlayers=1, max_len=5, n_env=2)
        base.update(kw)
        return abi.NarmCfg(**base)

    def refused(cfg, word):
        calls = [lambda: lib.cirs_narm_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_narm_tracker_init(C.byref(cfg), None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_narm_tracker_backward(C.byref(cfg), None, None, None, None, None, None, None, None, None, 4, None, None, None, 0,
                                                        None)]
        for call in calls:
            assert call() != 0
            assert word in lib.cirs_last_error(), (word, lib.cirs_last_error())
            assert lib.cirs_last_error().startswith(b"narm tracker:"), lib.cirs_last_error()
        if word != b"weights null":
            assert lib.cirs_narm_tracker_backward_workspace_bytes(C.byref(cfg), 7) == 0
    refused(cfg_of(nlayers=2), b"nlayers")
    refused(cfg_of(nlayers=0), b"nlayers")
    refused(cfg_of(dim_model=16), b"dim_model")
    refused(cfg_of(dim_state=0), b"dim_state")
    refused(cfg_of(dim_state=33), b"dim_state")
    refused(cfg_of(max_len=4097), b"max_len")
    refused(cfg_of(max_len=0), b"max_len")
    refused(cfg_of(n_env=0), b"n_env")
    good = cfg_of()
    refused(good, b"weights null")
    assert lib.cirs_narm_tracker_backward_workspace_bytes(C.byref(good), 0) == 0
    sizes = [lib.cirs_narm_tracker_backward_workspace_bytes(C.byref(good), r) for r in (1, 7, 100, 5000)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes)), sizes      # positive, and growing with n_rows
    # O(rows), not O(rows x len): the same rows under a forty times longer history need the same workspace
    assert lib.cirs_narm_tracker_backward_workspace_bytes(C.byref(cfg_of(max_len=200)), 5000) == sizes[-1]
    # a null member is named before any pointer is read: the weights struct with one group of members missing
    one = C.c_float(0.0)
    ptr = C.addressof(one)
    w = abi.NarmWeights(**{k: ptr for k, _ in abi.NarmWeights._fields_})
    w.w_hh = None
    assert lib.cirs_narm_tracker_step(C.byref(good), C.byref(w), None, None, None, None, None, 2, None, 20, None) != 0
    assert b"encoder weight pointer null" in lib.cirs_last_error() and b"w_hh" in lib.cirs_last_error()
    w = abi.NarmWeights(**{k: ptr for k, _ in abi.NarmWeights._fields_})
    w.bw = None
    assert lib.cirs_narm_tracker_init(C.byref(good), C.byref(w), None, None, None, 2, None, 20, None) != 0
    assert b"attention / read-out weight pointer null" in lib.cirs_last_error()
    w = abi.NarmWeights(**{k: ptr for k, _ in abi.NarmWeights._fields_})      # every weight present, the state struct missing: refused, nothing launched
    assert lib.cirs_narm_tracker_init(C.byref(good), C.byref(w), None, C.addressof(one), None, 2, C.addressof(one), 20, None) != 0
    assert b"state pointer null" in lib.cirs_last_error()
    assert C.sizeof(abi.NarmCfg) == 7 * 4 and C.sizeof(abi.NarmWeights) == 16 * 8 and C.sizeof(abi.NarmState) == 5 * 8
