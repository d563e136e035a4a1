"""CPU: the host restatement of the linear-recurrence tracker (cirs_hip/lru_host.py, real arithmetic) equals an independent formulation --
torch.complex128 numbers, lambda from torch.polar, an explicit Python loop over the positions, nn.Linear / nn.LayerNorm / nn.GELU modules loaded
by state_dict name -- in its states and, through autograd, in its gradients; its autograd equals the closed-form backward the device kernels
implement for the recurrence (the adjoint scan, the per-env sums for d lambda and d gamma, the chain to the three log vectors, the input
projection); the parameters carry their names in order and the init shares what it must with the GRU tracker's; StateTrackerLRU,
check_lru_shape and the library refuse what is not built before they touch a device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import lrucase
from cirs_hip import lru_host
from cirs_hip.lru_tracker import check_lru_shape, init_lru_tracker_params, lru_param_shapes
from lrucase import SLOT

D = 32
TWO_CASES = [0, 2]      # ragged lengths at T = 12; lengths 65 and 64


def _case(ci, dtype=torch.float64):
    U, I, B, T, L, S, hot = lrucase.CASES[ci]
    p = lru_host.cast_params(SLOT.params(ci), dtype)
    users, acts, rews, lens, rng = lrucase.teacher_inputs(U, I, B, T, hot)
    return p, (users, acts, rews), lens, rng


class _Unit(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.nu_log, self.theta_log, self.gamma_log = (torch.nn.Parameter(torch.zeros(D)) for _ in range(3))
        self.in_proj, self.out_proj, self.ln = torch.nn.Linear(D, 2 * D), torch.nn.Linear(2 * D, D), torch.nn.LayerNorm(D, eps=1e-5)


class _Ffn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.dense_1, self.dense_2, self.ln = torch.nn.Linear(D, 128), torch.nn.Linear(128, D), torch.nn.LayerNorm(D, eps=1e-5)
        self.act = torch.nn.GELU()      # approximate="none": the erf form


class _Lru(torch.nn.Module):
    """the model's own tensors under their state_dict names"""
    def __init__(self, S):
        super().__init__()
        self.lru, self.ffn, self.decoder = _Unit(), _Ffn(), torch.nn.Linear(D, S)

    def forward(self, X):
        u = self.lru
        lam = torch.polar(torch.exp(-torch.exp(u.nu_log)), torch.exp(u.theta_log))          # complex [D]
        V = u.in_proj(X)
        vc = torch.view_as_complex(torch.stack([V[..., :D], V[..., D:]], -1).contiguous())   # [B, L, D] complex
        h = torch.zeros(X.shape[0], D, dtype=vc.dtype)
        out = []
        for t in range(X.shape[1]):
            h = lam * h + torch.exp(u.gamma_log) * vc[:, t]
            z = u.ln(u.out_proj(torch.cat([h.real, h.imag], -1)) + X[:, t])
            m = self.ffn.ln(z + self.ffn.dense_2(self.ffn.act(self.ffn.dense_1(z))))
            out.append(self.decoder(m))
        return torch.stack(out, 1)


OWN = ("lru", "ffn", "decoder")


def _module(p, S):
    m = _Lru(S).double()
    m.load_state_dict({k: v.detach() for k, v in p.items() if k.split(".")[0] in OWN}, strict=True)
    return m


@pytest.mark.parametrize("ci", TWO_CASES, ids=[lrucase.IDS[c] for c in TWO_CASES])
def test_restatement_equals_complex_numbers_and_torch_modules(ci):
    U, I, B, T, L, S, hot = lrucase.CASES[ci]
    p, inputs, lens, rng = _case(ci)
    live = np.arange(T + 1)[None, :] < lens[:, None]
    assert live[0].sum() == T and (B < 2 or live[1].sum() == T - 1)
    got = lru_host.states(p, *inputs, 1)
    with torch.no_grad():
        want = _module(p, S)(lru_host.input_slots(p, *inputs))
    assert got.shape == want.shape == (B, T + 1, S)
    np.testing.assert_allclose(got.numpy()[live], want.numpy()[live], rtol=0, atol=1e-12)
    # grads(): autograd through the independent formulation, every tensor
    G = rng.normal(size=(T + 1, B, S)).astype(np.float32)
    g = lru_host.grads(p, *inputs, lens, G, 1, torch.float64)
    pi = lru_host.cast_params(p, torch.float64, requires_grad=True)
    up = lru_host.upstream(G, lens, B, T + 1, torch.float64)
    mod = _module(pi, S)      # copies of the lru.*, ffn.* and decoder.* tensors: their gradients arrive in the module
    (mod(lru_host.input_slots(pi, *inputs)) * up).sum().backward()
    own = dict(mod.named_parameters())
    assert set(g) == set(pi) and len(g) == 23
    for k, v in pi.items():
        want_g = (own[k] if k.split(".")[0] in OWN else v).grad.numpy()
        scale = np.abs(want_g).max()
        assert scale > 0, k
        assert np.abs(g[k] - want_g).max() / scale <= 1e-10, k


def _closed_form_recurrence_backward(n, X, lens, dH_re, dH_im):
    """Stages (G) and (H) of the device backward in numpy, env by env: the adjoint scan in descending p with its per-env sums, the fixed-order
    sum over the envs, the chain to the log vectors, dV = gamma * a, the input projection's gradients and its share of dX."""
    nu, th, gl = n["lru.nu_log"], n["lru.theta_log"], n["lru.gamma_log"]
    W, bias = n["lru.in_proj.weight"], n["lru.in_proj.bias"]
    mod, phi, ga = np.exp(-np.exp(nu)), np.exp(th), np.exp(gl)
    lr, li = mod * np.cos(phi), mod * np.sin(phi)
    B, L, _ = X.shape
    V = X @ W.T + bias
    dV = np.zeros_like(V)
    d_lr, d_li, d_ga = np.zeros(D), np.zeros(D), np.zeros(D)
    for b in range(B):
        ln = lens[b]
        h_re, h_im = np.zeros((ln, D)), np.zeros((ln, D))      # the forward scan again
        pr, pm = np.zeros(D), np.zeros(D)
        for p in range(ln):
            pr, pm = lr * pr - li * pm + ga * V[b, p, :D], lr * pm + li * pr + ga * V[b, p, D:]
            h_re[p], h_im[p] = pr, pm
        a_re, a_im = np.zeros(D), np.zeros(D)
        s_lr, s_li, s_ga = np.zeros(D), np.zeros(D), np.zeros(D)
        for p in range(ln - 1, -1, -1):
            a_re, a_im = dH_re[b, p] + lr * a_re + li * a_im, dH_im[b, p] + lr * a_im - li * a_re
            dV[b, p, :D], dV[b, p, D:] = ga * a_re, ga * a_im
            if p >= 1:
                s_lr += a_re * h_re[p - 1] + a_im * h_im[p - 1]
                s_li += -a_re * h_im[p - 1] + a_im * h_re[p - 1]
            s_ga += a_re * V[b, p, :D] + a_im * V[b, p, D:]
        d_lr += s_lr; d_li += s_li; d_ga += s_ga
    g = {"lru.nu_log": -np.exp(nu) * (lr * d_lr + li * d_li), "lru.theta_log": phi * (-li * d_lr + lr * d_li), "lru.gamma_log": ga * d_ga,
         "lru.in_proj.weight": dV.reshape(-1, 2 * D).T @ X.reshape(-1, D), "lru.in_proj.bias": dV.reshape(-1, 2 * D).sum(0)}
    return g, dV @ W


@pytest.mark.parametrize("ci", [0, 5, 7], ids=[lrucase.IDS[c] for c in (0, 5, 7)])
def test_closed_form_recurrence_backward_equals_autograd(ci):
    U, I, B, T, L, S, hot = lrucase.CASES[ci]
    p, inputs, lens, rng = _case(ci)
    G = rng.normal(size=(T + 1, B, S))
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    X = lru_host.input_slots(p, *inputs).detach().clone().requires_grad_(True)
    up = lru_host.upstream(G, lens, B, T + 1, torch.float64)
    # the gradient at the hidden states, from everything above the recurrence
    h_re, h_im = (h.detach().clone().requires_grad_(True) for h in lru_host.hidden_from_slots(p, X))
    (lru_host.states_from_hidden(p, X.detach(), h_re, h_im) * up).sum().backward()
    dH_re, dH_im = h_re.grad.clone(), h_im.grad.clone()
    for v in p.values():
        v.grad = None
    # autograd through the recurrence alone
    r_re, r_im = lru_host.hidden_from_slots(p, X)
    ((r_re * dH_re).sum() + (r_im * dH_im).sum()).backward()
    n = {k: v.detach().numpy() for k, v in p.items()}
    g, dX = _closed_form_recurrence_backward(n, X.detach().numpy(), lens, dH_re.numpy(), dH_im.numpy())

    def close(got, want, what):
        scale = np.abs(want).max()
        assert scale > 0, what
        err = np.abs(got - want).max() / scale
        assert err <= 1e-10, (what, err)
    close(dX, X.grad.numpy(), "dX")
    for k, v in g.items():
        close(v, p[k].grad.numpy(), k)


def test_param_names_order_shapes_and_init():
    sh = lru_param_shapes(11, 13, 32, 20)
    assert list(sh.items()) == [
        ("embedding_dict.feat_user.weight", (11, 32)), ("embedding_dict.feat_item.weight", (13, 32)), ("ffn_user.weight", (32, 32)),
        ("ffn_user.bias", (32,)), ("fnn_gate.weight", (32, 33)), ("fnn_gate.bias", (32,)),
        ("lru.nu_log", (32,)), ("lru.theta_log", (32,)), ("lru.gamma_log", (32,)),
        ("lru.in_proj.weight", (64, 32)), ("lru.in_proj.bias", (64,)), ("lru.out_proj.weight", (32, 64)), ("lru.out_proj.bias", (32,)),
        ("lru.ln.weight", (32,)), ("lru.ln.bias", (32,)),
        ("ffn.dense_1.weight", (128, 32)), ("ffn.dense_1.bias", (128,)), ("ffn.dense_2.weight", (32, 128)), ("ffn.dense_2.bias", (32,)),
        ("ffn.ln.weight", (32,)), ("ffn.ln.bias", (32,)),
        ("decoder.weight", (20, 32)), ("decoder.bias", (20,))]
    assert len(sh) == 23 and lru_param_shapes(11, 13, 32, 7)["decoder.weight"] == (7, 32)
    assert [k for k in sh if k.split(".")[0] in OWN] == list(_Lru(20).state_dict())
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_lru_tracker_params(11, 13, seed=5)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    # the shared tensors and the decoder are the GRU tracker's for the same seed, bit for bit
    from cirs_hip.gru_tracker import init_gru_tracker_params
    ref = init_gru_tracker_params(11, 13, seed=5, nlayers=1)
    n_shared = 0
    for k in p:
        if k in ref:
            assert torch.equal(p[k], ref[k]), k
            n_shared += 1
        else:
            assert k in lrucase.NEW and p[k].dtype == torch.float32 and torch.isfinite(p[k]).all(), k
    assert n_shared == 8
    again = init_lru_tracker_params(11, 13, seed=5)
    assert all(torch.equal(again[k], p[k]) for k in p)
    assert not torch.equal(init_lru_tracker_params(11, 13, seed=6)["lru.nu_log"], p["lru.nu_log"])
    # the ring: |lambda| < 1, the phase in (0, 2 pi], gamma^2 = 1 - |lambda|^2, everything finite, for ten seeds
    for seed in range(10):
        q = init_lru_tracker_params(11, 13, seed=seed)
        assert all(torch.isfinite(v).all() for v in q.values()), seed
        lr, li, ga = lru_host.eigenvalues(lru_host.cast_params(q, torch.float64))
        mod = torch.sqrt(lr * lr + li * li)
        assert float(mod.max()) < 1.0 and float(mod.min()) > 0.0, seed
        phi = torch.exp(q["lru.theta_log"].double())
        assert float(phi.min()) > 0.0 and float(phi.max()) <= 2 * np.pi + 1e-6, seed
        np.testing.assert_allclose((ga * ga).numpy(), (1 - mod * mod).numpy(), rtol=1e-5, atol=1e-7)
        for k, fan_in in (("lru.in_proj.weight", 32), ("lru.out_proj.weight", 64), ("ffn.dense_1.weight", 32), ("ffn.dense_2.weight", 128)):
            assert 0 < q[k].abs().max() <= 1 / np.sqrt(fan_in) + 1e-6, k      # torch's default nn.Linear init
        assert torch.equal(q["lru.ln.weight"], torch.ones(32)) and torch.equal(q["ffn.ln.bias"], torch.zeros(32))
    # the init's own tensors load by name into the torch modules
    _Lru(20).load_state_dict({k: v for k, v in p.items() if k.split(".")[0] in OWN}, strict=True)
    c = lrucase.lru_param_dict(11, 13, 1)
    assert list(c) == list(sh) and {k: tuple(v.shape) for k, v in c.items()} == sh
    lr, li, ga = lru_host.eigenvalues(lru_host.cast_params(c, torch.float64))
    mod, phi = torch.sqrt(lr * lr + li * li), torch.exp(c["lru.theta_log"].double())
    assert 0.30 - 1e-6 <= float(mod.min()) and float(mod.max()) <= 0.98 + 1e-6
    assert 0.05 - 1e-6 <= float(phi.min()) and float(phi.max()) <= 2 * np.pi - 0.05 + 1e-5 and float(phi.max()) > np.pi
    for k, fan_in in (("lru.in_proj.weight", 32), ("lru.out_proj.weight", 64), ("ffn.dense_1.weight", 32), ("ffn.dense_2.weight", 128)):
        assert abs(float(c[k].std()) * np.sqrt(fan_in) - 1.0) < 0.35, k
    from grucase import gru_param_dict
    base = gru_param_dict(11, 13, 1, nlayers=1)
    assert all(torch.equal(c[k], base[k]) for k in base if not k.startswith("gru."))


def test_check_shape_refusals_name_their_member():
    check_lru_shape(32, 20, 1, 128, 101)
    check_lru_shape(32, 32)
    check_lru_shape(32, 1, 1)
    for kw, word in [(dict(dim_model=16), "dim_model"), (dict(dim_state=0), "dim_state"), (dict(dim_state=33), "dim_state"),
                     (dict(nlayers=2), "nlayers"), (dict(nlayers=0), "nlayers"), (dict(d_hid=64), "d_hid"), (dict(max_len=4097), "max_len"),
                     (dict(max_len=0), "max_len")]:
        args = dict(dim_model=32, dim_state=20, nlayers=1, d_hid=128, max_len=101)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            check_lru_shape(**args)


def test_slot_record():
    assert (SLOT.name, SLOT.display, SLOT.entry) == ("lru", "LRU", "cirs_lru_tracker")
    assert SLOT.n_grad_tensors(1) == 23 and SLOT.flags(1) == [] and SLOT.plugin_kw(1) == {}
    assert SLOT.split(SLOT.CASES[1]) == ((30, 40, 3, 100, 20, 0.0), 1)
    assert len(SLOT.CASES) == len(SLOT.IDS) == 8 and SLOT.host is lru_host and all(c[4] == 1 for c in SLOT.CASES)
    assert SLOT.CASES[7][3] == lrucase.SCAN + 1 == 9
    assert set(lrucase.NEW) | {"embedding_dict.feat_item.weight", "decoder.bias"} == set(SLOT.state_names)
    assert set(SLOT.state_names) <= set(lru_param_shapes(5, 6))
    assert type(SLOT).check_unambiguous is type(SLOT).__mro__[1].check_unambiguous      # smooth: the base's no-op
    assert SLOT.walk == ((2050, 3, 1, 5),) and SLOT.carried == ()
    for ci, (U, I, B, T, L, S, hot) in enumerate(SLOT.CASES):      # the longest session of every case is certain
        lens = lrucase.teacher_inputs(U, I, B, T, hot)[3]
        assert lens[0] == T and (B < 2 or lens[1] == T - 1) and lens.min() >= 2 and lens.max() == T
    refusals = SLOT.engine_refusals({})
    assert len(refusals) == 1
    for exc, pattern, thunk in refusals:      # nlayers = 2: refused before any device use
        with pytest.raises(exc, match=pattern):
            thunk()


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_lru_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerLRU, _RecurrentStateTracker

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    assert issubclass(StateTrackerLRU, _RecurrentStateTracker)      # what Collector(dropout_redraw=True) refuses
    uc, ac, fc = _columns()
    kw = dict(dim_model=32, dim_state=20, dim_max_batch=4)
    for bad in (2, 0, 3):
        with pytest.raises(ValueError, match="nlayers"):
            StateTrackerLRU(uc, ac, fc, nlayers=bad, **kw)
    with pytest.raises(ValueError, match="d_hid"):
        StateTrackerLRU(uc, ac, fc, d_hid=64, **kw)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerLRU(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerLRU(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="max_len"):
        StateTrackerLRU(uc, ac, fc, MAX_TURN=4096, **kw)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerLRU(uc, ac, fc, dataset="VirtualTB-v0", **kw)
    with pytest.raises(TypeError):
        StateTrackerLRU(uc, ac, fc, window_size=3, **kw)


def test_plugin_class_keywords_and_attributes_without_a_device(monkeypatch):
    from core.state_tracker import StateTrackerLRU
    monkeypatch.setattr(StateTrackerLRU, "_setup", lambda self, shapes, init, seed: None)      # no device: the flat buffer is not built
    uc, ac, fc = _columns()
    st = StateTrackerLRU(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dropout=0.1, nhead=4, d_hid=128)
    assert st.training      # dropout is accepted and unused: its sites are not built
    assert st.dropout_p == 0.0 and st.nlayers == 1 and st.d_hid == 128 and st.CELL == "LRU"
    assert st._model_kw() == {"nlayers": 1} and st._engine_kw() == {"nlayers": 1}
    st.eval(); st.train()
    assert "dropout" in StateTrackerLRU.__doc__ and "not" in StateTrackerLRU.__doc__


def test_library_refuses_the_same_cfgs_without_a_gpu():
    from cirs_hip import abi
    lib = abi.lib()

    def cfg_of(**kw):
        base = dict(n_users=3, n_items=4, dim_model=32, dim_state=20, nlayers=1, max_len=5, n_env=2)
        base.update(kw)
        return abi.LruCfg(**base)

    def refused(cfg, word):
        calls = [lambda: lib.cirs_lru_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_lru_tracker_init(C.byref(cfg), None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_lru_tracker_backward(C.byref(cfg), None, None, None, None, None, None, None, None, None, 4, None, None, None, 0,
                                                       None)]
        for call in calls:
            assert call() != 0
            assert word in lib.cirs_last_error(), (word, lib.cirs_last_error())
            assert lib.cirs_last_error().startswith(b"lru tracker:"), lib.cirs_last_error()
        if word != b"weights null":
            assert lib.cirs_lru_tracker_backward_workspace_bytes(C.byref(cfg), 7) == 0
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
    assert lib.cirs_lru_tracker_backward_workspace_bytes(C.byref(good), 0) == 0
    sizes = [lib.cirs_lru_tracker_backward_workspace_bytes(C.byref(good), r) for r in (1, 7, 100, 5000)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes)), sizes      # positive, and growing with n_rows
    # O(rows) + O(n_env), not O(rows x len): the same rows need the same workspace at max_len 13 and at 4096
    at = [lib.cirs_lru_tracker_backward_workspace_bytes(C.byref(cfg_of(max_len=m)), 5000) for m in (13, 4096)]
    assert at[0] == at[1] > 0
    # ... and the per-env part (the adjoint scan's partials, the slot stage's user rows) grows with n_env alone
    more = [lib.cirs_lru_tracker_backward_workspace_bytes(C.byref(cfg_of(max_len=m, n_env=2 + 64)), 5000) for m in (13, 4096)]
    assert more[0] == more[1] and 64 * 3 * 32 * 4 <= more[0] - at[0] <= 64 * 1024
    # a null member is named before any pointer is read: the weights struct with one member missing
    one = C.c_float(0.0)
    ptr = C.addressof(one)
    w = abi.LruWeights(**{k: ptr for k, _ in abi.LruWeights._fields_})
    w.theta_log = None
    assert lib.cirs_lru_tracker_step(C.byref(good), C.byref(w), None, None, None, None, None, 2, None, 20, None) != 0
    assert b"recurrence / feed-forward weight pointer null" in lib.cirs_last_error()
    w = abi.LruWeights(**{k: ptr for k, _ in abi.LruWeights._fields_})
    w.dec_b = None
    assert lib.cirs_lru_tracker_init(C.byref(good), C.byref(w), None, None, None, 2, None, 20, None) != 0
    assert b"lru tracker: weight pointer null" in lib.cirs_last_error()
    w = abi.LruWeights(**{k: ptr for k, _ in abi.LruWeights._fields_})      # every weight present, the state struct missing: refused, nothing launched
    assert lib.cirs_lru_tracker_init(C.byref(good), C.byref(w), None, C.addressof(one), None, 2, C.addressof(one), 20, None) != 0
    assert b"state pointer null" in lib.cirs_last_error()
    # the structs as include/cirs_hip.h lays them out: seven int32, 23 pointers, four pointers
    assert C.sizeof(abi.LruCfg) == 7 * 4 and C.sizeof(abi.LruWeights) == 23 * 8 and C.sizeof(abi.LruState) == 4 * 8
    assert [k for k, _ in abi.LruState._fields_] == ["x_hist", "h_re", "h_im", "len"] and abi.LRU_MAX_LAYERS == 1
