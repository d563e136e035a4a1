"""CPU: the host restatement of the filter-MLP tracker (cirs_hip/fmlp_host.py) equals a W = 2 answer computed by hand in numpy and a stack of
torch modules (nn.LayerNorm, nn.Linear, F.gelu, torch.fft) loaded by state_dict name; its frequency-domain filter equals the circular
convolution with h = irfft(w, n=W) the device computes; its autograd equals the closed-form filter backward the device kernels implement, the
exact zeros included; a state depends on the last W slots and on x_0 only; the parameters carry their names in order and the init is
reproducible; StateTrackerFMLP, check_fmlp_shape and the library refuse what is not built before they touch a device."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fmlpcase
from cirs_hip import fmlp_host
from cirs_hip.fmlp_tracker import check_fmlp_shape, fmlp_param_shapes, init_fmlp_tracker_params
from fmlpcase import SLOT

D = 32
WINDOWS = [1, 2, 3, 5, 10, 16]


def _case(ci, dtype=torch.float64):
    U, I, B, T, (W, L), S, hot = fmlpcase.CASES[ci]
    p = fmlp_host.cast_params(SLOT.params(ci), dtype)
    users, acts, rews, lens, rng = fmlpcase.teacher_inputs(U, I, B, T, hot)
    return p, (users, acts, rews), lens, rng


# ---- by hand, W = 2 ----------------------------------------------------------------------------------------------------------------------
def _ln_np(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * g + b


def _gelu_np(u):
    return 0.5 * u * (1.0 + np.vectorize(math.erf)(u / math.sqrt(2.0)))


def _layer_w2_np(p, l, y0, y1):
    """One layer on the two-row tile (y0, y1), the filter written out: with the ortho transforms of length 2, bins (y0 + y1) / sqrt 2 and
    (y0 - y1) / sqrt 2, F0 = ((a0 + a1) y0 + (a0 - a1) y1) / 2 and F1 = ((a0 - a1) y0 + (a0 + a1) y1) / 2; a_k = the REAL part of bin k (both bins
    of W = 2 are real bins: the imaginary parts are not read)."""
    g = lambda k: p[f"layers.{l}.{k}"].numpy()  # noqa: E731
    cw = g("filter.complex_weight")
    a0, a1 = cw[0, :, 0], cw[1, :, 0]
    f0 = ((a0 + a1) * y0 + (a0 - a1) * y1) / 2
    f1 = ((a0 - a1) * y0 + (a0 + a1) * y1) / 2
    rows = []
    for y, f in ((y0, f0), (y1, f1)):
        a = _ln_np(y + f, g("filter.ln.weight"), g("filter.ln.bias"))
        m = _gelu_np(a @ g("ffn.dense_1.weight").T + g("ffn.dense_1.bias")) @ g("ffn.dense_2.weight").T + g("ffn.dense_2.bias")
        rows.append(_ln_np(a + m, g("ffn.ln.weight"), g("ffn.ln.bias")))
    return rows


def test_restatement_equals_the_w2_answer_by_hand():
    ci = 5
    U, I, B, T, (W, L), S, hot = fmlpcase.CASES[ci]
    assert (W, L) == (2, 2)
    p, inputs, lens, rng = _case(ci)
    got = fmlp_host.states(p, *inputs, W).numpy()
    X = fmlp_host.input_slots(p, *inputs).numpy()
    dec_w, dec_b = p["decoder.weight"].numpy(), p["decoder.bias"].numpy()
    for b in range(B):
        for t in range(int(lens[b])):
            h = X[b, 0]
            if t >= 1:
                y0, y1 = (X[b, t - 1] if t >= 2 else np.zeros(D)), X[b, t]      # position 1: the padded row in front
                for l in range(L):
                    y0, y1 = _layer_w2_np(p, l, y0, y1)      # the padded row is an ordinary row from layer 0's output on
                h = h + y1
            np.testing.assert_allclose(got[b, t], h @ dec_w.T + dec_b, rtol=0, atol=1e-12)


# ---- a stack of torch modules, loaded by name ----------------------------------------------------------------------------------------------
class _Filter(torch.nn.Module):
    def __init__(self, W):
        super().__init__()
        self.complex_weight = torch.nn.Parameter(torch.zeros(W // 2 + 1, D, 2))
        self.ln = torch.nn.LayerNorm(D)

    def forward(self, y):
        W = y.shape[-2]
        f = torch.fft.irfft(torch.fft.rfft(y, dim=-2, norm="ortho") * torch.view_as_complex(self.complex_weight), n=W, dim=-2, norm="ortho")
        return self.ln(y + f)


class _Ffn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.dense_1, self.dense_2, self.ln = torch.nn.Linear(D, 128), torch.nn.Linear(128, D), torch.nn.LayerNorm(D)

    def forward(self, a):
        return self.ln(a + self.dense_2(F.gelu(self.dense_1(a))))


class _Layer(torch.nn.Module):
    def __init__(self, W):
        super().__init__()
        self.filter, self.ffn = _Filter(W), _Ffn()

    def forward(self, y):
        return self.ffn(self.filter(y))


class _Fmlp(torch.nn.Module):
    def __init__(self, W, L, S):
        super().__init__()
        self.layers = torch.nn.ModuleList([_Layer(W) for _ in range(L)])
        self.decoder = torch.nn.Linear(D, S)


def _own(k):
    return k.split(".")[0] in ("layers", "decoder")


@pytest.mark.parametrize("ci", [0, 3, 6], ids=[fmlpcase.IDS[c] for c in (0, 3, 6)])
def test_restatement_equals_torch_modules_loaded_by_name(ci):
    U, I, B, T, (W, L), S, hot = fmlpcase.CASES[ci]
    p, inputs, lens, rng = _case(ci)
    live = np.arange(T + 1)[None, :] < lens[:, None]
    got = fmlp_host.states(p, *inputs, W)
    m = _Fmlp(W, L, S).double()
    m.load_state_dict({k: v for k, v in p.items() if _own(k)}, strict=True)
    X = fmlp_host.input_slots(p, *inputs)
    with torch.no_grad():
        rows = [m.decoder(X[:, 0])]
        for t in range(1, T + 1):
            tile = torch.zeros(B, W, D, dtype=torch.float64)
            for i in range(W):
                k = t - W + 1 + i
                if k >= 1:
                    tile[:, i] = X[:, k]
            for layer in m.layers:
                tile = layer(tile)
            rows.append(m.decoder(X[:, 0] + tile[:, W - 1]))
        want = torch.stack(rows, 1)
    assert got.shape == want.shape == (B, T + 1, S)
    np.testing.assert_allclose(got.numpy()[live], want.numpy()[live], rtol=0, atol=1e-12)


# ---- the two formulations of the filter --------------------------------------------------------------------------------------------------------
def _circulant(h, Y):
    """F[b, i, d] = sum_m h[(i - m) mod W, d] Y[b, m, d]: what the device computes"""
    W = Y.shape[-2]
    out = np.zeros_like(Y)
    for i in range(W):
        for m in range(W):
            out[:, i] += h[(i - m) % W] * Y[:, m]
    return out


@pytest.mark.parametrize("W", WINDOWS)
def test_rfft_form_equals_the_circulant_form(W):
    g = torch.Generator().manual_seed(100 + W)
    Y = torch.randn(4, W, D, generator=g, dtype=torch.float64)
    cw = torch.randn(W // 2 + 1, D, 2, generator=g, dtype=torch.float64)
    w = torch.view_as_complex(cw)
    freq = torch.fft.irfft(torch.fft.rfft(Y, dim=-2, norm="ortho") * w, n=W, dim=-2, norm="ortho").numpy()
    h = torch.fft.irfft(w, n=W, dim=0).numpy()
    assert h.shape == (W, D)
    np.testing.assert_allclose(freq, _circulant(h, Y.numpy()), rtol=0, atol=1e-12)
    # h from the integer-reduced phases, as the device forms it: (1 / W) sum_k c_k (re cos - im sin), the imaginary parts of the real bins unread
    hk = np.zeros((W, D))
    for n in range(W):
        for k in range(W // 2 + 1):
            real_bin = k == 0 or 2 * k == W
            ang = 2 * math.pi * ((k * n) % W) / W
            re, im = cw[k, :, 0].numpy(), (0.0 if real_bin else cw[k, :, 1].numpy())
            hk[n] += (1.0 if real_bin else 2.0) * (re * math.cos(ang) - im * math.sin(ang))
    np.testing.assert_allclose(hk / W, h, rtol=0, atol=1e-12)


@pytest.mark.parametrize("W", WINDOWS)
def test_closed_form_filter_backward_equals_autograd(W):
    g = torch.Generator().manual_seed(200 + W)
    Y = torch.randn(W, D, generator=g, dtype=torch.float64, requires_grad=True)
    cw = torch.randn(W // 2 + 1, D, 2, generator=g, dtype=torch.float64, requires_grad=True)
    dPre = torch.randn(W, D, generator=g, dtype=torch.float64)
    Fq = torch.fft.irfft(torch.fft.rfft(Y, dim=0, norm="ortho") * torch.view_as_complex(cw), n=W, dim=0, norm="ortho")
    ((Y + Fq) * dPre).sum().backward()
    y, dp = Y.detach().numpy(), dPre.numpy()
    h = torch.fft.irfft(torch.view_as_complex(cw.detach()), n=W, dim=0).numpy()
    dh = np.zeros((W, D))
    dY = dp.copy()
    for n in range(W):
        for i in range(W):
            dh[n] += dp[i] * y[(i - n) % W]
            dY[n] += h[(i - n) % W] * dp[i]
    dcw = np.zeros((W // 2 + 1, D, 2))
    for k in range(W // 2 + 1):
        real_bin = k == 0 or 2 * k == W
        ck = 1.0 if real_bin else 2.0
        for n in range(W):
            ang = 2 * math.pi * ((k * n) % W) / W
            dcw[k, :, 0] += ck / W * dh[n] * math.cos(ang)
            if not real_bin:
                dcw[k, :, 1] -= ck / W * dh[n] * math.sin(ang)
    got = cw.grad.numpy()
    np.testing.assert_allclose(got, dcw, rtol=0, atol=1e-12 * np.abs(dcw).max())
    np.testing.assert_allclose(Y.grad.numpy(), dY, rtol=0, atol=1e-12 * np.abs(dY).max())
    # the entries without effect: an exact zero, from autograd as from the closed form
    assert (got[0, :, 1] == 0).all() and (dcw[0, :, 1] == 0).all()
    if W % 2 == 0:
        assert (got[W // 2, :, 1] == 0).all() and (dcw[W // 2, :, 1] == 0).all()
    assert np.abs(got[..., 0]).min() > 0 and (W < 3 or np.abs(got[1, :, 1]).min() > 0)


def test_gelu_derivative_is_cdf_plus_u_pdf():
    u = torch.linspace(-6, 6, 481, dtype=torch.float64, requires_grad=True)
    F.gelu(u).sum().backward()
    x = u.detach().numpy()
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))
    pdf = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    np.testing.assert_allclose(u.grad.numpy(), cdf + x * pdf, rtol=0, atol=1e-12)


# ---- what a state depends on ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1], ids=[fmlpcase.IDS[c] for c in (0, 1)])
def test_state_depends_on_the_last_w_slots_and_x0_only(ci):
    U, I, B, T, (W, L), S, hot = fmlpcase.CASES[ci]
    p, inputs, lens, rng = _case(ci)
    X = fmlp_host.input_slots(p, *inputs)
    full = fmlp_host.states_from_slots(p, X, W)
    t = T      # the restatement computes every position of every env, whatever its length
    assert X.shape[1] == T + 1 and t > W
    last_w = torch.cat([X[:1, :1], X[:1, t - W + 1:t + 1]], 1)              # x_0, then the last W slots: the state of position W there
    got = fmlp_host.states_from_slots(p, last_w, W)[0, W]
    np.testing.assert_allclose(got.numpy(), full[0, t].numpy(), rtol=0, atol=1e-12)
    fewer = torch.cat([X[:1, :1], X[:1, t - W + 2:t + 1]], 1)               # one slot fewer: a padded row where x_{t-W+1} was
    other = fmlp_host.states_from_slots(p, fewer, W)[0, W - 1]
    assert float((other - full[0, t]).abs().max()) > 1e-3
    older = X.clone()
    older[0, t - W] += 1.0                                                   # a slot older than the window does not reach position t
    np.testing.assert_array_equal(fmlp_host.states_from_slots(p, older, W)[0, t].numpy(), full[0, t].numpy())


# ---- names, order, init ---------------------------------------------------------------------------------------------------------------------
def test_param_names_order_shapes_and_init():
    sh = fmlp_param_shapes(11, 13, 32, 20, 10, 2)
    head = [("embedding_dict.feat_user.weight", (11, 32)), ("embedding_dict.feat_item.weight", (13, 32)), ("ffn_user.weight", (32, 32)),
            ("ffn_user.bias", (32,)), ("fnn_gate.weight", (32, 33)), ("fnn_gate.bias", (32,))]
    layer = lambda l, W: [(f"layers.{l}.filter.complex_weight", (W // 2 + 1, 32, 2)), (f"layers.{l}.filter.ln.weight", (32,)),  # noqa: E731
                          (f"layers.{l}.filter.ln.bias", (32,)), (f"layers.{l}.ffn.dense_1.weight", (128, 32)), (f"layers.{l}.ffn.dense_1.bias", (128,)),
                          (f"layers.{l}.ffn.dense_2.weight", (32, 128)), (f"layers.{l}.ffn.dense_2.bias", (32,)), (f"layers.{l}.ffn.ln.weight", (32,)),
                          (f"layers.{l}.ffn.ln.bias", (32,))]
    assert list(sh.items()) == head + layer(0, 10) + layer(1, 10) + [("decoder.weight", (20, 32)), ("decoder.bias", (20,))]
    assert len(sh) == 8 + 9 * 2 and len(fmlp_param_shapes(11, 13, 32, 20, 10, 1)) == 17
    assert fmlp_param_shapes(11, 13, 32, 7, 5, 1)["layers.0.filter.complex_weight"] == (3, 32, 2)
    assert fmlp_param_shapes(11, 13, 32, 7, 1, 1)["layers.0.filter.complex_weight"] == (1, 32, 2)
    assert [k for k in sh if _own(k)] == list(_Fmlp(10, 2, 20).state_dict())      # the order a torch module with these children lists them
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_fmlp_tracker_params(11, 13, seed=5, window_size=10, nlayers=2)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    from cirs_hip.engine import init_tracker_params
    ref = init_tracker_params(11, 13, 1, seed=5, dim_model=32, dim_state=20, nlayers=1)
    n_shared = 0
    for k in p:
        assert p[k].dtype == torch.float32 and torch.isfinite(p[k]).all(), k
        if k in ref:
            assert torch.equal(p[k], ref[k]), k
            n_shared += 1
    assert n_shared == 8
    for l in range(2):
        cw = p[f"layers.{l}.filter.complex_weight"]
        assert 0.012 < float(cw.std()) < 0.03, float(cw.std())      # 0.02 N(0, 1)
        assert torch.equal(p[f"layers.{l}.filter.ln.weight"], torch.ones(32)) and torch.equal(p[f"layers.{l}.ffn.ln.bias"], torch.zeros(32))
        assert 0 < p[f"layers.{l}.ffn.dense_1.weight"].abs().max() <= 1 / np.sqrt(32) + 1e-6
        assert 0 < p[f"layers.{l}.ffn.dense_2.weight"].abs().max() <= 1 / np.sqrt(128) + 1e-6
    again = init_fmlp_tracker_params(11, 13, seed=5, window_size=10, nlayers=2)
    assert all(torch.equal(again[k], p[k]) for k in p)
    assert not torch.equal(init_fmlp_tracker_params(11, 13, seed=6)["layers.0.ffn.dense_1.weight"], p["layers.0.ffn.dense_1.weight"])
    m = _Fmlp(10, 2, 20)
    m.load_state_dict({k: v for k, v in p.items() if _own(k)}, strict=True)
    c = fmlpcase.fmlp_param_dict(11, 13, 1, 10, 2)
    assert list(c) == list(sh) and {k: tuple(v.shape) for k, v in c.items()} == sh
    assert abs(float(c["layers.0.filter.complex_weight"].std()) - 0.5) < 0.1
    assert abs(float(c["layers.1.ffn.dense_2.weight"].std()) * np.sqrt(128) - 1.0) < 0.2
    assert abs(float(c["layers.1.ffn.ln.weight"].mean()) - 1.0) < 0.1
    from grucase import gru_param_dict
    base = gru_param_dict(11, 13, 1, nlayers=1)
    assert all(torch.equal(c[k], base[k]) for k in base if not k.startswith("gru."))


def test_check_shape_refusals_name_their_member():
    check_fmlp_shape(32, 20, 10, 2, 128, 101)
    check_fmlp_shape(32, 32, 1, 1)
    check_fmlp_shape(32, 1, 16, 2)
    for kw, word in [(dict(dim_model=16), "dim_model"), (dict(dim_state=0), "dim_state"), (dict(dim_state=33), "dim_state"),
                     (dict(window_size=0), "window_size"), (dict(window_size=17), "window_size"), (dict(nlayers=0), "nlayers"),
                     (dict(nlayers=3), "nlayers"), (dict(d_hid=64), "d_hid"), (dict(d_hid=256), "d_hid"), (dict(max_len=4097), "max_len"),
                     (dict(max_len=0), "max_len")]:
        args = dict(dim_model=32, dim_state=20, window_size=10, nlayers=2, d_hid=128, max_len=101)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            check_fmlp_shape(**args)


def test_slot_record():
    assert (SLOT.name, SLOT.display, SLOT.entry) == ("fmlp", "FMLP", "cirs_fmlp_tracker")
    assert SLOT.n_grad_tensors((3, 2)) == 26 and SLOT.n_grad_tensors((16, 1)) == 17
    assert SLOT.flags((3, 2)) == ["--window-size", "3", "--fmlp-layers", "2"] and SLOT.plugin_kw((3, 2)) == {"window_size": 3, "nlayers": 2}
    assert SLOT.split(SLOT.CASES[1]) == ((30, 40, 3, 100, 20, 0.0), (10, 2))
    assert [c[4] for c in SLOT.CASES] == [(3, 2), (10, 2), (16, 2), (16, 1), (1, 2), (2, 2), (5, 2), (10, 2)]
    assert len(SLOT.CASES) == len(SLOT.IDS) == 8 and SLOT.host is fmlp_host
    assert (SLOT.rollout_model, SLOT.plugin_model, SLOT.example_model) == ((3, 2), (3, 2), (2, 1))
    assert set(SLOT.state_names) <= set(fmlp_param_shapes(5, 6, 32, 20, 3, 2))
    assert type(SLOT).check_unambiguous is type(SLOT).__mro__[1].check_unambiguous      # smooth: the base's no-op
    # one env more than a launch holds without walking would do; 1030 leaves the last group ragged
    (B, T, model, seed), = SLOT.walk
    assert B > 4 * 1 * 256 and B % 4 != 0 and (T, model) == (4, (3, 2))
    refusals = SLOT.engine_refusals({})
    assert [r[1] for r in refusals] == ["window_size", "window_size", "nlayers"]
    for exc, pattern, thunk in refusals:      # refused before any device use
        with pytest.raises(exc, match=pattern):
            thunk()


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_fmlp_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerFMLP, _RecurrentStateTracker

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    assert issubclass(StateTrackerFMLP, _RecurrentStateTracker)      # what Collector(dropout_redraw=True) refuses
    uc, ac, fc = _columns()
    kw = dict(dim_model=32, dim_state=20, dim_max_batch=4)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="window_size"):
            StateTrackerFMLP(uc, ac, fc, window_size=bad, **kw)
    for bad in (0, 3):
        with pytest.raises(ValueError, match="nlayers"):
            StateTrackerFMLP(uc, ac, fc, nlayers=bad, **kw)
    for bad in (64, 2048):
        with pytest.raises(ValueError, match="d_hid"):
            StateTrackerFMLP(uc, ac, fc, d_hid=bad, **kw)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerFMLP(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerFMLP(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="max_len"):
        StateTrackerFMLP(uc, ac, fc, MAX_TURN=4096, **kw)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerFMLP(uc, ac, fc, dataset="VirtualTB-v0", **kw)
    with pytest.raises(TypeError):
        StateTrackerFMLP(uc, ac, fc, dilations=(1, 2), **kw)


def test_plugin_class_keywords_and_attributes_without_a_device(monkeypatch):
    from core.state_tracker import StateTrackerFMLP
    monkeypatch.setattr(StateTrackerFMLP, "_setup", lambda self, shapes, init, seed: None)      # no device: the flat buffer is not built
    uc, ac, fc = _columns()
    st = StateTrackerFMLP(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dropout=0.1, nhead=4)
    assert st.training      # dropout is accepted and unused: its two sites are not built
    assert (st.window_size, st.nlayers, st.d_hid, st.dropout_p, st.CELL) == (10, 1, 128, 0.0, "FMLP")
    assert st._model_kw() == {"window_size": 10, "nlayers": 1} == st._engine_kw()
    st = StateTrackerFMLP(uc, ac, fc, 32, 20, 4, 0.0, "KuaishouEnv-v0", True, True, False, 8, 128, 2, window_size=3)      # d_hid given by position
    assert (st.window_size, st.nlayers) == (3, 2)
    st.eval(); st.train()
    assert "dropout" in StateTrackerFMLP.__doc__ and "not built" in StateTrackerFMLP.__doc__


def test_library_refuses_the_same_cfgs_without_a_gpu():
    from cirs_hip import abi
    lib = abi.lib()

    def cfg_of(**kw):
        base = dict(n_users=3, n_items=4, dim_model=32, dim_state=20, window=3, nlayers=2, max_len=5, n_env=2)
        base.update(kw)
        return abi.FmlpCfg(**base)

    def refused(cfg, word):
        calls = [lambda: lib.cirs_fmlp_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_fmlp_tracker_init(C.byref(cfg), None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_fmlp_tracker_backward(C.byref(cfg), None, None, None, None, None, None, None, None, None, 4, None, None, None, 0,
                                                        None)]
        for call in calls:
            assert call() != 0
            assert word in lib.cirs_last_error(), (word, lib.cirs_last_error())
            assert lib.cirs_last_error().startswith(b"fmlp tracker:"), lib.cirs_last_error()
        if word != b"weights null":
            assert lib.cirs_fmlp_tracker_backward_workspace_bytes(C.byref(cfg), 7) == 0
    refused(cfg_of(window=0), b"window")
    refused(cfg_of(window=17), b"window")
    refused(cfg_of(nlayers=0), b"nlayers")
    refused(cfg_of(nlayers=3), b"nlayers")
    refused(cfg_of(dim_model=16), b"dim_model")
    refused(cfg_of(dim_state=0), b"dim_state")
    refused(cfg_of(dim_state=33), b"dim_state")
    refused(cfg_of(max_len=4097), b"max_len")
    refused(cfg_of(max_len=0), b"max_len")
    refused(cfg_of(n_env=0), b"n_env")
    good = cfg_of()
    refused(good, b"weights null")
    assert lib.cirs_fmlp_tracker_backward_workspace_bytes(C.byref(good), 0) == 0
    sizes = [lib.cirs_fmlp_tracker_backward_workspace_bytes(C.byref(good), r) for r in (1, 7, 100, 5000)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes)), sizes      # positive, and growing with n_rows
    assert lib.cirs_fmlp_tracker_backward_workspace_bytes(C.byref(cfg_of(nlayers=1)), 5000) < sizes[-1]      # a layer's keeps are per layer
    assert lib.cirs_fmlp_tracker_backward_workspace_bytes(C.byref(cfg_of(max_len=200)), 5000) == sizes[-1]    # O(rows), not O(rows x len)
    # a null member is named before any pointer is read: the weights struct with one member of layer 1 missing (layer 1 is read at nlayers = 2 only)
    one = C.c_float(0.0)
    ptr = C.addressof(one)

    def weights():
        w = abi.FmlpWeights()
        for k, t in abi.FmlpWeights._fields_:
            if t is C.c_void_p:
                setattr(w, k, ptr)
            else:
                getattr(w, k)[0] = ptr
                getattr(w, k)[1] = ptr
        return w
    w = weights()
    w.cw[1] = None
    assert lib.cirs_fmlp_tracker_step(C.byref(good), C.byref(w), None, None, None, None, None, 2, None, 20, None) != 0
    assert b"filter weight pointer null" in lib.cirs_last_error() and b"cw" in lib.cirs_last_error()
    one_layer = cfg_of(nlayers=1)
    assert lib.cirs_fmlp_tracker_init(C.byref(one_layer), C.byref(w), None, ptr, None, 2, ptr, 20, None) != 0
    assert b"state pointer null" in lib.cirs_last_error()      # layer 1 is not read: the refusal is the next one
    w = weights()
    w.d2_b[0] = None
    assert lib.cirs_fmlp_tracker_init(C.byref(good), C.byref(w), None, None, None, 2, None, 20, None) != 0
    assert b"feed-forward weight pointer null" in lib.cirs_last_error()
    w = weights()      # every weight present, the state struct missing: refused, nothing launched
    assert lib.cirs_fmlp_tracker_init(C.byref(good), C.byref(w), None, C.addressof(one), None, 2, C.addressof(one), 20, None) != 0
    assert b"state pointer null" in lib.cirs_last_error()
    assert C.sizeof(abi.FmlpCfg) == 8 * 4 and C.sizeof(abi.FmlpWeights) == (8 + 9 * 2) * 8 and C.sizeof(abi.FmlpState) == 2 * 8
