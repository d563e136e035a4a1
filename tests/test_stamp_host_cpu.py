"""CPU: the host restatement of the attention-pool tracker (cirs_hip/stamp_host.py) gives hand-computed answers at W = 1 and W = 2, equals
the same model assembled from torch.nn.Linear modules loaded by state_dict name, leaves a position bit-identical when a slot older than its
window changes (the property the device relies on), reduces to decoder(x_0) once the attention is cut, and its autograd equals the closed-form
per-row backward the device kernels implement (the product, the two tanh, both factors of m_a, the sigmoid tile, W1, c, rows outside the
window cleared, the window fold in ascending p, weight gradients as products over rows and over (row, tile row) pairs); the parameters carry
their names in order; StateTrackerSTAMP and the library refuse what is not built before they touch a device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import stampcase
from cirs_hip import stamp_host
from cirs_hip.stamp_tracker import check_stamp_shape, init_stamp_tracker_params, stamp_param_shapes
from stampcase import SLOT

D = 32
TILE = 16      # rows of the device's tile: row t of position p is slot p - 15 + t


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _hand_params(a, b, g, beta, alpha, bA, gamma, bB):
    """W1 = a I, W2 = b I, W3 = g I, b_a = beta, w0 = 1/32 in every column, A = alpha I, b_A = bA, B = gamma I, b_B = bB, decoder = identity"""
    eye = torch.eye(D, dtype=torch.float64)
    full = lambda v: torch.full((D,), v, dtype=torch.float64)  # noqa: E731
    return {"attn.w1.weight": a * eye, "attn.w2.weight": b * eye, "attn.w3.weight": g * eye, "attn.bias": full(beta),
            "attn.w0.weight": torch.full((1, D), 1.0 / D, dtype=torch.float64), "mlp_a.weight": alpha * eye, "mlp_a.bias": full(bA),
            "mlp_b.weight": gamma * eye, "mlp_b.bias": full(bB), "decoder.weight": eye.clone(), "decoder.bias": torch.zeros(D, dtype=torch.float64)}


def test_known_answers_at_window_one_and_two():
    """Slots v e with e the alternating +-1 vector and diagonal weights: every vector of the model is a multiple of e plus a constant, so a
    position is a few scalars.  For a slot v_k e the gate's argument is (a v_k + b v_t + g v_s) e + beta =: s_k e + beta, and with w0 = 1/32
    in every column e_k = (sigmoid(s_k + beta) + sigmoid(-s_k + beta)) / 2.  x_0 = 9, x_1 = e, x_2 = 3 e, x_3 = -2 e."""
    a, b, g, beta, alpha, bA, gamma, bB = 0.5, 0.25, -0.75, 0.3, 2.0, 0.1, 1.5, -0.2
    p = _hand_params(a, b, g, beta, alpha, bA, gamma, bB)
    e = torch.tensor([1.0, -1.0] * (D // 2), dtype=torch.float64)
    en = e.numpy()
    X = torch.zeros(1, 4, D, dtype=torch.float64)
    X[0, 0], X[0, 1], X[0, 2], X[0, 3] = 9.0, e, 3 * e, -2 * e
    v = [None, 1.0, 3.0, -2.0]

    def ek(vk, vt, vs):
        s = a * vk + b * vt + g * vs
        return 0.5 * (_sig(s + beta) + _sig(-s + beta))

    def h(va, vt):      # m_a = va e, m_t = vt e
        return 9.0 + np.tanh(alpha * va * en + bA) * np.tanh(gamma * vt * en + bB)

    # W = 1: m_s = m_t = x_p, one attention term
    s1 = stamp_host.states_from_slots(p, X, 1).numpy()[0]
    np.testing.assert_allclose(s1[0], np.full(D, 9.0), rtol=0, atol=0)                 # h_0 = x_0
    for q in (1, 2, 3):
        np.testing.assert_allclose(s1[q], h(ek(v[q], v[q], v[q]) * v[q], v[q]), rtol=0, atol=1e-14, err_msg=f"W=1 position {q}")
    # W = 2: position 1 has one slot, position 2 the slots {1, 2} (m_s = 2 e), position 3 the slots {2, 3} (m_s = e / 2): slot 1 has left
    s2 = stamp_host.states_from_slots(p, X, 2).numpy()[0]
    np.testing.assert_allclose(s2[1], s1[1], rtol=0, atol=0)
    np.testing.assert_allclose(s2[2], h(ek(1.0, 3.0, 2.0) * 1.0 + ek(3.0, 3.0, 2.0) * 3.0, 3.0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(s2[3], h(ek(3.0, -2.0, 0.5) * 3.0 + ek(-2.0, -2.0, 0.5) * -2.0, -2.0), rtol=0, atol=1e-14)
    assert np.abs(s2[2] - s1[2]).max() > 1e-3      # the window matters


def _case(ci, dtype=torch.float64):
    U, I, B, T, W, S, hot = stampcase.CASES[ci]
    p = stamp_host.cast_params(SLOT.params(ci), dtype)
    users, acts, rews, lens, rng = stampcase.teacher_inputs(U, I, B, T, hot)
    return p, stamp_host.input_slots(p, users, acts, rews), lens, rng


class _Attn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w1, self.w2, self.w3 = (torch.nn.Linear(D, D, bias=False) for _ in range(3))
        self.bias = torch.nn.Parameter(torch.zeros(D))
        self.w0 = torch.nn.Linear(D, 1, bias=False)


class _Stamp(torch.nn.Module):
    """the model's own tensors under their state_dict names"""
    def __init__(self, S):
        super().__init__()
        self.attn, self.mlp_a, self.mlp_b, self.decoder = _Attn(), torch.nn.Linear(D, D), torch.nn.Linear(D, D), torch.nn.Linear(D, S)


def _modules(p):
    m = _Stamp(p["decoder.weight"].shape[0]).to(p["decoder.weight"].dtype)
    m.load_state_dict({k: v for k, v in p.items() if k.split(".")[0] in ("attn", "mlp_a", "mlp_b", "decoder")}, strict=True)
    return m


@pytest.mark.parametrize("ci", range(len(stampcase.CASES)), ids=stampcase.IDS)
def test_restatement_equals_linear_modules_loaded_by_name(ci):
    U, I, B, T, W, S, hot = stampcase.CASES[ci]
    p, X, lens, _ = _case(ci)
    got = stamp_host.states_from_slots(p, X, W).numpy()
    m = _modules(p)
    assert len(m.state_dict()) == 11      # the nine tensors of the attention and the read-out, and the decoder's two
    with torch.no_grad():
        want = [m.decoder(X[:, 0])]
        for q in range(1, T + 1):
            n = min(W, q)
            win = X[:, q - n + 1:q + 1]                                              # [B, n, D], the whole window at once
            m_s, m_t = win.mean(1), X[:, q]
            e = m.attn.w0(torch.sigmoid(m.attn.w1(win) + (m.attn.w2(m_t) + m.attn.w3(m_s) + m.attn.bias).unsqueeze(1)))      # [B, n, 1]
            h = X[:, 0] + torch.tanh(m.mlp_a((e * win).sum(1))) * torch.tanh(m.mlp_b(m_t))
            want.append(m.decoder(h))
        want = torch.stack(want, 1).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("ci", range(len(stampcase.CASES)), ids=stampcase.IDS)
def test_a_slot_older_than_the_window_leaves_the_state_bit_identical(ci, dtype):
    """What the device relies on when it reads the window's rows only: position q is a function of x_0 and the slots q - n_q + 1 .. q.  Every
    item slot in front of the window is changed at once; the state keeps its bits.  Changing the window's first slot does move it (so the test
    can fail)."""
    U, I, B, T, W, S, hot = stampcase.CASES[ci]
    p, X, lens, _ = _case(ci, dtype)
    full = stamp_host.states_from_slots(p, X, W)
    checked = 0
    for q in sorted({1, min(W, T), min(W + 1, T), T}):
        first = q - min(W, q) + 1
        if first > 1:
            older = X.clone()
            older[:, 1:first] = older[:, 1:first] * -3.0 + 1.0
            assert torch.equal(stamp_host.states_from_slots(p, older, W)[:, q], full[:, q]), f"position {q}"
            checked += 1
        inside = X.clone()
        inside[:, first] = inside[:, first] * -3.0 + 1.0
        assert not torch.equal(stamp_host.states_from_slots(p, inside, W)[:, q], full[:, q]), f"position {q}"
    assert checked > 0 or W >= T      # a window that never slides has no older slot


@pytest.mark.parametrize("ci", range(len(stampcase.CASES)), ids=stampcase.IDS)
def test_without_the_attention_the_state_is_the_decoder_of_x0(ci):
    """attn.w0 = 0 makes every e_k zero, so m_a = 0 and h_s = tanh(b_A): with mlp_a.bias = 0 as well the product vanishes and the state is
    decoder(x_0) at every position, exactly.  (With attn.w0 = 0 alone the state is decoder(x_0 + tanh(b_A) * h_t): m_a no longer reaches
    it, h_t still does.)"""
    U, I, B, T, W, S, hot = stampcase.CASES[ci]
    p, X, lens, _ = _case(ci)
    p = dict(p)
    p["attn.w0.weight"] = torch.zeros_like(p["attn.w0.weight"])
    alone = stamp_host.states_from_slots(p, X, W)
    h_t = torch.tanh(X @ p["mlp_b.weight"].T + p["mlp_b.bias"])
    want = (X[:, :1] + torch.tanh(p["mlp_a.bias"]) * h_t) @ p["decoder.weight"].T + p["decoder.bias"]
    np.testing.assert_allclose(alone[:, 1:].numpy(), want[:, 1:].numpy(), rtol=0, atol=1e-12)
    p["mlp_a.bias"] = torch.zeros_like(p["mlp_a.bias"])
    got = stamp_host.states_from_slots(p, X, W)
    x0 = X[:, 0] @ p["decoder.weight"].T + p["decoder.bias"]
    for q in range(T + 1):
        assert torch.equal(got[:, q], x0), f"position {q}"


def _closed_form_backward(n, x, lens, dH, W):
    """Stages (F), (B), (W), (X) of the device backward in numpy, per live row (b, p): a 16-row tile (row t = slot p - 15 + t) that holds the
    window's rows and zero rows in front of them."""
    B, L, _ = x.shape
    W1, W2, W3, ba, w0 = n["attn.w1.weight"], n["attn.w2.weight"], n["attn.w3.weight"], n["attn.bias"], n["attn.w0.weight"][0]
    A, bA, Bm, bB = n["mlp_a.weight"], n["mlp_a.bias"], n["mlp_b.weight"], n["mlp_b.bias"]
    g = {k: np.zeros_like(n[k]) for k in stampcase.NEW}
    dX = np.zeros_like(x)
    for b in range(B):
        dwin = np.zeros((lens[b], TILE, D))
        for p in range(1, lens[b]):
            nw = min(W, p)
            first = TILE - nw
            tile = np.zeros((TILE, D))
            for t in range(first, TILE):
                tile[t] = x[b, p - (TILE - 1) + t]
            # (F) the forward again
            ms = tile[first]
            for t in range(first + 1, TILE):
                ms = ms + tile[t]
            ms = ms / nw
            mt = tile[TILE - 1]
            c = W2 @ mt + W3 @ ms + ba
            sg = _sig(tile @ W1.T + c)                       # [16, 32]
            e = sg @ w0
            e[:first] = 0.0
            ma = e @ tile
            hs, ht = np.tanh(A @ ma + bA), np.tanh(Bm @ mt + bB)
            # (B) one row
            dh = dH[b, p]
            dpa, dpb = dh * ht * (1 - hs * hs), dh * hs * (1 - ht * ht)
            dma, dmt = A.T @ dpa, Bm.T @ dpb
            de = tile @ dma
            de[:first] = 0.0
            dG = (de[:, None] * w0[None, :]) * sg * (1 - sg)
            dc = dG.sum(0)
            dw = e[:, None] * dma[None, :] + dG @ W1 + (W3.T @ dc)[None, :] / nw
            dw[TILE - 1] += W2.T @ dc + dmt
            dw[:first] = 0.0
            dwin[p] = dw
            # (W) products over rows and over (row, tile row) pairs
            g["mlp_a.weight"] += np.outer(dpa, ma); g["mlp_a.bias"] += dpa
            g["mlp_b.weight"] += np.outer(dpb, mt); g["mlp_b.bias"] += dpb
            g["attn.w1.weight"] += dG.T @ tile
            g["attn.w0.weight"] += (de @ sg)[None, :]
            g["attn.w2.weight"] += np.outer(dc, mt); g["attn.w3.weight"] += np.outer(dc, ms); g["attn.bias"] += dc
        # (X) the fold
        for p in range(lens[b]):
            dX[b, 0] += dH[b, p]
        for k in range(1, lens[b]):
            for p in range(k, min(lens[b] - 1, k + W - 1) + 1):
                dX[b, k] += dwin[p, k - p + TILE - 1]
    return dX, g


@pytest.mark.parametrize("ci", range(len(stampcase.CASES)), ids=stampcase.IDS)
def test_closed_form_backward_equals_autograd(ci):
    U, I, B, T, W, S, hot = stampcase.CASES[ci]
    p, X, lens, rng = _case(ci)
    G = rng.normal(size=(T + 1, B, S))
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    X = X.detach().clone().requires_grad_(True)
    up = stamp_host.upstream(G, lens, B, T + 1, torch.float64)
    (stamp_host.states_from_slots(p, X, W) * up).sum().backward()
    n = {k: v.detach().numpy() for k, v in p.items()}
    dH = up.numpy() @ n["decoder.weight"]                # [B, T+1, D]; rows p >= len are zero
    dX, g = _closed_form_backward(n, X.detach().numpy(), lens, dH, W)

    def close(got, want, what):
        scale = np.abs(want).max()
        assert scale > 0, what
        err = np.abs(got - want).max() / scale
        assert err <= 1e-10, (what, err)
    close(dX, X.grad.numpy(), "dX")
    assert set(g) == set(stampcase.NEW)
    for k, v in g.items():
        close(v, p[k].grad.numpy(), k)


def test_param_names_order_shapes_and_init():
    sh = stamp_param_shapes(11, 13, 32, 20)
    assert list(sh.items()) == [
        ("embedding_dict.feat_user.weight", (11, 32)), ("embedding_dict.feat_item.weight", (13, 32)), ("ffn_user.weight", (32, 32)),
        ("ffn_user.bias", (32,)), ("fnn_gate.weight", (32, 33)), ("fnn_gate.bias", (32,)),
        ("attn.bias", (32,)), ("attn.w1.weight", (32, 32)), ("attn.w2.weight", (32, 32)), ("attn.w3.weight", (32, 32)), ("attn.w0.weight", (1, 32)),
        ("mlp_a.weight", (32, 32)), ("mlp_a.bias", (32,)), ("mlp_b.weight", (32, 32)), ("mlp_b.bias", (32,)),
        ("decoder.weight", (20, 32)), ("decoder.bias", (20,))]
    assert len(sh) == 17 and stamp_param_shapes(11, 13, 32, 7)["decoder.weight"] == (7, 32)
    # the order a torch module with these children lists them in (its own tensors before its children's): what the plugin's state_dict gives
    assert [k for k in sh if k.split(".")[0] in ("attn", "mlp_a", "mlp_b", "decoder")] == list(_Stamp(20).state_dict())
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_stamp_tracker_params(11, 13, seed=5)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    # the shared tensors are drawn exactly as init_tracker_params draws them
    from cirs_hip.engine import init_tracker_params
    ref = init_tracker_params(11, 13, 5, seed=5)
    n_shared = 0
    for k in p:
        if k in ref:
            assert torch.equal(p[k], ref[k]), k
            n_shared += 1
        else:
            assert k in stampcase.NEW and p[k].dtype == torch.float32 and torch.isfinite(p[k]).all(), k
            if k == "attn.bias":
                assert (p[k] == 0).all()
            else:
                assert 0 < p[k].abs().max() <= 1 / np.sqrt(32) + 1e-6, k      # torch's default nn.Linear init
    assert n_shared == 8
    assert torch.equal(init_stamp_tracker_params(11, 13, seed=5)["mlp_b.weight"], p["mlp_b.weight"])
    assert not torch.equal(init_stamp_tracker_params(11, 13, seed=6)["mlp_b.weight"], p["mlp_b.weight"])
    # the init's own tensors load by name into the torch modules
    m = _modules(p)
    for k, v in m.state_dict().items():
        assert torch.equal(v, p[k]), k
    c = stampcase.stamp_param_dict(11, 13, 1)
    assert list(c) == list(sh) and {k: tuple(v.shape) for k, v in c.items()} == sh
    for k in stampcase.SQUARE + ("attn.w0.weight",):
        assert abs(float(c[k].std()) * np.sqrt(32) - 1.0) < 0.35, k
    for k in ("attn.bias", "mlp_a.bias", "mlp_b.bias"):
        assert 0.03 < float(c[k].std()) < 0.2, k


def test_check_shape_refusals_name_their_member():
    check_stamp_shape(32, 20, 10, 101)
    check_stamp_shape(32, 32, 16)
    check_stamp_shape(32, 1, 1)
    for kw, word in [(dict(dim_model=16), "dim_model"), (dict(dim_state=0), "dim_state"), (dict(dim_state=33), "dim_state"),
                     (dict(window_size=0), "window_size"), (dict(window_size=17), "window_size"), (dict(max_len=4097), "max_len"),
                     (dict(max_len=0), "max_len")]:
        args = dict(dim_model=32, dim_state=20, window_size=10, max_len=101)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            check_stamp_shape(**args)


def test_slot_record():
    assert (SLOT.name, SLOT.display, SLOT.entry) == ("stamp", "STAMP", "cirs_stamp_tracker")
    assert SLOT.n_grad_tensors(10) == 17 and SLOT.flags(10) == ["--window-size", "10"] and SLOT.plugin_kw(3) == {"window_size": 3}
    assert SLOT.split(SLOT.CASES[2]) == ((120, 200, 33, 20, 20, 0.0), 16)
    assert len(SLOT.CASES) == len(SLOT.IDS) == 6 and SLOT.host is stamp_host
    assert (SLOT.rollout_model, SLOT.plugin_model) == (3, 3)
    assert type(SLOT).check_unambiguous is type(SLOT).__mro__[1].check_unambiguous      # smooth: the base's no-op
    refusals = SLOT.engine_refusals({})
    assert len(refusals) == 2
    for exc, pattern, thunk in refusals:      # window 0 and window 17: refused before any device use
        with pytest.raises(exc, match=pattern):
            thunk()


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_stamp_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerSTAMP, _RecurrentStateTracker

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    assert issubclass(StateTrackerSTAMP, _RecurrentStateTracker)      # what Collector(dropout_redraw=True) refuses
    uc, ac, fc = _columns()
    kw = dict(dim_model=32, dim_state=20, dim_max_batch=4)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="window_size"):
            StateTrackerSTAMP(uc, ac, fc, window_size=bad, **kw)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerSTAMP(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerSTAMP(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="max_len"):
        StateTrackerSTAMP(uc, ac, fc, MAX_TURN=4096, **kw)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerSTAMP(uc, ac, fc, dataset="VirtualTB-v0", **kw)
    with pytest.raises(TypeError):
        StateTrackerSTAMP(uc, ac, fc, dilations=(1, 2), **kw)


def test_plugin_class_keywords_and_attributes_without_a_device(monkeypatch):
    from core.state_tracker import StateTrackerSTAMP
    monkeypatch.setattr(StateTrackerSTAMP, "_setup", lambda self, shapes, init, seed: None)      # no device: the flat buffer is not built
    uc, ac, fc = _columns()
    st = StateTrackerSTAMP(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dropout=0.1, nhead=4, d_hid=64, nlayers=3)
    assert st.training      # dropout is accepted and unused: the model has no dropout site
    assert st.window_size == 10 and st.dropout_p == 0.0 and st.nlayers == 0 and st.CELL == "STAMP"
    assert st._model_kw() == {} and st._engine_kw() == {"window_size": 10}
    st.eval(); st.train()
    st = StateTrackerSTAMP(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, window_size=16)
    assert st.window_size == 16 and isinstance(st.window_size, int)


def test_library_refuses_the_same_cfgs_without_a_gpu():
    from cirs_hip import abi
    lib = abi.lib()

    def cfg_of(**kw):
        base = dict(n_users=3, n_items=4, dim_model=32, dim_state=20, window=10, max_len=5, n_env=2)
        base.update(kw)
        return abi.StampCfg(**base)

    def refused(cfg, word):
        calls = [lambda: lib.cirs_stamp_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_stamp_tracker_init(C.byref(cfg), None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_stamp_tracker_backward(C.byref(cfg), None, None, None, None, None, None, None, None, None, 4, None, None, None, 0,
                                                         None)]
        for call in calls:
            assert call() != 0
            assert word in lib.cirs_last_error(), (word, lib.cirs_last_error())
            assert b"stamp tracker" in lib.cirs_last_error()
        if word != b"weights null":
            assert lib.cirs_stamp_tracker_backward_workspace_bytes(C.byref(cfg), 7) == 0
    refused(cfg_of(window=0), b"window")
    refused(cfg_of(window=17), b"window")
    refused(cfg_of(window=-3), b"window")
    refused(cfg_of(dim_model=16), b"dim_model")
    refused(cfg_of(dim_state=0), b"dim_state")
    refused(cfg_of(dim_state=33), b"dim_state")
    refused(cfg_of(max_len=4097), b"max_len")
    for good in (cfg_of(), cfg_of(window=1), cfg_of(window=16)):
        refused(good, b"weights null")
        assert lib.cirs_stamp_tracker_backward_workspace_bytes(C.byref(good), 0) == 0
        assert lib.cirs_stamp_tracker_backward_workspace_bytes(C.byref(good), 7) > 0
    # a null member is named before any pointer is read: the weights struct with one group of members missing
    one = C.c_float(0.0)
    ptr = C.addressof(one)
    w = abi.StampWeights(**{k: ptr for k, _ in abi.StampWeights._fields_})
    w.w3 = None
    assert lib.cirs_stamp_tracker_step(C.byref(cfg_of()), C.byref(w), None, None, None, None, None, 2, None, 20, None) != 0
    assert b"attention weight pointer null" in lib.cirs_last_error() and b"w3" in lib.cirs_last_error()
    w = abi.StampWeights(**{k: ptr for k, _ in abi.StampWeights._fields_})
    w.mlp_b_b = None
    assert lib.cirs_stamp_tracker_init(C.byref(cfg_of()), C.byref(w), None, None, None, 2, None, 20, None) != 0
    assert b"read-out weight pointer null" in lib.cirs_last_error()
    assert C.sizeof(abi.StampCfg) == 7 * 4 and C.sizeof(abi.StampWeights) == 17 * 8 and C.sizeof(abi.StampState) == 2 * 8
