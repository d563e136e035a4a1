"""CPU: the host restatement of the convolutional window tracker (cirs_hip/caser_host.py) gives the known answers, equals torch's
conv2d -> relu -> max_pool1d plus the vertical conv2d, its autograd equals the closed-form backward the device kernels implement (arg-max
routing, window fold in ascending p, bank gradients as products over (row, position) pairs); the parameters carry torch's names;
StateTrackerCaser and the library refuse what is not built before they touch a device; and the cases' inputs are ones where float64 itself
is unambiguous at every max and every ReLU (the near-tie condition)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import casercase
from cirs_hip import caser_host
from cirs_hip.caser_tracker import caser_param_shapes, init_caser_tracker_params

D = 32


def _hand_params(heights, W, nf=2):
    p = {f"horizontal_cnn.{i}.weight": torch.zeros(nf, 1, h, D, dtype=torch.float64) for i, h in enumerate(heights)}
    p.update({f"horizontal_cnn.{i}.bias": torch.zeros(nf, dtype=torch.float64) for i in range(len(heights))})
    p.update({"vertical_cnn.weight": torch.zeros(1, 1, W, 1, dtype=torch.float64), "vertical_cnn.bias": torch.zeros(1, dtype=torch.float64),
              "fc.weight": torch.zeros(D, nf * len(heights) + D, dtype=torch.float64), "fc.bias": torch.zeros(D, dtype=torch.float64)})
    return p


def test_known_answer_a_zero_row_patch_wins_through_a_positive_bias():
    """W = 3, h = 2, window = [0, 0, 1]: patch 0 is all zero rows (c = bias), patch 1 sums one row of ones.  Filter 0 (weights -1/32, bias
    +0.25): c = [0.25, -0.75] -> the zero patch wins, o = 0.25.  Filter 1 (weights +1/32, bias -0.5): c = [-0.5, 0.5] -> o = 0.5."""
    W = 3
    p = _hand_params((2,), W)
    p["horizontal_cnn.0.weight"][0] = -1.0 / D
    p["horizontal_cnn.0.weight"][1] = 1.0 / D
    p["horizontal_cnn.0.bias"][:] = torch.tensor([0.25, -0.5])
    p["vertical_cnn.weight"][0, 0, :, 0] = torch.tensor([5.0, 7.0, 0.5])
    p["vertical_cnn.bias"][0] = -0.25
    X = torch.zeros(1, 2, D, dtype=torch.float64)      # x_0 (never in the window) and x_1 = ones
    X[0, 0] = 9.0
    X[0, 1] = 1.0
    win = caser_host.windows(X, W)
    assert win.shape == (1, 2, W, D) and (win[0, 0] == 0).all() and (win[0, 1, :2] == 0).all() and (win[0, 1, 2] == 1).all()
    cs, vpre = caser_host.pre_activations(p, win[0])
    np.testing.assert_allclose(cs[0][1].numpy(), [[0.25, -0.75], [-0.5, 0.5]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(cs[0][0].numpy(), [[0.25, 0.25], [-0.5, -0.5]], rtol=0, atol=0)      # position 0: every patch is all zero rows
    cat, _ = caser_host.features(p, win[0])
    np.testing.assert_allclose(cat[1, :2].numpy(), [0.25, 0.5], rtol=0, atol=1e-15)
    np.testing.assert_allclose(cat[0, :2].numpy(), [0.25, 0.0], rtol=0, atol=0)
    np.testing.assert_allclose(cat[1, 2:].numpy(), np.full(D, 0.25), rtol=0, atol=0)                # vertical: relu(-0.25 + 0.5 * 1)
    assert (cat[0, 2:] == 0).all()                                                                   # relu(-0.25)


def test_known_answer_height_w_gives_a_single_position():
    W = 4
    p = _hand_params((4,), W, nf=1)
    p["horizontal_cnn.0.weight"][0, 0] = torch.arange(1, W + 1, dtype=torch.float64)[:, None].expand(W, D) / D
    p["horizontal_cnn.0.bias"][0] = 0.5
    win = torch.stack([torch.full((D,), float(v), dtype=torch.float64) for v in (0, 0, 2, 3)])[None]      # [1, W, D]
    cs, _ = caser_host.pre_activations(p, win)
    assert cs[0].shape == (1, 1, 1)
    assert cs[0].item() == 0.5 + 3 * 2 + 4 * 3
    # identity fc and decoder: the state is x_0 + the concatenation's last 32 entries; here fc picks o_0 into every lane
    p["fc.weight"][:, 0] = 1.0
    p["decoder.weight"], p["decoder.bias"] = torch.eye(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    X = torch.zeros(1, 4, D, dtype=torch.float64)
    X[0, 0], X[0, 1], X[0, 2] = 1.0, 2.0, 3.0
    s = caser_host.states_from_slots(p, X, W).numpy()
    assert (s[0, 0] == 1.5).all() and (s[0, 2] == 1.0 + 0.5 + 3 * 2 + 4 * 3).all()      # position 2: window [0, 0, x_1, x_2]


def _case(ci, dtype=torch.float64):
    U, I, B, T, W, heights, S, hot = casercase.CASES[ci]
    p = caser_host.cast_params(casercase.case_params(ci), dtype)
    users, acts, rews, lens, rng = casercase.teacher_inputs(U, I, B, T, hot)
    return p, caser_host.input_slots(p, users, acts, rews), lens, rng


@pytest.mark.parametrize("ci", range(len(casercase.CASES)), ids=casercase.IDS)
def test_restatement_equals_torch_conv2d_relu_max_pool1d(ci):
    U, I, B, T, W, heights, S, hot = casercase.CASES[ci]
    p, X, lens, _ = _case(ci)
    got = caser_host.states_from_slots(p, X, W).numpy()
    win = caser_host.windows(X, W).reshape(B * (T + 1), 1, W, D)
    outs = []
    for i, h in enumerate(heights):
        c = F.relu(F.conv2d(win, p[f"horizontal_cnn.{i}.weight"], p[f"horizontal_cnn.{i}.bias"])).squeeze(3)      # [N, F, W - h + 1]
        outs.append(F.max_pool1d(c, c.shape[2]).squeeze(2))
    v = F.relu(F.conv2d(win, p["vertical_cnn.weight"], p["vertical_cnn.bias"])).reshape(-1, D)
    z = F.relu(F.linear(torch.cat(outs + [v], 1), p["fc.weight"], p["fc.bias"])).reshape(B, T + 1, D)
    want = F.linear(X[:, :1] + z, p["decoder.weight"], p["decoder.bias"]).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("ci", range(len(casercase.CASES)), ids=casercase.IDS)
def test_closed_form_backward_equals_autograd(ci):
    """What the device kernels compute, in numpy: per live row the forward again with the FIRST maximal t, dZ = dH [z > 0], dCAT = dZ fc,
    dO = dCAT [o > 0] at its arg-max, dV = dCAT [v > 0]; bank i's weight gradient = sum over (row, t) of DC[row, t, f] patch[row, t]; and
    dX[b,0] = sum_p dH[b,p], dX[b,k] = sum_{p=k}^{min(len-1, k+W-1)} dWin_p[k-p+W-1] in ascending p."""
    U, I, B, T, W, heights, S, hot = casercase.CASES[ci]
    p, X, lens, rng = _case(ci)
    G = rng.normal(size=(T + 1, B, S))
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    X = X.detach().clone().requires_grad_(True)
    up = caser_host.upstream(G, lens, B, T + 1, torch.float64)
    (caser_host.states_from_slots(p, X, W) * up).sum().backward()
    n = {k: v.detach().numpy() for k, v in p.items()}
    x = X.detach().numpy()
    nh, nf = len(heights), casercase.NUM_FILTERS
    dH = up.numpy() @ n["decoder.weight"]                # [B, T+1, D]; rows p >= len are zero
    wv, fc = n["vertical_cnn.weight"].reshape(-1), n["fc.weight"]
    wh = [n[f"horizontal_cnn.{i}.weight"][:, 0] for i in range(nh)]
    dX = np.zeros_like(x)
    g_wh, g_bh = [np.zeros_like(w) for w in wh], [np.zeros(nf) for _ in wh]
    g_wv, g_bv, g_fc, g_fcb = np.zeros(W), 0.0, np.zeros_like(fc), np.zeros(D)
    for b in range(B):
        dwin = np.zeros((lens[b], W, D))
        for q in range(lens[b]):
            win = np.stack([x[b, q - W + 1 + j] if q - W + 1 + j >= 1 else np.zeros(D) for j in range(W)])
            cat, arg = np.zeros(nf * nh + D), []
            for i, h in enumerate(heights):
                c = np.stack([(wh[i] * win[t:t + h]).sum((1, 2)) for t in range(W - h + 1)], 1) + n[f"horizontal_cnn.{i}.bias"][:, None]
                arg.append(c.argmax(1))                  # numpy: the first maximal t
                cat[i * nf:(i + 1) * nf] = np.maximum(c.max(1), 0)
            cat[nf * nh:] = np.maximum(wv @ win + n["vertical_cnn.bias"], 0)
            z = np.maximum(fc @ cat + n["fc.bias"], 0)
            dz = dH[b, q] * (z > 0)
            g_fc += np.outer(dz, cat); g_fcb += dz
            dcat = (dz @ fc) * (cat > 0)
            dv = dcat[nf * nh:]
            g_wv += win @ dv; g_bv += dv.sum()
            dwin[q] = wv[:, None] * dv[None, :]
            for i, h in enumerate(heights):
                for f in range(nf):
                    a, do = arg[i][f], dcat[i * nf + f]
                    g_wh[i][f] += do * win[a:a + h]; g_bh[i][f] += do
                    dwin[q, a:a + h] += do * wh[i][f]
        for q in range(lens[b]):
            dX[b, 0] += dH[b, q]
        for k in range(1, lens[b]):
            for q in range(k, min(lens[b] - 1, k + W - 1) + 1):
                dX[b, k] += dwin[q, k - q + W - 1]

    def close(got, want, what):
        scale = np.abs(want).max()
        np.testing.assert_allclose(got / scale, want / scale, rtol=0, atol=1e-12, err_msg=what)
    close(dX, X.grad.numpy(), "dX")
    close(g_fc, p["fc.weight"].grad.numpy(), "fc.weight"); close(g_fcb, p["fc.bias"].grad.numpy(), "fc.bias")
    close(g_wv, p["vertical_cnn.weight"].grad.numpy().reshape(-1), "vertical_cnn.weight")
    close(np.array([g_bv]), p["vertical_cnn.bias"].grad.numpy(), "vertical_cnn.bias")
    for i in range(nh):
        close(g_wh[i], p[f"horizontal_cnn.{i}.weight"].grad.numpy()[:, 0], f"horizontal_cnn.{i}.weight")
        close(g_bh[i], p[f"horizontal_cnn.{i}.bias"].grad.numpy(), f"horizontal_cnn.{i}.bias")


@pytest.mark.parametrize("ci", range(len(casercase.CASES)), ids=casercase.IDS)
def test_no_case_sits_near_a_tie(ci):
    """The condition under which a float32 forward takes the branches float64 takes: every quantity at which the gradient is discontinuous
    is at least 8 x the float32 restatement's own maximum error on that quantity away from its kink.  8: the device's error on the other
    trackers was at most about 1.6 x the float32 restatement's; the factor leaves room for a different summation order."""
    U, I, B, T, W, heights, S, hot = casercase.CASES[ci]
    users, acts, rews, lens, _ = casercase.teacher_inputs(U, I, B, T, hot)
    for what, (margin, err32) in casercase.near_tie_margins(casercase.case_params(ci), users, acts, rews, lens, W).items():
        print(f"near-tie {casercase.IDS[ci]} {what}: min {margin:.3e}  float32 restatement error {err32:.3e}  ratio {margin / max(err32, 1e-300):.1f}")
        assert margin >= 8 * err32, what


def test_param_names_order_shapes_and_init():
    sh = caser_param_shapes(11, 13, 32, 20, 10, (2, 3, 4))
    assert list(sh.items()) == [
        ("embedding_dict.feat_user.weight", (11, 32)), ("embedding_dict.feat_item.weight", (13, 32)), ("ffn_user.weight", (32, 32)),
        ("ffn_user.bias", (32,)), ("fnn_gate.weight", (32, 33)), ("fnn_gate.bias", (32,)),
        ("horizontal_cnn.0.weight", (16, 1, 2, 32)), ("horizontal_cnn.0.bias", (16,)), ("horizontal_cnn.1.weight", (16, 1, 3, 32)),
        ("horizontal_cnn.1.bias", (16,)), ("horizontal_cnn.2.weight", (16, 1, 4, 32)), ("horizontal_cnn.2.bias", (16,)),
        ("vertical_cnn.weight", (1, 1, 10, 1)), ("vertical_cnn.bias", (1,)), ("fc.weight", (32, 80)), ("fc.bias", (32,)),
        ("decoder.weight", (20, 32)), ("decoder.bias", (20,))]
    assert caser_param_shapes(11, 13, 32, 7, 4, (1, 4))["fc.weight"] == (32, 64)
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_caser_tracker_params(11, 13, seed=5)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    # the shared tensors are drawn as init_tracker_params draws them, whatever the window and the banks
    from cirs_hip.engine import init_tracker_params
    ref = init_tracker_params(11, 13, 5, seed=5)
    q = init_caser_tracker_params(11, 13, seed=5, window_size=4, filter_sizes=(1, 4))
    for k in p:
        if k in ref:
            assert torch.equal(p[k], ref[k]) and torch.equal(q[k], ref[k]), k
        else:
            assert p[k].abs().max() > 0 and torch.isfinite(p[k]).all(), k
    assert torch.equal(init_caser_tracker_params(11, 13, seed=5)["fc.weight"], p["fc.weight"])
    assert not torch.equal(init_caser_tracker_params(11, 13, seed=6)["fc.weight"], p["fc.weight"])
    c = casercase.caser_param_dict(11, 13, 1, 10, (2, 3, 4))
    assert list(c) == list(sh) and {k: tuple(v.shape) for k, v in c.items()} == sh
    b = torch.cat([c[k].reshape(-1) for k in c if k.endswith("cnn.0.bias") or k == "fc.bias"])
    assert (b > 0).any() and (b < 0).any() and (b.abs() >= 0.05).all()


def test_filters_round_trip_through_conv2d_modules_by_name():
    W, heights = 10, (2, 3, 4)
    p = init_caser_tracker_params(11, 13, seed=5, window_size=W, filter_sizes=heights)
    hor = torch.nn.ModuleList([torch.nn.Conv2d(1, 16, (h, 32)) for h in heights])
    ver = torch.nn.Conv2d(1, 1, (W, 1))
    hor.load_state_dict({k[len("horizontal_cnn."):]: v for k, v in p.items() if k.startswith("horizontal_cnn.")}, strict=True)
    ver.load_state_dict({k[len("vertical_cnn."):]: v for k, v in p.items() if k.startswith("vertical_cnn.")}, strict=True)
    back = {"horizontal_cnn." + k: v for k, v in hor.state_dict().items()}
    back.update({"vertical_cnn." + k: v for k, v in ver.state_dict().items()})
    assert set(back) == {k for k in p if "cnn" in k}
    for k, v in back.items():
        assert torch.equal(v, p[k]), k
    # and the modules compute what the restatement computes
    win = torch.randn(5, W, 32, generator=torch.Generator().manual_seed(0))
    cs, vpre = caser_host.pre_activations(p, win)
    with torch.no_grad():
        for i in range(len(heights)):
            np.testing.assert_allclose(hor[i](win[:, None]).squeeze(3).numpy(), cs[i].numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(ver(win[:, None]).reshape(5, 32).numpy(), vpre.numpy(), rtol=0, atol=1e-5)


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


BAD_FILTERS = [((0, 2), 10), ((2, 5), 10), ((3, 2), 10), ((2, 2), 10), ((), 10), ((2, 3, 4), 3), ((2, 3), 17), ((2,), 0)]


def test_state_tracker_caser_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerCaser, _RecurrentStateTracker

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    assert issubclass(StateTrackerCaser, _RecurrentStateTracker)      # what Collector(dropout_redraw=True) refuses
    uc, ac, fc = _columns()
    kw = dict(dim_model=32, dim_state=20, dim_max_batch=4)
    for hs, W in BAD_FILTERS:
        with pytest.raises(ValueError, match="filter_sizes"):
            StateTrackerCaser(uc, ac, fc, window_size=W, filter_sizes=hs, **kw)
    for W in (17, 3, 0):
        with pytest.raises(ValueError, match="window_size"):
            StateTrackerCaser(uc, ac, fc, window_size=W, **kw)
    with pytest.raises(ValueError, match="num_filters"):
        StateTrackerCaser(uc, ac, fc, num_filters=8, **kw)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerCaser(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerCaser(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="max_len"):
        StateTrackerCaser(uc, ac, fc, MAX_TURN=4096, **kw)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerCaser(uc, ac, fc, dataset="VirtualTB-v0", **kw)
    with pytest.raises(ValueError, match="dropout"):
        StateTrackerCaser(uc, ac, fc, dropout=0.1, **kw)


def test_dropout_is_refused_in_training_mode_only(monkeypatch):
    from core.state_tracker import StateTrackerCaser
    monkeypatch.setattr(StateTrackerCaser, "_setup", lambda self, shapes, init, seed: None)      # no device: the flat buffer is not built
    uc, ac, fc = _columns()
    st = StateTrackerCaser(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dropout=0.0, nhead=4, d_hid=64, nlayers=3)
    assert st.window_size == 10 and st.filter_sizes == (2, 3, 4) and st.num_filters == 16
    st.eval()
    st.dropout_p = 0.1
    st.eval()
    with pytest.raises(ValueError, match="dropout"):
        st.train()
    st.dropout_p = 0.0
    st.train()


def test_library_refuses_the_same_cfgs_without_a_gpu():
    from cirs_hip import abi
    lib = abi.lib()

    def cfg_of(W=10, hs=(2, 3, 4), **kw):
        base = dict(n_users=3, n_items=4, dim_model=32, dim_state=20, window=W, max_len=5, n_env=2, n_heights=len(hs))
        base.update(kw)
        return abi.CaserCfg(heights=(C.c_int32 * 4)(*(tuple(hs) + (0,) * (4 - len(hs)))), **base)

    def refused(cfg, word):
        calls = [lambda: lib.cirs_caser_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_caser_tracker_init(C.byref(cfg), None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_caser_tracker_backward(C.byref(cfg), None, None, None, None, None, None, None, None, None, 4, None, None, None, 0, None)]
        for call in calls:
            assert call() != 0
            assert word in lib.cirs_last_error(), (word, lib.cirs_last_error())
        if word != b"weights null":
            assert lib.cirs_caser_tracker_backward_workspace_bytes(C.byref(cfg), 7) == 0
    for hs, W in BAD_FILTERS:
        if len(hs) == 0:
            refused(cfg_of(W, hs), b"n_heights")
        elif W in (0, 17):
            refused(cfg_of(W, hs), b"window")
        else:
            refused(cfg_of(W, hs), b"heights")
    refused(cfg_of(n_heights=5), b"n_heights")
    refused(cfg_of(dim_model=16), b"dim_model")
    refused(cfg_of(dim_state=0), b"dim_state")
    refused(cfg_of(dim_state=33), b"dim_state")
    refused(cfg_of(max_len=4097), b"max_len")
    good = cfg_of()
    refused(good, b"weights null")
    assert lib.cirs_caser_tracker_backward_workspace_bytes(C.byref(good), 0) == 0
    assert lib.cirs_caser_tracker_backward_workspace_bytes(C.byref(good), 7) > 0
    assert C.sizeof(abi.CaserCfg) == 12 * 4 and C.sizeof(abi.CaserWeights) == 20 * 8 and C.sizeof(abi.CaserState) == 2 * 8
