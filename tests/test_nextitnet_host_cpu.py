"""CPU: the host restatement of the dilated-convolution tracker (cirs_hip/nextitnet_host.py) gives a hand-computed answer, equals a stack of
nn.Conv1d / nn.LayerNorm modules loaded by name, gives the same state from the last R slots alone (the property the device relies on), and
its autograd equals the closed-form per-row cone backward the device kernels implement (ReLU mask, LayerNorm backward, the three taps
transposed, rows before the first item cleared at every level, window fold in ascending p, tap gradients as products over (row, tile row)
pairs); the parameters carry torch's names; StateTrackerNextItNet and the library refuse what is not built before they touch a device; and
the cases' inputs are ones where float64 itself is unambiguous at every ReLU (the near-tie condition)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import nextitnetcase
from cirs_hip import nextitnet_host
from cirs_hip.nextitnet_tracker import check_nextitnet_shape, init_nextitnet_tracker_params, nextitnet_param_shapes
from nextitnetcase import SLOT

D = 32
TILE = 16      # rows of the device's tile: row t of position p is slot p - 15 + t


def test_known_answer_two_items_one_block():
    """One block, dilation 1, weights W[:, :, j] = w_j I / ... chosen so that c is hand-computable: tap 2 (the position itself) = 1 * I, tap 1
    (one back) = 2 * I, tap 0 = 4 * I; bias 0.5.  x_1 = e (the alternating +-1 vector), x_2 = 3 e:  c_1 = 0.5 + x_1 (both other taps read
    padding), c_2 = 0.5 + x_2 + 2 x_1 = 0.5 + 5 e.  LayerNorm of 0.5 + a e over 32 channels (mean 0.5, variance a^2): e * a / sqrt(a^2 + eps);
    with ln.weight 2 and ln.bias 0.25: n = 0.25 + 2 e a / sqrt(a^2 + eps); y = x + relu(n)."""
    e = torch.tensor([1.0, -1.0] * (D // 2), dtype=torch.float64)
    eye = torch.eye(D, dtype=torch.float64)
    p = {"blocks.0.conv.weight": torch.stack([4 * eye, 2 * eye, 1 * eye], -1), "blocks.0.conv.bias": torch.full((D,), 0.5, dtype=torch.float64),
         "blocks.0.ln.weight": torch.full((D,), 2.0, dtype=torch.float64), "blocks.0.ln.bias": torch.full((D,), 0.25, dtype=torch.float64),
         "decoder.weight": eye.clone(), "decoder.bias": torch.zeros(D, dtype=torch.float64)}
    X = torch.zeros(1, 3, D, dtype=torch.float64)
    X[0, 0], X[0, 1], X[0, 2] = 9.0, e, 3 * e
    s = nextitnet_host.states_from_slots(p, X, (1,)).numpy()[0]
    en = e.numpy()

    def y(x, a):
        return x + np.maximum(0.25 + 2 * en * a / np.sqrt(a * a + 1e-5), 0)
    np.testing.assert_allclose(s[0], np.full(D, 9.0), rtol=0, atol=0)                 # h_0 = x_0: x_0 is never convolved
    np.testing.assert_allclose(s[1], 9.0 + y(en, 1.0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(s[2], 9.0 + y(3 * en, 5.0), rtol=0, atol=1e-14)


def _case(ci, dtype=torch.float64):
    U, I, B, T, dil, S, hot = nextitnetcase.CASES[ci]
    p = nextitnet_host.cast_params(nextitnetcase.case_params(ci), dtype)
    users, acts, rews, lens, rng = nextitnetcase.teacher_inputs(U, I, B, T, hot)
    return p, nextitnet_host.input_slots(p, users, acts, rews), lens, rng


def _modules(p, dilations):
    blocks = torch.nn.ModuleList([torch.nn.ModuleDict({"conv": torch.nn.Conv1d(D, D, 3, dilation=int(d)), "ln": torch.nn.LayerNorm(D)}) for d in dilations])
    blocks = blocks.to(p["blocks.0.conv.weight"].dtype)
    blocks.load_state_dict({k[len("blocks."):]: v for k, v in p.items() if k.startswith("blocks.")}, strict=True)
    return blocks


@pytest.mark.parametrize("ci", range(len(nextitnetcase.CASES)), ids=nextitnetcase.IDS)
def test_restatement_equals_conv1d_and_layernorm_modules_loaded_by_name(ci):
    U, I, B, T, dil, S, hot = nextitnetcase.CASES[ci]
    p, X, lens, _ = _case(ci)
    got = nextitnet_host.states_from_slots(p, X, dil).numpy()
    blocks = _modules(p, dil)
    with torch.no_grad():
        y = X[:, 1:].transpose(1, 2)                                             # [B, D, T]
        for blk, d in zip(blocks, dil):
            c = blk["conv"](torch.cat([torch.zeros(B, D, 2 * d, dtype=y.dtype), y], 2))      # causal left padding
            y = y + torch.relu(blk["ln"](c.transpose(1, 2))).transpose(1, 2)
        h = X[:, :1] + torch.cat([torch.zeros(B, 1, D, dtype=y.dtype), y.transpose(1, 2)], 1)
        want = torch.nn.functional.linear(h, p["decoder.weight"], p["decoder.bias"]).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("ci", range(len(nextitnetcase.CASES)), ids=nextitnetcase.IDS)
def test_the_last_r_slots_alone_give_the_same_state(ci):
    """What the device relies on: position p from x_0 and its last R = 1 + 2 sum(d) item slots alone -- the restatement's own padding puts the
    zero rows in front of them, at every layer's input -- equals position p of the full-sequence evaluation.  One slot fewer does not (so the
    test can fail): the cone really is R slots wide."""
    U, I, B, T, dil, S, hot = nextitnetcase.CASES[ci]
    p, X, lens, _ = _case(ci)
    full = nextitnet_host.states_from_slots(p, X, dil).numpy()
    R = nextitnet_host.receptive_field(dil)
    assert R == 1 + 2 * sum(dil)
    for q in range(1, T + 1):
        lo = max(1, q - R + 1)
        alone = nextitnet_host.states_from_slots(p, torch.cat([X[:, :1], X[:, lo:q + 1]], 1), dil).numpy()[:, -1]
        np.testing.assert_allclose(alone, full[:, q], rtol=0, atol=1e-12, err_msg=f"position {q}")
    if T >= R:
        short = nextitnet_host.states_from_slots(p, torch.cat([X[:, :1], X[:, T - R + 2:T + 1]], 1), dil).numpy()[:, -1]
        assert np.abs(short - full[:, T]).max() > 1e-6


def _cone_backward(n, x, lens, dH, dil):
    """The algorithm of stages (F), (B), (W), (X) in numpy, per live row (b, p): a 16-row tile (row t = slot p - 15 + t, zero rows before the first
    item kept zero after every block), every block on all 16 rows, the backward from the top block down starting from dH at row 15."""
    B, L, _ = x.shape
    nb = len(dil)
    W = [n[f"blocks.{l}.conv.weight"] for l in range(nb)]
    g = {f"blocks.{l}.{k}": np.zeros_like(n[f"blocks.{l}.{k}"]) for l in range(nb) for k in ("conv.weight", "conv.bias", "ln.weight", "ln.bias")}
    dX = np.zeros_like(x)
    R = 1 + 2 * sum(dil)
    for b in range(B):
        dwin = np.zeros((lens[b], TILE, D))
        for p in range(lens[b]):
            item = np.array([p - (TILE - 1) + t >= 1 for t in range(TILE)])
            y = np.stack([x[b, p - (TILE - 1) + t] if item[t] else np.zeros(D) for t in range(TILE)])
            kept = []
            for l, d in enumerate(dil):
                ypad = np.concatenate([np.zeros((8, D)), y])                     # the zero front rows
                c = n[f"blocks.{l}.conv.bias"] + sum(ypad[8 - (2 - j) * d:8 - (2 - j) * d + TILE] @ W[l][:, :, j].T for j in range(3))
                mean = c.mean(1, keepdims=True)
                rstd = 1 / np.sqrt(((c - mean) ** 2).mean(1, keepdims=True) + 1e-5)
                nh = (c - mean) * rstd
                nn_ = nh * n[f"blocks.{l}.ln.weight"] + n[f"blocks.{l}.ln.bias"]
                kept.append((ypad, nh, rstd, nn_))
                y = np.where(item[:, None], y + np.maximum(nn_, 0), 0.0)
            dy = np.zeros((TILE, D))
            if p >= 1:
                dy[TILE - 1] = dH[b, p]
            for l in reversed(range(nb)):
                d = dil[l]
                ypad, nh, rstd, nn_ = kept[l]
                dn = dy * (nn_ > 0)
                g[f"blocks.{l}.ln.weight"] += (dn * nh).sum(0); g[f"blocks.{l}.ln.bias"] += dn.sum(0)
                a = dn * n[f"blocks.{l}.ln.weight"]
                dc = rstd * (a - a.mean(1, keepdims=True) - nh * (a * nh).mean(1, keepdims=True))
                g[f"blocks.{l}.conv.bias"] += dc.sum(0)
                dcpad = np.concatenate([dc, np.zeros((8, D))])                    # the zero back rows
                for j in range(3):
                    s = (2 - j) * d
                    g[f"blocks.{l}.conv.weight"][:, :, j] += dc.T @ ypad[8 - s:8 - s + TILE]
                    dy = dy + dcpad[s:s + TILE] @ W[l][:, :, j]
                dy = np.where(item[:, None], dy, 0.0)
            dwin[p] = dy
        for p in range(lens[b]):
            dX[b, 0] += dH[b, p]
        for k in range(1, lens[b]):
            for p in range(k, min(lens[b] - 1, k + R - 1) + 1):
                dX[b, k] += dwin[p, k - p + TILE - 1]
    return dX, g


@pytest.mark.parametrize("ci", range(len(nextitnetcase.CASES)), ids=nextitnetcase.IDS)
def test_closed_form_cone_backward_equals_autograd(ci):
    U, I, B, T, dil, S, hot = nextitnetcase.CASES[ci]
    p, X, lens, rng = _case(ci)
    G = rng.normal(size=(T + 1, B, S))
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    X = X.detach().clone().requires_grad_(True)
    up = nextitnet_host.upstream(G, lens, B, T + 1, torch.float64)
    (nextitnet_host.states_from_slots(p, X, dil) * up).sum().backward()
    n = {k: v.detach().numpy() for k, v in p.items()}
    dH = up.numpy() @ n["decoder.weight"]                # [B, T+1, D]; rows p >= len are zero
    dX, g = _cone_backward(n, X.detach().numpy(), lens, dH, dil)

    def close(got, want, what):
        scale = np.abs(want).max()
        np.testing.assert_allclose(got / scale, want / scale, rtol=0, atol=1e-12, err_msg=what)
    close(dX, X.grad.numpy(), "dX")
    for k, v in g.items():
        close(v, p[k].grad.numpy(), k)


def _report(what, margins):
    for blk, (margin, err32) in margins.items():
        print(f"near-tie {what} {blk}: min |n| {margin:.3e}  float32 restatement error {err32:.3e}  ratio {margin / max(err32, 1e-300):.1f}")
        assert margin >= nextitnetcase.FACTOR * err32, (what, blk)


@pytest.mark.parametrize("ci", range(len(nextitnetcase.CASES)), ids=nextitnetcase.IDS)
def test_no_case_sits_near_a_relu_kink(ci):
    """The condition under which a float32 forward takes the branches float64 takes: every LayerNorm output a ReLU reads is at least 8 x the
    float32 restatement's own maximum error on it away from zero (the factor and its reason: DESIGN.md 7.5).  The recorded ratio of the chosen
    seed is the one measured here."""
    U, I, B, T, dil, S, hot = nextitnetcase.CASES[ci]
    users, acts, rews, lens, _ = nextitnetcase.teacher_inputs(U, I, B, T, hot)
    p = nextitnetcase.case_params(ci)
    _report(nextitnetcase.IDS[ci], nextitnetcase.near_tie_margins(p, users, acts, rews, lens, dil))
    ratio = nextitnetcase.near_tie_ratio(p, users, acts, rews, lens, dil)
    assert abs(ratio - nextitnetcase.RATIOS[ci]) <= 0.05 * nextitnetcase.RATIOS[ci] + 0.1, (ratio, nextitnetcase.RATIOS[ci])


@pytest.mark.parametrize("what,model,seed,U,I,B", [("rollout B=6", SLOT.rollout_model, SLOT.rollout_seed, 200, 300, 6),
                                                   ("rollout B=70", SLOT.rollout_model, SLOT.rollout_seed, 200, 300, 70),
                                                   ("plugin", SLOT.plugin_model, SLOT.plugin_seed, 100, 300, 16)])
def test_the_rollout_and_plugin_parameters_keep_clear_of_the_kinks(what, model, seed, U, I, B):
    """The rollout and plugin tests' parameters on full-length teacher-forced histories at those tests' sizes (their own actions are the
    device policy's; the plugin test repeats the check on them)."""
    T, S = 8, 20
    users, acts, rews, _, _ = nextitnetcase.teacher_inputs(U, I, B, T)
    _report(what, nextitnetcase.near_tie_margins(SLOT.param_dict(U, I, seed, S, model), users, acts, rews, np.full(B, T + 1), model))


def test_check_shape_refusals_name_their_member():
    check_nextitnet_shape(32, 20, (1, 2, 4), 3, 101)
    check_nextitnet_shape(32, 32, (1, 2, 1, 2))
    check_nextitnet_shape(32, 1, (4, 3))
    for kw, word in [(dict(dim_model=16), "dim_model"), (dict(dim_state=0), "dim_state"), (dict(dim_state=33), "dim_state"),
                     (dict(dilations=()), "n_blocks"), (dict(dilations=(1, 1, 1, 1, 1)), "n_blocks"), (dict(dilations=(0, 1)), "dilations"),
                     (dict(dilations=(1, 5)), "dilations"), (dict(dilations=(4, 4)), "dilations"), (dict(dilations=(2, 2, 2, 2)), "sum"),
                     (dict(kernel_size=2), "kernel_size"), (dict(max_len=4097), "max_len"), (dict(max_len=0), "max_len")]:
        args = dict(dim_model=32, dim_state=20, dilations=(1, 2, 4), kernel_size=3, max_len=101)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            check_nextitnet_shape(**args)


def test_param_names_order_shapes_and_init():
    sh = nextitnet_param_shapes(11, 13, 32, 20, (1, 2))
    assert list(sh.items()) == [
        ("embedding_dict.feat_user.weight", (11, 32)), ("embedding_dict.feat_item.weight", (13, 32)), ("ffn_user.weight", (32, 32)),
        ("ffn_user.bias", (32,)), ("fnn_gate.weight", (32, 33)), ("fnn_gate.bias", (32,)),
        ("blocks.0.conv.weight", (32, 32, 3)), ("blocks.0.conv.bias", (32,)), ("blocks.0.ln.weight", (32,)), ("blocks.0.ln.bias", (32,)),
        ("blocks.1.conv.weight", (32, 32, 3)), ("blocks.1.conv.bias", (32,)), ("blocks.1.ln.weight", (32,)), ("blocks.1.ln.bias", (32,)),
        ("decoder.weight", (20, 32)), ("decoder.bias", (20,))]
    assert len(nextitnet_param_shapes(11, 13, 32, 7, (1, 2, 1, 2))) == 8 + 4 * 4
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    p = init_nextitnet_tracker_params(11, 13, seed=5, dilations=(1, 2))
    assert torch.equal(torch.random.get_rng_state(), before)
    assert {k: tuple(v.shape) for k, v in p.items()} == sh and list(p) == list(sh)
    # the shared tensors are drawn as init_tracker_params draws them, whatever the blocks
    from cirs_hip.engine import init_tracker_params
    ref = init_tracker_params(11, 13, 5, seed=5)
    q = init_nextitnet_tracker_params(11, 13, seed=5, dilations=(4, 1, 2))
    n_shared = 0
    for k in p:
        if k in ref:
            assert torch.equal(p[k], ref[k]) and torch.equal(q[k], ref[k]), k
            n_shared += 1
        else:
            assert torch.isfinite(p[k]).all(), k
            if k.endswith("ln.bias"):
                assert (p[k] == 0).all(), k          # torch's default LayerNorm: weight 1, bias 0
            elif k.endswith("ln.weight"):
                assert (p[k] == 1).all(), k
            else:
                assert p[k].abs().max() > 0, k
    assert n_shared == 8
    assert torch.equal(init_nextitnet_tracker_params(11, 13, seed=5, dilations=(1, 2))["blocks.1.conv.weight"], p["blocks.1.conv.weight"])
    assert not torch.equal(init_nextitnet_tracker_params(11, 13, seed=6, dilations=(1, 2))["blocks.1.conv.weight"], p["blocks.1.conv.weight"])
    # the init's block tensors load by name into the torch modules
    blocks = _modules(p, (1, 2))
    for k, v in blocks.state_dict().items():
        assert torch.equal(v, p["blocks." + k]), k
    c = nextitnetcase.nextitnet_param_dict(11, 13, 1, (1, 2))
    assert list(c) == list(sh) and {k: tuple(v.shape) for k, v in c.items()} == sh
    b = torch.cat([c[k].reshape(-1) for k in c if k.startswith("blocks.") and k.endswith(".bias")])
    assert (b > 0).any() and (b < 0).any() and (b.abs() >= 0.05).all() and (b.abs() <= 0.15).all()
    assert abs(float(c["blocks.0.ln.weight"].mean()) - 1.0) < 0.1


def test_slot_record():
    assert (SLOT.name, SLOT.display, SLOT.entry) == ("nextitnet", "NextItNet", "cirs_nextitnet_tracker")
    assert SLOT.n_grad_tensors((1, 2, 4)) == 20 and SLOT.flags((1, 2, 4)) == ["--dilations", "1,2,4"] and SLOT.plugin_kw((1, 2)) == {"dilations": (1, 2)}
    assert SLOT.split(SLOT.CASES[2]) == ((120, 200, 33, 20, 20, 0.0), (1, 2, 1, 2))
    assert len(SLOT.CASES) == len(SLOT.IDS) == len(nextitnetcase.SEEDS) == len(nextitnetcase.RATIOS) == 6


def _columns(U=11, I=13):
    return [types.SimpleNamespace(vocabulary_size=U)], [types.SimpleNamespace(vocabulary_size=I)], []


def test_state_tracker_nextitnet_refuses_what_is_not_built(monkeypatch):
    from core import state_tracker
    from core.state_tracker import StateTrackerNextItNet, _RecurrentStateTracker

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(state_tracker, "flat_tracker_params", no_device)
    assert issubclass(StateTrackerNextItNet, _RecurrentStateTracker)      # what Collector(dropout_redraw=True) refuses
    uc, ac, fc = _columns()
    kw = dict(dim_model=32, dim_state=20, dim_max_batch=4)
    for bad in ((0, 1), (1, 5), (4, 4), (2, 2, 2, 2)):
        with pytest.raises(ValueError, match="dilations"):
            StateTrackerNextItNet(uc, ac, fc, dilations=bad, **kw)
    for bad in ((), (1, 1, 1, 1, 1)):
        with pytest.raises(ValueError, match="n_blocks"):
            StateTrackerNextItNet(uc, ac, fc, dilations=bad, **kw)
    with pytest.raises(ValueError, match="kernel_size"):
        StateTrackerNextItNet(uc, ac, fc, kernel_size=5, **kw)
    with pytest.raises(ValueError, match="dim_model"):
        StateTrackerNextItNet(uc, ac, fc, dim_model=16, dim_state=20, dim_max_batch=4)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="dim_state"):
            StateTrackerNextItNet(uc, ac, fc, dim_model=32, dim_state=bad, dim_max_batch=4)
    with pytest.raises(ValueError, match="max_len"):
        StateTrackerNextItNet(uc, ac, fc, MAX_TURN=4096, **kw)
    with pytest.raises(NotImplementedError, match="VirtualTB"):
        StateTrackerNextItNet(uc, ac, fc, dataset="VirtualTB-v0", **kw)
    with pytest.raises(TypeError):
        StateTrackerNextItNet(uc, ac, fc, window_size=4, **kw)


def test_plugin_class_keywords_and_attributes_without_a_device(monkeypatch):
    from core.state_tracker import StateTrackerNextItNet
    monkeypatch.setattr(StateTrackerNextItNet, "_setup", lambda self, shapes, init, seed: None)      # no device: the flat buffer is not built
    uc, ac, fc = _columns()
    st = StateTrackerNextItNet(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dropout=0.1, nhead=4, d_hid=64, nlayers=3)
    assert st.training      # dropout is accepted and unused: the model has no dropout site
    assert st.dilations == (1, 2, 4) and st.kernel_size == 3 and st.dropout_p == 0.0 and st.nlayers == 0 and st.CELL == "NextItNet"
    assert st._model_kw() == {"dilations": (1, 2, 4)} and st._engine_kw()["dilations"] == (1, 2, 4)
    st.eval(); st.train()
    st = StateTrackerNextItNet(uc, ac, fc, dim_model=32, dim_state=20, dim_max_batch=4, dilations=[1, 2, 1, 2])
    assert st.dilations == (1, 2, 1, 2) and all(isinstance(d, int) for d in st.dilations)


def test_library_refuses_the_same_cfgs_without_a_gpu():
    from cirs_hip import abi
    lib = abi.lib()

    def cfg_of(ds=(1, 2, 4), **kw):
        base = dict(n_users=3, n_items=4, dim_model=32, dim_state=20, n_blocks=len(ds), max_len=5, n_env=2)
        base.update(kw)
        return abi.NextItNetCfg(dilations=(C.c_int32 * 4)(*(tuple(ds)[:4] + (0,) * (4 - len(ds)))), **base)

    def refused(cfg, word):
        calls = [lambda: lib.cirs_nextitnet_tracker_step(C.byref(cfg), None, None, None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_nextitnet_tracker_init(C.byref(cfg), None, None, None, None, 2, None, 20, None),
                 lambda: lib.cirs_nextitnet_tracker_backward(C.byref(cfg), None, None, None, None, None, None, None, None, None, 4, None, None, None, 0,
                                                             None)]
        for call in calls:
            assert call() != 0
            assert word in lib.cirs_last_error(), (word, lib.cirs_last_error())
            assert b"nextitnet tracker" in lib.cirs_last_error()
        if word != b"weights null":
            assert lib.cirs_nextitnet_tracker_backward_workspace_bytes(C.byref(cfg), 7) == 0
    refused(cfg_of(()), b"n_blocks")
    refused(cfg_of(n_blocks=5), b"n_blocks")
    refused(cfg_of((0, 1)), b"dilations")
    refused(cfg_of((1, 5)), b"dilations")
    refused(cfg_of((4, 4)), b"dilations")
    refused(cfg_of((2, 2, 2, 2)), b"dilations")
    refused(cfg_of(dim_model=16), b"dim_model")
    refused(cfg_of(dim_state=0), b"dim_state")
    refused(cfg_of(dim_state=33), b"dim_state")
    refused(cfg_of(max_len=4097), b"max_len")
    for good in (cfg_of(), cfg_of((1, 2, 1, 2)), cfg_of((4, 3)), cfg_of((1,))):
        refused(good, b"weights null")
        assert lib.cirs_nextitnet_tracker_backward_workspace_bytes(C.byref(good), 0) == 0
        assert lib.cirs_nextitnet_tracker_backward_workspace_bytes(C.byref(good), 7) > 0
    assert C.sizeof(abi.NextItNetCfg) == 11 * 4 and C.sizeof(abi.NextItNetWeights) == 24 * 8 and C.sizeof(abi.NextItNetState) == 2 * 8
