"""CPU: the gradient / Adam comparators of tests/gradcase.py -- the fp32-against-float64 ratios of the host restatement behind B and B_ROW,
the subtle errors the comparators must reject, and the float64 Adam recurrence against torch.optim.Adam."""
import numpy as np
import pytest
import torch

import gradcase as G


def _f32(g64):
    return {k: np.asarray(v, np.float64).astype(np.float32) for k, v in g64.items()}


_refs = {}


def _ref(name, b=0):
    """(float64 gradient, touched map) of batch b of a case at its initial weights; computed once, never modified."""
    if (name, b) not in _refs:
        c = G.build(name)
        _refs[(name, b)] = (G.reference(c, c["init"], c["batches"][b])[1], G.touched(c["spec"], c["batches"][b][0]))
    return _refs[(name, b)]


def _data_grad(c, rows, p=None):
    """float64 data gradient (no regulariser) of the samples `rows` of batch 0 as their share of the batch mean."""
    x, y, s = c["batches"][0]
    hyper = dict(c["hyper"], l2_embedding=0.0, l2_linear=0.0, l2_all=0.0)
    _, g = G.host_module(c["spec"]).loss_and_grad(c["init"] if p is None else p, x[rows], y[rows], s[rows], **hyper, dtype=torch.float64)
    return {k: v.numpy() * (len(x[rows]) / len(x)) for k, v in g.items()}


def test_measured_ratios_stay_within_a_quarter_of_the_bars():
    print(f"B = {G.B:.3e}, B_ROW = {G.B_ROW:.3e}")
    print(f"#   {'case':<28s} {'r_T':>9s} {'r_row':>9s}")
    worst_t = worst_row = 0.0
    for name in G.CASES:
        c = G.build(name)
        host = G.host_module(c["spec"])
        r_t = r_row = 0.0
        for b, batch in enumerate(c["batches"]):
            g64, tmap = _ref(name, b)
            _, g32 = host.loss_and_grad(c["init"], *batch, **c["hyper"], dtype=torch.float32)
            r = G.grad_ratios({k: v.numpy() for k, v in g32.items()}, g64, tmap, b=G.B)
            r_t = max(r_t, max(v[0] for v in r.values()))
            r_row = max(r_row, max(v[1] for v in r.values() if v[1] is not None))
        print(f"#   {name:<28s} {r_t:9.2e} {r_row:9.2e}")
        worst_t, worst_row = max(worst_t, r_t), max(worst_row, r_row)
    print(f"largest r_T {worst_t:.3e} (B / 8 = {G.B / 8:.3e}), largest r_row {worst_row:.3e} (B_ROW / 8 = {G.B_ROW / 8:.3e})")
    assert worst_t <= G.B / 4 and worst_row <= G.B_ROW / 4


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_inputs_are_in_range(name):
    c = G.build(name)
    spec, host = c["spec"], G.host_module(c["spec"])
    p = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in c["init"].items()}
    for x, y, s in c["batches"]:
        xt = torch.as_tensor(x, dtype=torch.float64)
        if spec["trainer"] == "deepfm":
            ids, hi = x[:, [0, 1, 7, 8]], [spec["U"], spec["I"], spec["U"], spec["I"]]
            feats = x[:, [2, 3, 4, 5, 9, 10, 11, 12]]
            diffs = [host.pair_forward(p, xt[:, :7]) - host.pair_forward(p, xt[:, 7:])]
        else:
            ids, hi = x[:, [0, 1, 2, 3, 9, 10]], [spec["U"]] * 2 + [spec["I"]] * 4
            feats = x[:, [4, 5, 6, 7, 11, 12, 13, 14]]
            yp, yn = host.main_forward(p, xt[:, :9]), host.main_forward(p, torch.cat([xt[:, :2], xt[:, 9:]], dim=1))
            diffs = [yp - yn, host.ui_forward(p, xt[:, 0], xt[:, 2], "int") - host.ui_forward(p, xt[:, 0], xt[:, 9], "int"),
                     host.ui_forward(p, xt[:, 1], xt[:, 3], "con") - host.ui_forward(p, xt[:, 1], xt[:, 10], "con")]
        assert (ids >= 0).all() and (ids < np.array(hi)[None, :]).all() and (feats >= 0).all() and (feats < spec["F"]).all()
        assert max(float(d.abs().max()) for d in diffs) < 30, "the saturated BPR regime is out of scope"
        assert 0 <= y.min() and y.max() <= 5
    if spec["special"] == "segments":
        x = c["batches"][0][0]
        fp, fn = (x[:, 2:6], x[:, 9:13]) if spec["trainer"] == "deepfm" else (x[:, 4:8], x[:, 11:15])
        assert len(np.unique(x[:, 0])) == 1                                    # one segment of every user row
        assert 4 * ((fp == 0).all(1).sum() + (fn == 0).all(1).sum()) > 1000    # key 0 of the feature scatter
        for xb in (b[0] for b in c["batches"]):
            cols = [1, 8] if spec["trainer"] == "deepfm" else [2, 9]
            assert 0 in xb[:, cols] and spec["I"] - 1 in xb[:, cols]
        assert 0 in c["batches"][1][0][:, 0] and spec["U"] - 1 in c["batches"][1][0][:, 0]
    if spec["trainer"] == "dice" and spec["n"] > 3:
        assert (c["batches"][1][2] == 1).all() and all((b[2] > 0).any() and (b[2] < 0).any() for b in c["batches"][::2])


def test_the_float64_gradient_rounded_to_fp32_passes():
    for name in ("deepfm-pairwise-ab-slabcap", "deepfm-pd-segments", "dice-segments", "dice-E8"):
        c = G.build(name)
        g64, tmap = _ref(name)
        used = G.check_grads(_f32(g64), g64, tmap, what=name)
        assert max(used) < 0.05
        G.check_exact(_f32(g64), c["init"], tmap, G.L2, what=name)


def _rejected(g, g64, tmap):
    with pytest.raises(AssertionError):
        G.check_grads(g, g64, tmap, what="mutated")


def test_rejects_one_tensor_scaled():
    for name, tensor in (("deepfm-pairwise-ab", "dnn.linears.1.weight"), ("deepfm-ips", "linear.embedding_dict.photo_id.weight"),
                         ("dice-E16", "embedding_dict.photo_con.weight"), ("dice-E8", "last_ui.weight")):
        g64, tmap = _ref(name)
        g = _f32(g64)
        g[tensor] = (g[tensor] * np.float32(1.001)).astype(np.float32)
        _rejected(g, g64, tmap)


def test_rejects_one_sample_missing_from_a_dense_weight_at_8200_rows():
    """Samples with a gradient of ordinary size: each is 0.6e-4 .. 2e-4 of the tensor's largest entry (1 / 8200 = 1.2e-4).  A sample the
    model already fits, whose own gradient is a tenth of that (the batch's last one: 7e-6), lies inside the fp32 rounding of the
    reference's own sums, where no bar can see it."""
    c = G.build("deepfm-pairwise-ab-slabcap")
    g64, tmap = _ref("deepfm-pairwise-ab-slabcap")
    for j in (0, 1, 4099):
        one = _data_grad(c, [j])
        for tensor in ("dnn.linears.0.weight", "dnn.linears.1.weight", "last.weight"):
            g = _f32(g64)
            g[tensor] = (g64[tensor] - one[tensor]).astype(np.float32)
            _rejected(g, g64, tmap)


def test_rejects_one_sample_missing_from_a_table_row_touched_twice():
    for name, tensor, col in (("deepfm-pairwise-ab", "embedding_dict.photo_id.weight", [1, 8]), ("dice-E8", "embedding_dict.photo_int.weight", [2, 9]),
                              ("deepfm-pairwise-ab-slabcap", "embedding_dict.feat.weight", None)):
        c = G.build(name)
        x = c["batches"][0][0]
        g64, tmap = _ref(name)
        if col is None:       # the rarest feature id of the large batch: a rarely touched row beside hot ones
            cols = [2, 3, 4, 5, 9, 10, 11, 12]
            ids, cnt = np.unique(x[:, cols][x[:, cols] > 0], return_counts=True)
            row = int(ids[np.argmin(cnt)])
            j = int(np.flatnonzero((x[:, cols] == row).any(1))[0])
        else:
            ids, cnt = np.unique(x[:, col], return_counts=True)
            row = int(ids[cnt == 2][0])
            j = int(np.flatnonzero((x[:, col] == row).any(1))[0])
        one = _data_grad(c, [j])
        assert np.abs(one[tensor][row]).max() > 0
        g = _f32(g64)
        g[tensor][row] = (g64[tensor][row] - one[tensor][row]).astype(np.float32)
        _rejected(g, g64, tmap)


def test_rejects_a_segment_cut_after_32_contributions():
    for name, tensor in (("deepfm-pd-segments", "embedding_dict.user_id.weight"), ("dice-segments", "embedding_dict.user_int.weight"),
                         ("deepfm-pd-segments", "linear.embedding_dict.user_id.weight")):
        c = G.build(name)
        g64, tmap = _ref(name)
        n = c["spec"]["n"]
        rest = _data_grad(c, np.arange(32, n))           # everything the one user's row receives from the samples past the 32nd
        g = _f32(g64)
        g[tensor][3] = (g64[tensor][3] - rest[tensor][3]).astype(np.float32)
        _rejected(g, g64, tmap)


def test_rejects_the_last_row_slab_missing_from_the_first_dnn_weight():
    from cirs_hip import deepfm_host
    c = G.build("deepfm-pairwise-ab-slabcap")
    g64, tmap = _ref("deepfm-pairwise-ab-slabcap")
    x, y, s = (torch.as_tensor(z, dtype=torch.float64) for z in c["batches"][0])
    n = len(x)
    rows = np.arange(n - 80, n)          # 2n = 16400 pair rows in 256 slabs of 80: the last slab that holds rows is the last 80 negative rows
    p = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in c["init"].items()}
    w1 = p["dnn.linears.0.weight"].clone().requires_grad_(True)
    yp = deepfm_host.pair_forward(p, x[rows, :7])
    yn = deepfm_host.pair_forward(dict(p, **{"dnn.linears.0.weight": w1}), x[rows, 7:])          # the path through the negative rows alone
    alpha = p["ab_embedding_dict.alpha_u.weight"][x[rows, 0].long(), 0]
    beta = p["ab_embedding_dict.beta_i.weight"][x[rows, 1].long(), 0]
    loss_y, bpr, _ = deepfm_host.loss_terms("pairwise", y[rows], yp, yn, s[rows], alpha, beta)
    slab = torch.autograd.grad(loss_y + bpr, w1)[0].numpy() * (len(rows) / n)
    assert np.abs(slab).max() > 0
    g = _f32(g64)
    g["dnn.linears.0.weight"] = (g64["dnn.linears.0.weight"] - slab).astype(np.float32)
    _rejected(g, g64, tmap)


def test_rejects_a_data_gradient_on_the_padding_row():
    for name in ("deepfm-ips", "dice-E8", "deepfm-pairwise-ab-slabcap"):
        c = G.build(name)
        g64, tmap = _ref(name)
        feat = "embedding_dict.feat.weight"
        row = int(np.flatnonzero(tmap[feat])[0])
        c2 = 2 * (G.L2["l2_all"] + G.L2["l2_embedding"])
        data = g64[feat][row] - c2 * c["init"][feat][row].astype(np.float64)       # what a touched row receives
        assert np.abs(data).max() > 0
        g = _f32(g64)
        g[feat][0] = (g64[feat][0] + data).astype(np.float32)
        with pytest.raises(AssertionError):
            G.check_exact(g, c["init"], tmap, G.L2, what="mutated")
        g[feat][0] = (g64[feat][0] + 1e-3 * data).astype(np.float32)
        with pytest.raises(AssertionError):
            G.check_exact(g, c["init"], tmap, G.L2, what="mutated")


def test_exact_zero_check_rejects_noise_and_stale_rows():
    c = G.build("dice-E8")
    g64, tmap = _ref("dice-E8")
    g = _f32(g64)
    G.check_exact(g, c["init"], tmap, G.L2)
    for sign in (1.0, -1.0):
        g = _f32(g64)
        g["out_ui.bias"] = (g["out_ui.bias"].astype(np.float64) + sign * 1e-9).astype(np.float32)
        with pytest.raises(AssertionError):
            G.check_exact(g, c["init"], tmap, G.L2, what="mutated")
    # a row the previous batch touched and this one does not, left uncleared
    _, tmap1 = _ref("dice-E8", 1)
    tensor = "embedding_dict.photo_int.weight"
    stale = int(np.flatnonzero(tmap1[tensor] & ~tmap[tensor])[0])
    g = _f32(g64)
    g[tensor][stale] += np.float32(1e-6)
    with pytest.raises(AssertionError):
        G.check_exact(g, c["init"], tmap, G.L2, what="mutated")
    g = _f32(g64)
    g["linear_model.embedding_dict.feat.weight"][5] *= np.float32(1.00001)
    with pytest.raises(AssertionError):
        G.check_exact(g, c["init"], tmap, G.L2, what="mutated")


def test_adam_recurrence_reproduces_torch_adam():
    rng = np.random.RandomState(5)
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    p = torch.tensor(rng.normal(0, 0.3, 500), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    q, m, v = p.detach().numpy().copy(), np.zeros(500), np.zeros(500)
    for t in range(1, 4):
        g = rng.normal(0, 1, 500) * 10.0 ** rng.uniform(-6, 1, 500)
        p.grad = torch.tensor(g)
        opt.step()
        b1, b2, e, step_size, bc2s = G.adam_constants(t, lr, betas, eps, as_device=False)
        m, v = G.adam_moments(m, v, g, b1, b2)
        q, _ = G.adam_update(q, m, v, step_size, bc2s, e)
        st = opt.state[p]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(q, p.detach().numpy(), rtol=1e-12, atol=1e-15)
    # t = 10000 with preset moments
    st = opt.state[p]
    m, v = rng.normal(0, 0.1, 500), rng.uniform(1e-6, 1, 500)
    st["exp_avg"].copy_(torch.tensor(m)); st["exp_avg_sq"].copy_(torch.tensor(v))
    if torch.is_tensor(st["step"]):
        st["step"].fill_(9999)
    else:
        st["step"] = 9999
    g = rng.normal(0, 1, 500)
    q = p.detach().numpy().copy()
    p.grad = torch.tensor(g)
    opt.step()
    b1, b2, e, step_size, bc2s = G.adam_constants(10000, lr, betas, eps, as_device=False)
    m, v = G.adam_moments(m, v, g, b1, b2)
    q, _ = G.adam_update(q, m, v, step_size, bc2s, e)
    np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(q, p.detach().numpy(), rtol=1e-12, atol=1e-15)
    # the device's constants differ from these only by their fp32 rounding
    d = G.adam_constants(10000, lr, betas, eps)
    np.testing.assert_allclose(d, (b1, b2, e, step_size, bc2s), rtol=2.0 ** -23)


def test_adam_check_rejects_a_wrong_bias_correction_and_a_fused_rounding():
    rng = np.random.RandomState(6)
    f = np.float32
    p0, m0, v0 = f(rng.normal(0, 0.3, 4000)), f(rng.normal(0, 0.01, 4000)), f(rng.uniform(1e-8, 1e-3, 4000))
    g = f(rng.normal(0, 0.05, 4000))
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8

    def device_like(t, t_used=None):
        b1, b2, e, step_size, bc2s = (f(z) for z in G.adam_constants(t if t_used is None else t_used, lr, betas, eps))
        m1 = m0 + (f(1) - b1) * (g - m0)
        v1 = v0 * b2 + (f(1) - b2) * g * g
        return m1, v1, p0 - step_size * (m1 / (np.sqrt(v1) / bc2s + e))
    d = np.float64
    for t in (1, 3, 10000):
        m1, v1, p1 = device_like(t)
        used = G.check_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), m1.astype(d), v1.astype(d), p1.astype(d), t, lr, betas, eps)
        assert max(used) <= 1.0
    m1, v1, p1 = device_like(3, t_used=4)          # the step count off by one
    with pytest.raises(AssertionError):
        G.check_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), m1.astype(d), v1.astype(d), p1.astype(d), 3, lr, betas, eps)
    m1, v1, p1 = device_like(3)
    with pytest.raises(AssertionError):            # beta1 = 0.9 as a double instead of the fp32 value is visible in m
        G.check_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), (m1 * f(1.000002)).astype(d), v1.astype(d), p1.astype(d), 3, lr, betas, eps)
