"""CPU: the gradient / Adam comparators of tests/vtbgradcase.py for the two VirtualTaobao trainers -- the fp32-against-float64 figures of
the host restatement behind B and Z_MARGIN, the share of rows the kink guard passes over when the fp32 torch chain stands in for the
device, the case inputs, and the subtle errors the comparators must reject (each built from float64 pieces; the unmutated gradient
passes the comparator the mutation is fed to).

Two mutations lie below what any bar can see: an Adam step count off by one at t = 10000, where the bias corrections of t and t + 1
differ by less than an fp32 rounding (it is rejected at t = 1 and t = 3), and the first row of slab 1 missing from the 129-row MLP
case, a row the model already fits (it is rejected in the 129-row MMoE case; see the test).  The tests of single missing rows print how
many B the row is worth."""
import numpy as np
import pytest
import torch

import vtbgradcase as V
from cirs_hip import mmoe_host


def _f32(g64):
    return {k: np.asarray(v, np.float64).astype(np.float32) for k, v in g64.items()}


_refs = {}


def _ref(name):
    """(batch, float64 gradient, no-data-gradient map) of the first guarded batch of a case at its initial weights; computed once, never
    modified."""
    if name not in _refs:
        c = V.build(name)
        batch, _, _ = V.take_batch(c, 0, c["init"], V.SKIP_SHARE_HOST, what=name)
        _refs[name] = (batch, V.reference(c, c["init"], batch)[1], V.no_data_grad(c["spec"], batch[0]))
    return _refs[name]


def _data_grad(c, batch, rows):
    """float64 data gradient (no regulariser) of the samples `rows` of `batch` as their share of the batch mean."""
    sub = tuple(col[rows] for col in batch)
    _, g = V.reference(c, c["init"], sub, l2_linear=0.0, l2_all=0.0)
    return {k: v * (len(sub[0]) / len(batch[0])) for k, v in g.items()}


_measured = {}


def _measure(name):
    """(largest r_T, its tensor, largest |z32 - z64|, rows passed over, rows consumed, largest share per step) of a case's host replay."""
    if name not in _measured:
        c = V.build(name)
        r_t, r_name, skipped, consumed, share = 0.0, "", 0, 0, 0.0

        def dz_of(p, x):
            z32, z64 = (mmoe_host.hidden_preactivations(p, x, dt) for dt in (torch.float32, torch.float64))
            return max(float((a.double() - b).abs().max()) for a, b in zip(z32, z64))
        dz = dz_of(c["init"], c["pool"][0])
        for st, p, batch, sk, con in V.host_replay(c):
            _, g64 = V.reference(c, p, batch)
            _, g32 = V.reference(c, p, batch, dtype=torch.float32)
            r = V.grad_ratios(g32, g64, V.no_data_grad(c["spec"], batch[0]))
            worst = max(r, key=r.get)
            if r[worst] > r_t:
                r_t, r_name = r[worst], worst
            dz = max(dz, dz_of(p, batch[0]))
            skipped, consumed, share = skipped + sk, consumed + con, max(share, sk / con)
        _measured[name] = (r_t, r_name, dz, skipped, consumed, share)
    return _measured[name]


def test_measured_figures_stay_within_a_quarter_of_the_bars_and_the_guard_passes_over_few_rows():
    print(f"B = {V.B:.3e}, Z_MARGIN = {V.Z_MARGIN:.3e}")
    print(f"#   {'case':<22s} {'r_T':>9s}  {'on':<38s} {'dz':>9s}  passed over")
    worst_r = worst_dz = 0.0
    for name in V.CASES:
        r_t, r_name, dz, skipped, consumed, share = _measure(name)
        print(f"#   {name:<22s} {r_t:9.2e}  {r_name:<38s} {dz:9.2e}  {skipped} of {consumed}")
        worst_r, worst_dz = max(worst_r, r_t), max(worst_dz, dz)
        assert share <= V.SKIP_SHARE_HOST            # host_replay asserts it per step already
        assert dz <= V.margin_of(V.CASES[name]) / 4
    print(f"largest r_T {worst_r:.3e} (B / 8 = {V.B / 8:.3e}), largest dz {worst_dz:.3e} (Z_MARGIN / 16 = {V.Z_MARGIN / 16:.3e})")
    assert worst_r <= V.B / 4 and worst_dz <= V.Z_MARGIN / 4


def test_the_guard_refuses_a_pool_that_is_mostly_kinks():
    c = V.build("mlp-96-n17")
    with pytest.raises(AssertionError, match="passed over"):
        V.take_batch(c, 0, c["init"], V.SKIP_SHARE_DEVICE, z_margin=0.01)
    batch, cursor, skipped = V.take_batch(c, 0, c["init"], 1.0, z_margin=1e-3)
    assert cursor == 17 + skipped and len(batch[0]) == 17
    assert (V.min_abs_z(c["init"], batch[0]) >= 1e-3).all()


@pytest.mark.parametrize("name", list(V.CASES))
def test_case_inputs_are_in_range(name):
    c = V.build(name)
    spec, pool = c["spec"], c["pool"]
    x = pool[0]
    assert all(len(col) == V.pool_rows(spec) for col in pool) and all(col.dtype == np.float32 for col in pool)
    assert set(np.unique(x[:, :88])) <= {0.0, 1.0} and 0.05 < x[:, :88].mean() < 0.25
    assert x[:, 88:90].min() >= 0 and x[:, 88:90].max() <= 10 and x[:, 90].min() >= 1 and x[:, 90].max() <= 29
    if spec["kind"] == "mmoe":
        assert x.shape[1] == 118 and np.abs(x[:, 91:]).max() <= 1
        y, e = pool[1], pool[2]
        assert set(np.unique(y)) <= set(range(11)) and e.min() >= 0
        assert [(k, v.shape) for k, v in c["init"].items()] == mmoe_host.shapes(*spec["dnn"])
    else:
        y = pool[1]
        assert x.shape[1] == 91 and y.shape[1] == 28 and np.abs(y[:, :27]).max() <= 1 and set(np.unique(y[:, 27])) <= set(range(11))
        assert (y[:, 27].max() == 0) == spec["no_click"]          # the structure of the case survives the pool
        assert mmoe_host.mlp_shape_of(c["init"]) == (list(spec["dnn"]), spec["experts"], spec["expert_dim"])
    assert all(v.dtype == np.float32 for v in c["init"].values())


def test_the_cases_cover_the_shapes_and_batch_sizes():
    mm = [s for s in V.CASES.values() if s["kind"] == "mmoe"]
    assert {s["dnn"] for s in mm} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert sorted(s["n"] for s in mm) == [1, 3, 5, 16, 17, 129, 1025]
    ml = {(s["dnn"], s["experts"], s["expert_dim"], s["n"], s["no_click"]) for s in V.CASES.values() if s["kind"] == "mlp"}
    assert ml == {((256, 256), 4, 8, 1, False), ((5, 3), 2, 3, 3, False), ((96,), 2, 5, 17, False), ((40, 72, 24), 3, 6, 33, False),
                  ((5, 3, 4), 2, 2, 16, False), ((31, 256, 1), 8, 8, 65, False), ((17, 33), 1, 64, 50, False), ((256,), 64, 1, 129, False),
                  ((96,), 2, 5, 16, True)}
    # the expert | gate block of (5, 3, 4) starts at float offset 27: K = 4 on LoadNT's scalar path
    assert 3 * 5 + 4 * 3 == 27


def test_some_input_column_is_zero_in_the_small_batches():
    """The exact check has something to hold: a Bernoulli(0.15) column without a single 1."""
    for name in ("mmoe-64x128-n3", "mmoe-64x64-n17", "mlp-5x3-n3", "mlp-96-noclick-n16"):
        _, _, nomap = _ref(name)
        assert (~nomap["dnn.linears.0.weight"]).sum() >= 4


def test_the_float64_gradient_rounded_to_fp32_passes():
    for name in V.CASES:
        c = V.build(name)
        _, g64, nomap = _ref(name)
        used = V.check_grads(_f32(g64), g64, what=name)
        exact = V.check_exact(_f32(g64), c["init"], nomap, what=name)
        print(f"{name}: the float64 gradient rounded to fp32 uses {used:.4f} of B and {exact:.3f} of the 2 ulp")
        assert used < 0.01 and exact <= 0.75


def _rejected(g, g64):
    V.check_grads(_f32(g64), g64, what="unmutated")
    with pytest.raises(AssertionError):
        V.check_grads(g, g64, what="mutated")


def _rejected_exact(g, g64, c, nomap):
    V.check_exact(_f32(g64), c["init"], nomap, what="unmutated")
    with pytest.raises(AssertionError):
        V.check_exact(g, c["init"], nomap, what="mutated")


def test_rejects_one_tensor_scaled():
    for name, tensor in (("mmoe-128x128-n129", "dnn.linears.1.weight"), ("mmoe-64x128-n3", "mmoe_layer.gating_networks.0.weight"),
                         ("mmoe-128x64-n1025", "tower_network.0.weight"), ("mlp-40x72x24-n33", "dnn.linears.2.weight"),
                         ("mlp-256-E64-n129", "mmoe_layer.expert_network.weight"), ("mlp-96-n17", "out.0.bias")):
        _, g64, _ = _ref(name)
        g = _f32(g64)
        g[tensor] = (g64[tensor] * 1.001).astype(np.float32)
        _rejected(g, g64)


@pytest.mark.parametrize("name", ["mmoe-128x128-n129", "mlp-256-E64-n129", "mmoe-128x64-n1025"])
def test_rejects_the_last_batch_row_missing_from_the_first_layers_weight(name):
    c = V.build(name)
    batch, g64, _ = _ref(name)
    n = c["spec"]["n"]
    one = _data_grad(c, batch, [n - 1])["dnn.linears.0.weight"]
    print(f"{name}: the last row's share of dnn.linears.0.weight is {np.abs(one).max() / np.abs(g64['dnn.linears.0.weight']).max() / V.B:.1f} B")
    g = _f32(g64)
    g["dnn.linears.0.weight"] = (g64["dnn.linears.0.weight"] - one).astype(np.float32)
    _rejected(g, g64)


def test_rejects_the_first_row_of_slab_1_and_a_whole_slab_missing():
    """129 rows: rps = 34, so slab 1 is rows 34 .. 67 and the last slab rows 102 .. 128.  The single row is taken out of the MMoE case
    alone: row 34 of the MLP case has no click and a click prediction that is nearly right, its whole gradient is 0 .. 2.4 B of a
    tensor's largest entry, which no bar can see reliably (the case's last row, 26 .. 118 B, is rejected above)."""
    for name in ("mmoe-128x128-n129", "mlp-256-E64-n129"):
        c = V.build(name)
        batch, g64, _ = _ref(name)
        n = c["spec"]["n"]
        rps = (((n + 3) // 4) + 1) & ~1
        assert rps == 34
        for rows in ([rps], np.arange(rps, 2 * rps), np.arange(3 * rps, n))[c["spec"]["kind"] == "mlp":]:
            part = _data_grad(c, batch, rows)
            for tensor in [k for k in g64 if k.endswith(".weight") and k != "linear_model.weight"]:
                share = np.abs(part[tensor]).max() / np.abs(g64[tensor]).max() / V.B
                if len(rows) == 1:
                    print(f"{name}: row {rows[0]} is {share:.1f} B of {tensor}")
                assert share > 1.5
                g = _f32(g64)
                g[tensor] = (g64[tensor] - part[tensor]).astype(np.float32)
                _rejected(g, g64)


def test_rejects_the_first_layers_weight_read_untransposed_from_its_transposed_slot():
    """The slot holds W^T [K, H] row by row; read as [H, K] without undoing the transpose, the element count is kept and every entry
    lands elsewhere."""
    for name in ("mmoe-64x64-n17", "mlp-96-n17", "mlp-5x3-n3"):
        _, g64, _ = _ref(name)
        w = g64["dnn.linears.0.weight"]
        g = _f32(g64)
        g["dnn.linears.0.weight"] = np.ascontiguousarray(w.T).reshape(w.shape).astype(np.float32)
        assert g["dnn.linears.0.weight"].size == w.size
        _rejected(g, g64)


def test_rejects_a_bias_gradient_counted_twice():
    for name, tensor in (("mmoe-128x128-n16", "dnn.linears.0.bias"), ("mmoe-64x64-n1", "out.0.bias"), ("mlp-40x72x24-n33", "dnn.linears.2.bias"),
                         ("mlp-31x256x1-n65", "mmoe_layer.expert_network.bias"), ("mlp-17x33-E1-n50", "out.1.bias")):
        c = V.build(name)
        _, g64, _ = _ref(name)
        data = g64[tensor] - 2 * V.L2_ALL * c["init"][tensor].astype(np.float64)
        g = _f32(g64)
        g[tensor] = (g64[tensor] + data).astype(np.float32)
        _rejected(g, g64)


def test_exact_check_rejects_stale_entries_and_noise():
    for name in ("mmoe-64x128-n3", "mlp-5x3-n3", "mlp-96-noclick-n16"):
        c = V.build(name)
        _, g64, nomap = _ref(name)
        k = int(np.flatnonzero(~nomap["dnn.linears.0.weight"])[0])
        g = _f32(g64)
        g["dnn.linears.0.weight"][1, k] += np.float32(1e-6)            # left from a previous batch that had a 1 in column k
        _rejected_exact(g, g64, c, nomap)
        task = "linear_model_task.0.weight" if c["spec"]["kind"] == "mmoe" else "linear_model_task.1.weight"
        g = _f32(g64)
        g[task][k, 0] += np.float32(1e-6)
        _rejected_exact(g, g64, c, nomap)
        for sign in (1.0, -1.0):
            g = _f32(g64)
            g["linear_model.weight"] = (g["linear_model.weight"].astype(np.float64) + sign * 1e-9).astype(np.float32)
            _rejected_exact(g, g64, c, nomap)
        g = _f32(g64)                                                  # the l2_linear part forgotten: 1e-3 of 2 c p
        g["linear_model.weight"] = (2 * V.L2_ALL * c["init"]["linear_model.weight"].astype(np.float64)).astype(np.float32)
        _rejected_exact(g, g64, c, nomap)
    c = V.build("mlp-96-noclick-n16")
    batch, g64, nomap = _ref("mlp-96-noclick-n16")
    clicked = V.build("mlp-96-n17")                                    # the same shape with clicks: what a data gradient there looks like
    b2, g2, _ = _ref("mlp-96-n17")
    for tensor in ("tower_network.0.weight", "out.0.bias", "mmoe_layer.gating_networks.0.weight"):
        data = g2[tensor] - 2 * V.L2_ALL * clicked["init"][tensor].astype(np.float64)
        assert np.abs(data).max() > 0
        g = _f32(g64)
        g[tensor] = (g64[tensor] + 1e-3 * data).astype(np.float32)
        _rejected_exact(g, g64, c, nomap)
    c = V.build("mlp-17x33-E1-n50")
    _, g64, nomap = _ref("mlp-17x33-E1-n50")
    for tensor in ("mmoe_layer.gating_networks.0.weight", "mmoe_layer.gating_networks.1.weight"):
        g = _f32(g64)
        g[tensor][0, 3] += np.float32(1e-7)
        _rejected_exact(g, g64, c, nomap)


def test_adam_check_rejects_a_step_count_off_by_one():
    c = V.build("mlp-40x72x24-n33")
    _, g64, _ = _ref("mlp-40x72x24-n33")
    f, d = np.float32, np.float64
    p0 = np.concatenate([v.reshape(-1) for v in c["init"].values()])
    g = np.concatenate([_f32(g64)[k].reshape(-1) for k in c["init"]])
    rng = np.random.RandomState(8)
    m0, v0 = f(0.1 * g * rng.uniform(0.5, 1.5, g.shape)), f(1e-3 * g * g * rng.uniform(0.5, 1.5, g.shape))
    lr, betas, eps = V.ADAM["lr"], V.ADAM["betas"], V.ADAM["eps"]

    def device_like(t_used):
        b1, b2, e, step_size, bc2s = (f(z) for z in V.adam_constants(t_used, lr, betas, eps))
        m1 = m0 + (f(1) - b1) * (g - m0)
        v1 = v0 * b2 + (f(1) - b2) * g * g
        return m1, v1, p0 - step_size * (m1 / (np.sqrt(v1) / bc2s + e))
    for t in (1, 3, 10000):
        m1, v1, p1 = device_like(t)
        used = V.check_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), m1.astype(d), v1.astype(d), p1.astype(d), t, lr, betas, eps)
        assert max(used) <= 1.0
        if t == 10000:       # 1 - beta^t differs between t = 10000 and 10001 by 5e-8 at the most: below fp32 and below every bar
            continue
        m1, v1, p1 = device_like(t + 1)
        with pytest.raises(AssertionError):
            V.check_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), m1.astype(d), v1.astype(d), p1.astype(d), t, lr, betas, eps)
