"""Helpers for the gradient / Adam parity tests of the two VirtualTaobao trainers (tests/test_gpu_vtb_train_grads.py,
tests/test_vtb_train_grads_cpu.py): csrc/mmoe_train.hip, csrc/mlp_train.hip and the grad_adam_kernel of csrc/train_step.hip they share.

The device step leaves `grads` = data gradient + 2 c p, the moments and the parameters in plain buffers.  check_step compares the gradient
with float64 autograd of the host restatement (cirs_hip.mmoe_host.loss_and_grad / mlp_loss_and_grad) at the parameters the step started
from, the entries that can have no data gradient with 2 c p exactly, both loss columns, and the Adam update with gradcase's float64
recurrence fed the device's OWN gradient: nothing passes through Adam's g / |g|, which hides the gradient's magnitude from
traincase.compare_params.  The Adam part is gradcase's, unchanged: tstep::adam_one (train_step.h) has the three statements of optim.h's
adam_update, the build uses -ffp-contract=off and tstep::adam_args rounds the bias corrections like adam_constants(as_device=True).

Cases come from fixed seeds (no golden file): build(name) -> dict(name, spec, init, pool).  A step's batch is the next n rows of the
case's pool that pass the kink guard (take_batch)."""
import numpy as np
import torch

import mlpcase
import mmoecase
from gradcase import ADAM, LOSS_RTOL, M_BAR, P_BAR, UPD_BAR, V_BAR, V_TINY, adam_constants, adam_moments, adam_update, check_adam  # noqa: F401

L2_LINEAR, L2_ALL = 1e-5, 1e-2
L2 = dict(l2_linear=L2_LINEAR, l2_all=L2_ALL)
N_STEPS = 4            # three consecutive steps and the step at t = 10000

# ---- the gradient bar and the kink margin ------------------------------------------------------------------------------------------
# per named tensor T:      max |g - g64| <= B * max |g64_T|
# a batch row is passed over when a hidden pre-activation of the float64 forward lies within Z_MARGIN of zero (take_batch)
# Both come from the FLOAT32 RUN OF THE HOST RESTATEMENT on the CPU against its float64 run, never from the device:
#   r_T  = max |g32 - g64| / max |g64_T|  of mmoe_host.loss_and_grad / mlp_loss_and_grad, the largest over the tensors with a data gradient
#   dz   = max |z32 - z64|                of mmoe_host.hidden_preactivations
# over the four batches of every case at the parameters the fp32 torch chain reaches (host_replay), dz over the whole pool at the
# initial parameters as well.  B = 8 x the largest r_T: the device's slab sums are sequential (up to 258 terms per slab at 1025 rows)
# where torch's are blocked.  Z_MARGIN = 16 x the largest dz.  tests/test_vtb_train_grads_cpu.py measures both again, prints this
# table and holds them within B / 4 and Z_MARGIN / 4.  Measured:
#   case                         r_T  on                                            dz  passed over
#   mmoe-64x64-n1           6.03e-06  mmoe_layer.gating_networks.0.weight     2.09e-06  0 of 4
#   mmoe-64x128-n3          1.27e-05  mmoe_layer.gating_networks.0.weight     3.68e-06  0 of 12   <- largest r_T
#   mmoe-128x64-n5          1.80e-06  mmoe_layer.gating_networks.0.weight     4.06e-06  0 of 20
#   mmoe-128x128-n16        9.70e-06  dnn.linears.0.weight                    6.62e-06  0 of 64
#   mmoe-64x64-n17          2.51e-06  mmoe_layer.gating_networks.0.weight     3.88e-06  0 of 68
#   mmoe-128x128-n129       2.55e-06  mmoe_layer.gating_networks.0.weight     8.91e-06  10 of 526   <- largest dz
#   mmoe-128x64-n1025       1.01e-06  mmoe_layer.gating_networks.0.weight     6.58e-06  46 of 4146
#   mlp-256x256-n1          2.42e-06  mmoe_layer.gating_networks.1.weight     2.73e-06  0 of 4
#   mlp-5x3-n3              2.60e-07  mmoe_layer.expert_network.bias          7.01e-07  0 of 12
#   mlp-96-n17              1.22e-05  mmoe_layer.gating_networks.0.weight     1.03e-06  0 of 68
#   mlp-40x72x24-n33        4.02e-06  mmoe_layer.gating_networks.0.weight     2.54e-06  3 of 135
#   mlp-5x3x4-n16           3.93e-07  dnn.linears.2.weight                    9.69e-07  0 of 64
#   mlp-31x256x1-n65        3.95e-07  tower_network.1.weight                  4.95e-07  1 of 261
#   mlp-17x33-E1-n50        4.01e-07  mmoe_layer.expert_network.weight        1.12e-06  1 of 201
#   mlp-256-E64-n129        8.41e-06  mmoe_layer.gating_networks.0.weight     5.67e-07  14 of 530
#   mlp-96-noclick-n16      1.98e-06  mmoe_layer.gating_networks.1.weight     1.03e-06  0 of 64
# (passed over: the rows the kink guard skipped in the four steps of the fp32 chain, of the rows it consumed.)
# The seeds are plain numbers but for two: at one row the gate's gradient is, for some rows, a difference of nearly equal terms, and
# the fp32 run's r_T on it ranged from 2e-7 to 1.3e-4 over twelve seeds; such a row would widen B for every other case, so the
# one-row MMoE case has a seed whose rows are ordinary.  Below 16 rows a single row passed over is already more than a sixteenth of a
# step, so the five-row case has a seed in which the fp32 chain passes over none.
B = 8 * 1.272e-5            # 1.02e-4
Z_MARGIN = 16 * 8.909e-6    # 1.43e-4
# One case cannot live with the common margin: the 256 units of the second layer of (31, 256, 1) have pre-activations of 0.34 on
# average (dnn_scale), and 4 to 10 % of a step's rows have one of them within 1.4e-4 of zero -- more than the share a step may pass
# over, with every one of seventeen seeds tried.  Its own forward is 18 x more exact than the largest dz, so it takes 16 x its OWN dz: a narrower guard asks more
# of the device, never less.
Z_MARGIN_31x256x1 = 16 * 4.95e-7
SKIP_SHARE_DEVICE, SKIP_SHARE_HOST = 1.0 / 8, 1.0 / 16     # the share of the rows a step consumed that the guard may pass over


def _mmoe(dnn, n, seed):
    return dict(kind="mmoe", dnn=dnn, experts=4, expert_dim=8, n=n, seed=seed, no_click=False, z_margin=None)


def _mlp(dnn, experts, expert_dim, n, seed, no_click=False, z_margin=None):
    return dict(kind="mlp", dnn=dnn, experts=experts, expert_dim=expert_dim, n=n, seed=seed, no_click=no_click, z_margin=z_margin)


CASES = {
    # ---- the one-task MMoE (K = 118: the last of four 32-wide weight tiles holds 22 columns); every shape check_cfg accepts ------------
    "mmoe-64x64-n1": _mmoe((64, 64), 1, 1112),          # three of the four row slabs empty; 15 dead tile rows; half of an MFMA row pair empty
    "mmoe-64x128-n3": _mmoe((64, 128), 3, 1102),        # fewer rows than wavefronts: rps = 2, slab 1 holds one row, slabs 2 and 3 none
    "mmoe-128x64-n5": _mmoe((128, 64), 5, 1113),        # rps = 2: slab 2 holds one row, slab 3 none
    "mmoe-128x128-n16": _mmoe((128, 128), 16, 1104),    # exactly one full row tile
    "mmoe-64x64-n17": _mmoe((64, 64), 17, 1105),        # a second row tile with one live row
    "mmoe-128x128-n129": _mmoe((128, 128), 129, 1106),  # rps = 34: a second 32-row trip of two rows; last slab of 27
    "mmoe-128x64-n1025": _mmoe((128, 64), 1025, 1107),  # rps = 258: many trips; 65 row tiles, the last with one row; last slab of 251
    # ---- the two-task MLP (K = 91: the last of three weight tiles holds 27 columns) -----------------------------------------------------
    "mlp-256x256-n1": _mlp((256, 256), 4, 8, 1, 1201),          # four column tiles per wave of mlp_rows_kernel; one row
    "mlp-5x3-n3": _mlp((5, 3), 2, 3, 3, 1202),                  # every width below 16 and odd; LoadNT's scalar path
    "mlp-96-n17": _mlp((96,), 2, 5, 17, 1203),                  # one hidden layer; a row tile of one row
    "mlp-40x72x24-n33": _mlp((40, 72, 24), 3, 6, 33, 1204),     # three layers; column tiles of 8 and 24 left over
    "mlp-5x3x4-n16": _mlp((5, 3, 4), 2, 2, 16, 1205),           # the expert matrix has K = 4 at float offset 27: a K % 4 == 0 matrix on the scalar path
    "mlp-31x256x1-n65": _mlp((31, 256, 1), 8, 8, 65, 1206, z_margin=Z_MARGIN_31x256x1),   # a layer of width 1; K = 31
    "mlp-17x33-E1-n50": _mlp((17, 33), 1, 64, 50, 1207),        # E = 1, 2 D = 128 (kLdM = 132): the gate soft-max is identically 1
    "mlp-256-E64-n129": _mlp((256,), 64, 1, 129, 1208),         # E D + 2 E = 192 fills the widest LDS plane (kLdE = 196); rps = 34
    "mlp-96-noclick-n16": _mlp((96,), 2, 5, 16, 1209, True),    # every click 0: the action task's gradient is exactly zero
}


def host_fn(spec):
    from cirs_hip import mmoe_host
    return mmoe_host.loss_and_grad if spec["kind"] == "mmoe" else mmoe_host.mlp_loss_and_grad


def pool_rows(spec):
    """Four batches and room for the rows the guard passes over."""
    return 5 * spec["n"] + 24


_cache = {}


def build(name):
    """-> dict(name, spec, init {name: fp32 array}, pool = the batch columns (x, y, exposure | x, y) as fp32 arrays of pool_rows rows);
    built once, shared, never modified by a test."""
    if name not in _cache:
        spec = CASES[name]
        if spec["kind"] == "mmoe":
            init = mmoecase.stressed_init(spec["dnn"])
            pool = mmoecase.inputs(pool_rows(spec), seed=spec["seed"])
        else:
            dnn = spec["dnn"]
            init = mlpcase.stressed_init(dnn, spec["experts"], spec["expert_dim"], scale=mlpcase.dnn_scale(dnn) if max(dnn) > 128 else None)
            pool = mlpcase.inputs(pool_rows(spec), seed=spec["seed"], no_click=spec["no_click"])
        # one fp32 image feeds the device and the float64 reference alike
        _cache[name] = dict(name=name, spec=spec, init={k: np.asarray(v, np.float32) for k, v in init.items()},
                            pool=tuple(np.ascontiguousarray(c, np.float32) for c in pool))
    return _cache[name]


def make_trainer(case):
    from cirs_hip.mmoe_train import MlpTrainer, MMoETrainer
    cls = MMoETrainer if case["spec"]["kind"] == "mmoe" else MlpTrainer
    return cls(case["init"], **L2, **ADAM)


# ---- the kink guard ------------------------------------------------------------------------------------------------------------------
def min_abs_z(p, x):
    """Per row of x the smallest |pre-activation| over every hidden unit, in the float64 forward at the parameters p."""
    from cirs_hip import mmoe_host
    return np.min([z.abs().min(1).values.numpy() for z in mmoe_host.hidden_preactivations(p, x, torch.float64)], axis=0)


def margin_of(spec):
    return Z_MARGIN if spec["z_margin"] is None else spec["z_margin"]


def take_batch(case, cursor, p, max_share, what="", z_margin=None):
    """The next n rows of the pool from `cursor` on whose hidden pre-activations all stay Z_MARGIN away from zero in the float64 forward at
    p (a unit closer than that may take the other side of the relu in fp32, and one flipped unit moves a weight-gradient row by a whole
    sample's share).  -> (batch columns, new cursor, rows passed over).  The count is printed; more than max_share of the consumed rows
    passed over fails."""
    n, pool = case["spec"]["n"], case["pool"]
    ok = min_abs_z(p, pool[0][cursor:]) >= (margin_of(case["spec"]) if z_margin is None else z_margin)
    keep = np.flatnonzero(ok)[:n]
    assert len(keep) == n, f"{what}: the pool of {len(pool[0])} rows is used up"
    consumed = int(keep[-1]) + 1
    skipped = consumed - n
    print(f"{what}: kink guard passed over {skipped} of {consumed} rows")
    assert skipped <= max_share * consumed, f"{what}: the kink guard passed over {skipped} of {consumed} rows (more than {max_share:.4f})"
    return tuple(c[cursor + keep] for c in pool), cursor + consumed, skipped


# ---- which entries carry a data gradient -------------------------------------------------------------------------------------------
def no_data_grad(spec, x):
    """{tensor name: False (no data gradient by construction) | boolean mask over the INPUT columns k, True where some batch row has
    x[:, k] != 0 (`dnn.linears.0.weight` [H, K]: its columns; `linear_model_task.*.weight` [K, 1]: its entries)}; a tensor not named has
    a data gradient everywhere.  Decided from the structure of the batch alone."""
    live = (np.asarray(x) != 0).any(0)
    out = {"linear_model.weight": False, "dnn.linears.0.weight": live}
    if spec["kind"] == "mmoe":
        out["linear_model_task.0.weight"] = live
        return out
    out["linear_model_task.1.weight"] = live
    if spec["no_click"]:       # d loss / d y_pred of the action task is 2 click (...) / 27 n = 0
        out.update({"tower_network.0.weight": False, "out.0.bias": False, "mmoe_layer.gating_networks.0.weight": False})
    if spec["experts"] == 1:   # a soft-max over one logit is the constant 1
        out.update({"mmoe_layer.gating_networks.0.weight": False, "mmoe_layer.gating_networks.1.weight": False})
    return out


def l2_of(name):
    """The regulariser's constant of a tensor from the fp32 constants the device receives, in float64."""
    c = np.float64(np.float32(L2_ALL))
    return c + np.float64(np.float32(L2_LINEAR)) if name == "linear_model.weight" else c


# ---- the comparators (host only: the CPU test feeds them mutated gradients) ---------------------------------------------------------
def grad_ratios(g, g64, nomap):
    """-> {name: max |g - g64| / max |g64_T|} over the tensors with a data gradient.  Those marked False are left out: there the fp32 host
    run shows the rounding noise of a sum that is identically zero, which the device never forms (check_exact holds them to 2 ulp)."""
    out = {}
    for name, want in g64.items():
        if nomap.get(name) is False:
            continue
        want = np.asarray(want, np.float64)
        err = np.abs(np.asarray(g[name], np.float64).reshape(want.shape) - want).max()
        top = np.abs(want).max()
        out[name] = float(err / top) if top > 0 else (0.0 if err == 0 else np.inf)
    return out


def check_grads(g, g64, b=None, what=""):
    """The gradient bar of the module's head on every tensor of g64.  -> the largest share of B used."""
    b = B if b is None else b
    used = 0.0
    assert set(g) == set(g64), f"{what}: tensors {sorted(set(g) ^ set(g64))}"
    for name, want in g64.items():
        want = np.asarray(want, np.float64)
        got = np.asarray(g[name], np.float64)
        assert got.shape == want.shape, f"{what}: {name}: shape {got.shape} for {want.shape}"
        err, top = np.abs(got - want), np.abs(want).max()
        assert err.max() <= b * top, (f"{what}: {name}: max |g - g64| {err.max():.3e} > B max |g64| = {b * top:.3e} "
                                      f"(ratio {err.max() / max(top, 1e-300):.3e}) at {np.unravel_index(int(err.argmax()), err.shape)}")
        if top > 0:
            used = max(used, float(err.max() / (b * top)))
    return used


def check_exact(g, p, nomap, what=""):
    """Entries without a data gradient by construction hold 2 c p to within 2 ulp (fp32).  g, p: {name: fp32 arrays}.  -> the largest
    share of the 2 ulp used."""
    used = 0.0
    for name, m in nomap.items():
        gi, pi = np.asarray(g[name], np.float32), np.asarray(p[name], np.float32)
        assert gi.shape == pi.shape
        if m is False:
            sel = np.ones(gi.shape, bool)
        elif name == "dnn.linears.0.weight":
            sel = np.broadcast_to(~m[None, :], gi.shape)
        else:
            sel = np.broadcast_to(~m[:, None], gi.shape)
        if not sel.any():
            continue
        got = gi[sel].astype(np.float64)
        want = 2.0 * l2_of(name) * pi[sel].astype(np.float64)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        bad = np.abs(got - want) > 2 * ulp
        assert not bad.any(), (f"{what}: {name}: {int(bad.sum())} of {int(sel.sum())} entries without a data gradient differ from 2 c p by "
                               f"more than 2 ulp (largest {np.abs(got - want).max():.3e})")
        used = max(used, float((np.abs(got - want) / (2 * ulp)).max()))
    return used


def check_loss(loss, cols, what=""):
    loss, cols = np.asarray(loss, np.float64), np.asarray(cols, np.float64)
    print(f"{what}: loss device {loss.tolist()} float64 {cols.tolist()}")
    np.testing.assert_allclose(loss, cols, rtol=LOSS_RTOL, atol=0, err_msg=f"{what}: loss columns")
    return float((np.abs(loss - cols) / (LOSS_RTOL * np.abs(cols))).max())


def reference(case, p, batch, dtype=torch.float64, **l2):
    """Loss columns and gradient of `batch` at the parameters p (name -> array) as numpy arrays."""
    cols, grads = host_fn(case["spec"])(p, *batch, **(l2 or L2), dtype=dtype)
    return cols.numpy(), {k: v.numpy() for k, v in grads.items()}


# ---- the fp32 torch chain that stands in for the device on the CPU -----------------------------------------------------------------
def host_replay(case, z_margin=None):
    """The four batches of a case as the kink guard builds them when fp32 autograd + torch.optim.Adam stand in for the device step.
    Yields (step index, parameters the step starts from {name: fp32 array}, batch, rows passed over, rows consumed)."""
    p = {k: torch.tensor(v, requires_grad=True) for k, v in case["init"].items()}
    opt = torch.optim.Adam(list(p.values()), **ADAM)
    fn, cursor = host_fn(case["spec"]), 0
    for st in range(N_STEPS):
        start = {k: v.detach().numpy().copy() for k, v in p.items()}
        batch, new_cursor, skipped = take_batch(case, cursor, start, SKIP_SHARE_HOST, what=f"{case['name']} host step {st + 1}", z_margin=z_margin)
        yield st, start, batch, skipped, new_cursor - cursor
        cursor = new_cursor
        _, grads = fn(start, *batch, **L2, dtype=torch.float32)
        for k, v in p.items():
            v.grad = grads[k]
        opt.step()


# ---- the device step check -----------------------------------------------------------------------------------------------------------
def _np(named):
    return {k: v.detach().cpu().numpy() for k, v in named.items()}


def check_step(tr, case, cursor, what="", record=True):
    """One device step on the next guarded batch of the case's pool, checked as the module's head describes.
    -> (new cursor, dict of the shares of each bar the device used)."""
    from conftest import close
    p_named = _np(tr.state_dict())
    batch, cursor, _ = take_batch(case, cursor, p_named, SKIP_SHARE_DEVICE, what=what)
    p0, m0, v0, t0 = tr.flat.clone(), tr.adam_m.clone(), tr.adam_v.clone(), tr.step_count
    loss = tr.step(*batch).cpu().numpy().astype(np.float64)
    assert tr.step_count == t0 + 1
    g, m1, v1, p1 = (z.cpu().numpy() for z in (tr.grads, tr.adam_m, tr.adam_v, tr.flat))
    p0, m0, v0 = p0.cpu().numpy(), m0.cpu().numpy(), v0.cpu().numpy()
    assert all(np.isfinite(z).all() for z in (g, m1, v1, p1, loss)), f"{what}: non-finite values after the step"
    g_named = _np(tr.gradients())
    cols, g64 = reference(case, p_named, batch)
    used = dict(grad=check_grads(g_named, g64, what=what), loss=check_loss(loss, cols, what=what),
                exact=check_exact(g_named, p_named, no_data_grad(case["spec"], batch[0]), what=what))
    d = np.float64
    used["adam_m"], used["adam_v"], used["adam_p"] = check_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), m1.astype(d), v1.astype(d),
                                                                p1.astype(d), t0 + 1, ADAM["lr"], ADAM["betas"], ADAM["eps"], what=what)
    print(f"{what}: share of each bar used {{{', '.join(f'{k}: {v:.4f}' for k, v in used.items())}}}")
    if record:          # the headroom goes to the session's parity_margins.json: err / bar against 0 with atol 1
        close(np.array(list(used.values())), np.zeros(len(used)), rtol=0, atol=1.0, what=f"vtb train grads {what} {list(used)}")
    return cursor, used
