"""Helpers for the gradient / Adam parity tests of the Kuaishou trainers (tests/test_gpu_usertrain_grads.py, tests/test_usertrain_grads_cpu.py).

The device step leaves `grads` = data gradient + 2 c p, the moments and the parameters in plain buffers: check_step compares the gradient
with float64 autograd of the host restatement (cirs_hip.deepfm_host / dice_host .loss_and_grad), the entries that can have no data gradient
with 2 c p exactly, and the Adam update with the float64 recurrence fed the device's OWN gradient -- none of it passes through Adam's
g / |g|, which hides the gradient's magnitude from the parameter comparisons of the older tests.

Cases are generated from fixed seeds (no golden file): build(name) -> dict(spec, init, batches, hyper)."""
import numpy as np
import torch

LOSS_RTOL = 3e-5
L2 = dict(l2_embedding=1e-5, l2_linear=1e-5, l2_all=0.1)
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)

# ---- the gradient bars -----------------------------------------------------------------------------------------------------------
# per named tensor T:      max |g - g64| <= B * max |g64_T|
# per touched table row:   max |g_row - g64_row| <= B_ROW * max |g64_row| + B * 1e-2 * max |g64_T|
# B and B_ROW are 8 x the largest ratio the fp32 run of loss_and_grad on the CPU shows against its float64 run, over every case and tensor
# below (r_T = max |g32 - g64| / max |g64_T|; r_row = the smallest factor with which every touched row of the fp32 run meets the row
# formula at this B).  8 x: the device sums sequentially per key and per row slab (up to 16400 terms, error ~ sqrt(n) 2^-24) where torch's
# blocked sums do not grow.  The device's own error never enters.  tests/test_usertrain_grads_cpu.py measures the ratios again and holds
# them within B / 4 and B_ROW / 4.  Measured (largest over the four batches of each case):
#   case                            r_T      r_row
#   deepfm-pairwise-ab           2.63e-07  0.00e+00
#   deepfm-ips                   3.39e-07  0.00e+00
#   deepfm-pd                    7.47e-07  3.12e-07
#   deepfm-pairwise              3.40e-07  0.00e+00
#   dice-E8                      6.56e-07  0.00e+00
#   dice-E16                     4.98e-07  0.00e+00
#   dice-E32                     5.85e-07  0.00e+00
#   deepfm-ips-n1                3.29e-06  2.23e-06
#   deepfm-ips-n3                5.12e-07  0.00e+00
#   dice-n1                      2.35e-06  2.13e-06
#   dice-n3                      5.42e-06  5.82e-09
#   deepfm-pd-segments           6.06e-07  0.00e+00
#   dice-segments                2.45e-06  1.93e-06
#   deepfm-pairwise-ab-slabcap   6.55e-06  1.59e-05      <- both largest ratios
#   dice-slabcap                 3.60e-06  7.38e-08
#   deepfm-ips-bigtables         3.25e-07  0.00e+00
#   dice-bigtables               6.04e-07  0.00e+00
#   deepfm-pairwise-ab-E5        2.38e-06  0.00e+00
#   deepfm-pairwise-ab-E33       3.34e-07  0.00e+00
#   deepfm-pairwise-ab-E64       8.98e-07  1.72e-06
# (r_row = 0: the floor B * 1e-2 * max |g64_T| of the row formula already covers every touched row of the fp32 run.)
B = 8 * 6.553e-6            # 5.24e-5
B_ROW = 8 * 1.588e-5        # 1.27e-4

# ---- the Adam bars: derived, a handful of fp32 roundings each (the build divides and takes square roots correctly rounded) -------
#   m' = m + (1 - b1) (g - m)                 three roundings of terms <= |m| + |g|:          |dm| <= 2^-21 (|m| + |g|)
#   v' = b2 v + (1 - b2) g g                  four roundings of positive terms <= v':          |dv| <= 2^-20 v' + 1.2e-38 (underflow of g g)
#   p' = p - step (m' / (sqrt(v') / bc2s + eps))  five roundings in the update, one of p':    |dp| <= 2^-23 |p| + 2^-19 |update|
M_BAR, V_BAR, V_TINY, P_BAR, UPD_BAR = 2.0 ** -21, 2.0 ** -20, 1.2e-38, 2.0 ** -23, 2.0 ** -19


def _spec(trainer, E, U, I, F, n, seed, kind=None, use_ab=False, special=None):
    return dict(trainer=trainer, E=E, U=U, I=I, F=F, n=n, seed=seed, kind=kind, use_ab=use_ab, special=special)


CASES = {
    # 1, 2: the recorded shape; every loss kind, alpha/beta, the three DICE embedding sizes
    "deepfm-pairwise-ab": _spec("deepfm", 8, 50, 80, 32, 37, 101, "pairwise", True),
    "deepfm-ips": _spec("deepfm", 8, 50, 80, 32, 37, 102, "ips"),
    "deepfm-pd": _spec("deepfm", 8, 50, 80, 32, 37, 103, "pd"),
    "deepfm-pairwise": _spec("deepfm", 8, 50, 80, 32, 37, 104, "pairwise"),
    "dice-E8": _spec("dice", 8, 50, 80, 32, 37, 201),
    "dice-E16": _spec("dice", 16, 50, 80, 32, 37, 202),
    "dice-E32": _spec("dice", 32, 50, 80, 32, 37, 203),
    # 3: fewer rows than the workgroup's four wavefronts
    "deepfm-ips-n1": _spec("deepfm", 8, 7, 9, 32, 1, 301, "ips"),
    "deepfm-ips-n3": _spec("deepfm", 8, 7, 9, 32, 3, 302, "ips"),
    "dice-n1": _spec("dice", 8, 7, 9, 32, 1, 303),
    "dice-n3": _spec("dice", 8, 7, 9, 32, 3, 304),
    # 4: long segments (one user, padding features), ids 0 and V - 1, more than 16 row slabs
    "deepfm-pd-segments": _spec("deepfm", 16, 7, 600, 32, 600, 401, "pd", special="segments"),
    "dice-segments": _spec("dice", 16, 7, 600, 32, 600, 402, special="segments"),
    # 5, 6: more rows than 256 slabs of 64
    "deepfm-pairwise-ab-slabcap": _spec("deepfm", 16, 64, 128, 32, 8200, 501, "pairwise", True),
    "dice-slabcap": _spec("dice", 8, 64, 128, 32, 4100, 601),
    # 7, 8: more parameters than one trip of the Adam kernel's grid
    "deepfm-ips-bigtables": _spec("deepfm", 16, 3000, 12000, 32, 64, 701, "ips"),
    "dice-bigtables": _spec("dice", 16, 3000, 6000, 32, 64, 801),
    # 9: embedding sizes the DeepFM entry accepts and nothing else runs
    "deepfm-pairwise-ab-E5": _spec("deepfm", 5, 20, 30, 16, 37, 901, "pairwise", True),
    "deepfm-pairwise-ab-E33": _spec("deepfm", 33, 20, 30, 16, 37, 902, "pairwise", True),
    "deepfm-pairwise-ab-E64": _spec("deepfm", 64, 20, 30, 16, 37, 903, "pairwise", True),
}
N_BATCHES = 4          # three consecutive steps and the step at t = 10000


def host_module(spec):
    from cirs_hip import deepfm_host, dice_host
    return deepfm_host if spec["trainer"] == "deepfm" else dice_host


def layout(spec):
    from cirs_hip import deepfm_train, dice_train
    return (deepfm_train if spec["trainer"] == "deepfm" else dice_train).layout(spec["U"], spec["I"], spec["F"], spec["E"])


def _init(spec, rng):
    """Dense weight matrices ~N(0, 1/sqrt(fan_in)); tables N(0, 0.3) like the recorded cases, padding row 0; alpha / beta 1 +- 0.2.  The
    weight of the raw duration (up to 60) is N(0, 0.02) so that logits stay moderate; biases are small and non-zero, the two output
    biases in +-[0.002, 0.01] (small enough that 1e-9 is many ulp of 2 c p)."""
    init = {}
    for name, shape in layout(spec):
        if name.startswith("ab_embedding_dict."):
            if not spec["use_ab"]:
                continue
            w = rng.uniform(0.8, 1.2, shape)
        elif "embedding_dict" in name:
            w = rng.normal(0, 0.3, shape)
        elif name in ("linear.weight", "linear_main.weight", "linear_model.weight"):
            w = rng.normal(0, 0.02, shape)
        elif name.startswith("out"):
            w = rng.uniform(0.002, 0.01, shape) * rng.choice([-1.0, 1.0], shape)
        elif name.endswith(".bias"):
            w = rng.normal(0, 0.01, shape)
        else:
            w = rng.normal(0, 1.0 / np.sqrt(shape[-1]), shape)
        init[name] = w.astype(np.float32)
    init["embedding_dict.feat.weight"][0] = 0
    return init


def _feats(rng, n, F, pad_rows=None):
    f = np.where(np.arange(4)[None, :] < rng.randint(1, 5, n)[:, None], rng.randint(1, F, (n, 4)), 0)
    if pad_rows is not None:
        f[pad_rows] = 0
    return f


def _batch(spec, rng, b):
    """One batch: ids inside their tables, y in [0, 5], durations in [2, 60], the score of the loss kind."""
    n, U, I, F = spec["n"], spec["U"], spec["I"], spec["F"]
    seg = spec["special"] == "segments"
    user = rng.randint(0, U, n)
    pos, neg = rng.randint(0, I, n), rng.randint(0, I, n)
    pad_p = pad_n = None
    if seg:
        if b % 2 == 0:
            user[:] = 3                                # one segment of every user row
        else:
            user[0], user[1] = 0, U - 1
        pad_p, pad_n = rng.rand(n) < 0.5, rng.rand(n) < 0.5      # all-padding feature rows: key 0 far more than 1000 times
        pos[0], pos[1], neg[2], neg[3] = 0, I - 1, 0, I - 1
    fp, fn = _feats(rng, n, F, pad_p), _feats(rng, n, F, pad_n)
    if seg:
        fp[5, 0], fn[6, 3] = F - 1, F - 1
    dp, dn = rng.uniform(2, 60, n), rng.uniform(2, 60, n)
    y = rng.uniform(0, 5, n)
    if spec["trainer"] == "deepfm":
        user_neg = np.where(rng.rand(n) < 0.2, rng.randint(0, U, n), user)      # the negative pair mostly, not always, has the positive's user
        x = np.column_stack([user, pos, fp, dp, user_neg, neg, fn, dn])
        score = {"pairwise": rng.uniform(0, 3, n), "ips": np.exp(rng.uniform(np.log(0.05), np.log(20), n)), "pd": rng.uniform(0.01, 1, n)}[spec["kind"]]
    else:
        user_con = user if seg else rng.randint(0, U, n)
        pos_con, neg_con = rng.randint(0, I, n), rng.randint(0, I, n)
        x = np.column_stack([user, user_con, pos, pos_con, fp, dp, neg, neg_con, fn, dn])
        score = np.ones(n) if (b == 1 and n > 3) else rng.choice([-1.0, 1.0], n)
        if n > 3 and b != 1:
            score[0], score[1] = 1.0, -1.0
    return x.astype(np.float32), y.astype(np.float32), score.astype(np.float32)


_cache = {}


def build(name):
    """-> dict(name, spec, init, batches [N_BATCHES x (x, y, score)], hyper = the keyword arguments of loss_and_grad); built once, shared,
    never modified by a test."""
    if name not in _cache:
        spec = CASES[name]
        rng = np.random.RandomState(spec["seed"])
        hyper = dict(L2)
        if spec["trainer"] == "deepfm":
            hyper.update(kind=spec["kind"], use_ab=spec["use_ab"], lambda_ab=0.7 if spec["use_ab"] else 0.0)
        _cache[name] = dict(name=name, spec=spec, init=_init(spec, rng), batches=[_batch(spec, rng, b) for b in range(N_BATCHES)], hyper=hyper)
    return _cache[name]


def make_trainer(case):
    spec, h = case["spec"], case["hyper"]
    if spec["trainer"] == "deepfm":
        from cirs_hip.deepfm_train import DeepFMTrainer
        return DeepFMTrainer(case["init"], use_ab=h["use_ab"], lambda_ab=h["lambda_ab"], loss_kind=h["kind"], **L2, **ADAM)
    from cirs_hip.dice_train import DiceTrainer
    return DiceTrainer(case["init"], **L2, **ADAM)


# ---- which entries carry a data gradient ---------------------------------------------------------------------------------------
def touched(spec, x):
    """{tensor name: boolean row mask of the rows the batch's ids reach | None (dense layer: every entry) | False (no data gradient by
    construction)} for every tensor of the layout."""
    x = np.asarray(x)
    sizes = dict(U=spec["U"], I=spec["I"], F=spec["F"])

    def rows(which, cols):
        m = np.zeros(sizes[which], bool)
        m[x[:, cols].astype(np.int64).reshape(-1)] = True
        return m
    out = {}
    if spec["trainer"] == "deepfm":
        u, i, f = rows("U", [0, 7]), rows("I", [1, 8]), rows("F", [2, 3, 4, 5, 9, 10, 11, 12])
        f_emb = f.copy(); f_emb[0] = False                       # padding_idx = 0
        for name, _ in layout(spec):
            if name.startswith("linear_model."):
                out[name] = False
            elif name.startswith("ab_embedding_dict."):
                out[name] = (rows("U", [0]) if "alpha_u" in name else rows("I", [1])) if spec["use_ab"] else False
            elif "embedding_dict" in name:
                out[name] = u if "user_id" in name else i if "photo_id" in name else f_emb if name == "embedding_dict.feat.weight" else f
            else:
                out[name] = None
        return out
    f = rows("F", [4, 5, 6, 7, 11, 12, 13, 14])
    f_emb = f.copy(); f_emb[0] = False
    by_table = dict(user_int=rows("U", [0]), user_con=rows("U", [1]), photo_int=rows("I", [2, 9]), photo_con=rows("I", [3, 10]))
    for name, _ in layout(spec):
        if name.startswith("linear_model.") or name in ("linear_ui.embedding_dict.user_int.weight", "out_ui.bias"):
            out[name] = False            # linear_ui's user weight and out_ui.bias sit in both forwards of every BPR difference
        elif name == "linear_ui.embedding_dict.photo_int.weight":
            out[name] = rows("I", [2, 9, 3, 10])               # indexed with the con ids in the con calls
        elif "embedding_dict" in name:
            t = name.split("embedding_dict.")[1].split(".")[0]
            out[name] = (f_emb if name == "embedding_dict.feat.weight" else f) if t == "feat" else by_table[t]
        else:
            out[name] = None
    return out


def l2_of(name, l2_embedding, l2_linear, l2_all, **_):
    """The regulariser's constant of a tensor, summed in fp32 like the device's."""
    c = np.float32(l2_all)
    if name.startswith("embedding_dict."):
        c = np.float32(l2_embedding) + c
    if name.startswith("linear_model."):
        c = np.float32(l2_linear) + c
    return c


# ---- the comparators (host only: the CPU test feeds them mutated gradients) -------------------------------------------------------
def grad_ratios(g, g64, tmap, b=None):
    """-> {name: (r_T, r_row)}: r_T = max |g - g64| / max |g64_T|; r_row = the smallest B_ROW with which every touched row meets the row
    formula at B = b (None when the tensor has no rows to check or b is None).  Tensors without a data gradient by construction are left
    out: there the fp32 host run shows the rounding noise of a sum that is identically zero, which the device never forms (check_exact
    holds those to 2 ulp instead)."""
    out = {}
    for name, want in g64.items():
        if tmap[name] is False:
            continue
        want = np.asarray(want, np.float64)
        err = np.abs(np.asarray(g[name], np.float64).reshape(want.shape) - want)
        top = np.abs(want).max()
        r_t = float(err.max() / top) if top > 0 else (0.0 if err.max() == 0 else np.inf)
        r_row = None
        m = tmap[name]
        if b is not None and isinstance(m, np.ndarray) and m.any():
            e_row = err.reshape(len(m), -1).max(1)[m]
            w_row = np.abs(want).reshape(len(m), -1).max(1)[m]
            over = np.maximum(e_row - b * 1e-2 * top, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(over > 0, over / w_row, 0.0)
            r_row = float(r.max())
        out[name] = (r_t, r_row)
    return out


def check_grads(g, g64, tmap, b=None, b_row=None, what=""):
    """The gradient bar of the module's head on every tensor of g64.  -> (largest share of B used, largest share of the row bar used)."""
    b, b_row = B if b is None else b, B_ROW if b_row is None else b_row
    used_t = used_row = 0.0
    for name, want in g64.items():
        want = np.asarray(want, np.float64)
        err = np.abs(np.asarray(g[name], np.float64).reshape(want.shape) - want)
        top = np.abs(want).max()
        assert err.max() <= b * top, f"{what}: {name}: max |g - g64| {err.max():.3e} > B max |g64| = {b * top:.3e} (ratio {err.max() / max(top, 1e-300):.3e})"
        if top > 0:
            used_t = max(used_t, float(err.max() / (b * top)))
        m = tmap[name]
        if isinstance(m, np.ndarray) and m.any():
            e_row = err.reshape(len(m), -1).max(1)[m]
            bar = b_row * np.abs(want).reshape(len(m), -1).max(1)[m] + b * 1e-2 * top
            worst = int(np.argmax(e_row / bar))
            assert np.all(e_row <= bar), f"{what}: {name}: row {np.flatnonzero(m)[worst]}: |g - g64| {e_row[worst]:.3e} > row bar {bar[worst]:.3e}"
            used_row = max(used_row, float((e_row / bar).max()))
    return used_t, used_row


def check_exact(g, p, tmap, l2, what=""):
    """Entries without a data gradient by construction hold 2 c p to within 2 ulp (fp32): untouched table rows, the padding row, tensors
    marked False.  g, p: {name: fp32 arrays}; a tensor absent from p (alpha / beta without use_ab) is all zeros."""
    for name, m in tmap.items():
        if m is None or name not in g:          # a host gradient has no alpha / beta entry without use_ab; the device's always has
            continue
        gi = np.asarray(g[name], np.float32)
        pi = np.asarray(p[name], np.float32).reshape(gi.shape) if name in p else np.zeros_like(gi)
        sel = np.ones(gi.shape[0], bool) if m is False else ~m
        if not sel.any():
            continue
        got = gi.reshape(gi.shape[0], -1)[sel].astype(np.float64)
        want = (2.0 * np.float64(l2_of(name, **l2))) * pi.reshape(gi.shape[0], -1)[sel].astype(np.float64)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        bad = np.abs(got - want) > 2 * ulp
        assert not bad.any(), (f"{what}: {name}: {int(bad.sum())} entries without a data gradient differ from 2 c p by more than 2 ulp "
                               f"(largest {np.abs(got - want).max():.3e})")


def adam_constants(t, lr, betas, eps, as_device=True):
    """-> (b1, b2, eps, step_size, bc2s) of step number t (1-based) in float64.  as_device: lr, betas and eps are the fp32 values the
    entry receives and the two bias corrections are rounded to fp32 after being formed in double, like dice_launch_step's."""
    if not as_device:
        return betas[0], betas[1], eps, lr / (1.0 - betas[0] ** t), np.sqrt(1.0 - betas[1] ** t)
    b1, b2, eps, lr = (np.float64(np.float32(z)) for z in (betas[0], betas[1], eps, lr))
    return b1, b2, eps, np.float64(np.float32(lr / (1.0 - b1 ** t))), np.float64(np.float32(np.sqrt(1.0 - b2 ** t)))


def adam_moments(m, v, g, b1, b2):
    return m + (1.0 - b1) * (g - m), b2 * v + (1.0 - b2) * g * g


def adam_update(p, m1, v1, step_size, bc2s, eps):
    upd = step_size * (m1 / (np.sqrt(v1) / bc2s + eps))
    return p - upd, upd


def check_adam(p0, m0, v0, g, m1, v1, p1, t, lr, betas, eps, what=""):
    """Device moments / parameters (fp32 arrays as float64) against the recurrence fed the device's own gradient; the parameter update
    from the device's own new moments.  -> the largest share of the three bars used."""
    b1, b2, eps, step_size, bc2s = adam_constants(t, lr, betas, eps)
    rm, rv = adam_moments(m0, v0, g, b1, b2)
    dm, bar_m = np.abs(m1 - rm), M_BAR * (np.abs(m0) + np.abs(g))
    dv, bar_v = np.abs(v1 - rv), V_BAR * rv + V_TINY
    rp, upd = adam_update(p0, m1, v1, step_size, bc2s, eps)
    dp, bar_p = np.abs(p1 - rp), P_BAR * np.abs(p0) + UPD_BAR * np.abs(upd)
    used = []
    for tag, d, bar in (("m", dm, bar_m), ("v", dv, bar_v), ("p", dp, bar_p)):
        ok = d <= bar
        i = int(np.argmax(d - bar))
        assert ok.all(), f"{what}: Adam {tag}: {int((~ok).sum())} entries outside the bar, worst at {i}: |diff| {d[i]:.3e} > {bar[i]:.3e}"
        with np.errstate(divide="ignore", invalid="ignore"):
            used.append(float(np.where(bar > 0, d / bar, 0.0).max()))
    return used


def reference(case, p, batch):
    """float64 loss columns and gradient of `batch` at the parameters p (name -> array)."""
    cols, grads = host_module(case["spec"]).loss_and_grad(p, *batch, **case["hyper"], dtype=torch.float64)
    return cols.numpy(), {k: v.numpy() for k, v in grads.items()}


# ---- the device step check ----------------------------------------------------------------------------------------------------------
def _named(tr, flat):
    """A flat host array -> {name: view} along the trainer's layout."""
    out = {}
    for name, view in tr.views.items():
        off = (view.data_ptr() - tr.flat.data_ptr()) // 4
        out[name] = flat[off:off + view.numel()].reshape(tuple(view.shape))
    return out


def _spec_of(tr):
    c = tr.cfg
    return dict(trainer="dice" if type(tr).__name__ == "DiceTrainer" else "deepfm", U=c.n_user_vocab, I=c.n_item_vocab, F=c.n_feat_vocab,
                E=c.emb_dim, use_ab=getattr(tr, "use_ab", False))


def check_step(tr, host, batch, hyper, what="", record=True):
    """One device step on `batch`, checked as the module's head describes.  -> dict of the shares of each bar the device used."""
    from conftest import close
    spec = _spec_of(tr)
    p0, m0, v0, t0 = tr.flat.clone(), tr.adam_m.clone(), tr.adam_v.clone(), tr.step_count
    loss = tr.step(*batch).cpu().numpy().astype(np.float64)
    assert tr.step_count == t0 + 1
    g, m1, v1, p1 = (z.cpu().numpy() for z in (tr.grads, tr.adam_m, tr.adam_v, tr.flat))
    p0, m0, v0 = p0.cpu().numpy(), m0.cpu().numpy(), v0.cpu().numpy()
    assert all(np.isfinite(z).all() for z in (g, m1, v1, p1, loss)), f"{what}: non-finite values after the step"
    g_named, p_named = _named(tr, g), _named(tr, p0)
    absent = [k for k in p_named if k.startswith("ab_embedding_dict.") and not hyper.get("use_ab", True)]
    p_host = {k: v for k, v in p_named.items() if k not in absent}
    cols, grads = host.loss_and_grad(p_host, *batch, **hyper, dtype=torch.float64)
    cols, g64 = cols.numpy(), {k: v.numpy() for k, v in grads.items()}
    tmap = touched(spec, batch[0])
    used_t, used_row = check_grads(g_named, g64, tmap, what=what)
    print(f"{what}: loss device {loss.tolist()} float64 {cols.tolist()}")
    np.testing.assert_allclose(loss, cols, rtol=LOSS_RTOL, atol=0, err_msg=f"{what}: loss columns")
    l2 = {k: hyper[k] for k in ("l2_embedding", "l2_linear", "l2_all")}
    check_exact(g_named, p_host, tmap, l2, what=what)
    for k in absent:
        assert not g_named[k].any() and not _named(tr, p1)[k].any(), f"{what}: {k} must stay zero without alpha/beta"
    d = np.float64
    used_m, used_v, used_p = check_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), m1.astype(d), v1.astype(d), p1.astype(d), t0 + 1,
                                        tr.lr, tr.betas, tr.eps, what=what)
    used = dict(grad=used_t, grad_row=used_row, adam_m=used_m, adam_v=used_v, adam_p=used_p)
    print(f"{what}: share of each bar used {used}")
    if record:          # the headroom goes to the session's parity_margins.json: err / bar against 0 with atol 1
        close(np.array(list(used.values())), np.zeros(len(used)), rtol=0, atol=1.0, what=f"usertrain grads {what} {list(used)}")
    return used
