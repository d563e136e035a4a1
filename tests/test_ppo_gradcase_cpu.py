"""CPU: what tests/test_gpu_ppo_step_grads.py stands on (tests/ppogradcase.py).

1. The reference is the reference's: ppo_loss in float64 on the first minibatch of the two recorded updates (tests/golden/learn.npz, and
   learn_opts.npz with dual clip) gives the recorded loss terms.
2. Every case, after the builder's deterministic adjustment, keeps every row MARGIN away from every branch point of the loss (no row is left
   out), populates every branch of the backward, and is one on which a plain fp32 evaluation agrees with float64 to 1e-5 -- so the bar the
   device is held to (4 x the fp32 evaluation's error, at least 3e-6) never exceeds 4e-5.
3. The clip + Adam comparator accepts an fp32 emulation of adam_next_kernel's element update and rejects the mistakes it is there for."""
import numpy as np
import pytest
import torch

import nn_oracle
import ppogradcase as pg
from conftest import close
from test_oracle_learn import load_learn

E32_MAX = 1e-5


@pytest.mark.parametrize("golden", ["learn", "learn_opts"])
def test_ppo_loss_reproduces_the_recorded_first_minibatch(golden_dir, golden):
    z, _, pp, perms = load_learn(golden_dir, golden)
    _, _, eps_clip, vf_coef, ent_coef, _, _, bs, _ = z["hyper"]
    dual_clip = float(z["opts"][0]) if float(z["opts"][0]) > 1.0 else None
    assert (dual_clip is not None) == (golden == "learn_opts")
    idx = torch.as_tensor(perms[0][:int(bs)]).long()
    obs = nn_oracle.flatten_episodes(torch.as_tensor(z["obs"]), z["lens"]).double()
    col = lambda k: torch.as_tensor(z[k]).double()[idx]
    got = pg.ppo_loss({k: v.double() for k, v in pp.items()}, obs[idx], torch.as_tensor(z["b_act"]).long()[idx], col("b_adv"), col("b_returns"),
                      col("b_v_s"), col("b_logp_old"), eps_clip=float(eps_clip), vf_coef=float(vf_coef), ent_coef=float(ent_coef), norm_adv=True,
                      value_clip=True, dual_clip=dual_clip)
    for x, k in zip(got, ("loss", "loss_clip", "loss_vf", "loss_ent")):
        close(float(x), z[k][0], 1e-5, 1e-5, f"ppo_loss on {golden}.npz: {k}[0]")


@pytest.mark.parametrize("name", list(pg.CASES))
def test_case_is_off_every_branch_point_and_fp32_resolves_it(name):
    case = pg.build(name)
    hy, mb, I = case["hyper"], case["mb"], case["I"]
    # the batch itself: mb distinct rows, NaN everywhere else, distinct tracker cells, valid actions in every row
    idx = case["idx"].astype(np.int64)
    assert len(set(idx.tolist())) == mb and case["n_rows"] == mb + pg.EXTRA_ROWS
    out = np.setdiff1d(np.arange(case["n_rows"]), idx)
    for k in ("obs", "adv", "ret", "v_s", "logp"):
        col = case["batch"][k]
        assert bool(torch.isnan(col[out]).all()) and bool(torch.isfinite(col[idx]).all()), k
    act = case["batch"]["act"]
    assert int(act.min()) >= 0 and int(act.max()) < I and not act[out].any()
    cells = case["b_t"].astype(np.int64) * case["n_env"] + case["b_env"]
    assert len(set(cells.tolist())) == case["n_rows"] and cells.max() < case["n_env"] * (case["max_turn"] + 1)
    last, chunk0 = pg.forced_actions(I)
    taken = case["cols"][1]
    assert int((taken == last).sum()) >= mb // 3 and (mb < 2 or int((taken == chunk0).sum()) >= (mb - 1) // 3)
    # margins: every row, none excluded
    t = pg._terms64(case["p"], case["cols"], hy)
    m = {k: float(v.min()) for k, v in pg.margins(t, hy).items()}
    relu = float(torch.minimum(t["h1p"].abs().min(), t["h2p"].abs().min()))
    room = float((1 - t["p_a"]).min())
    cl = pg.classes(t, hy)
    ref = pg.reference(name)
    print(f"{name}: moved {case['moved']} rows; margins {({k: float('%.2e' % v) for k, v in m.items()})}; min |pre-activation| {relu:.2e}; "
          f"min 1 - p_a {room:.2e}; classes {cl}; e32 {({k: float('%.2e' % v) for k, v in ref['e32'].items()})}")
    for k, v in m.items():
        assert v >= pg.MARGIN, (k, v)
    assert relu >= pg.RELU_MARGIN and room >= pg.UPPER_CLAMP_ROOM
    if mb >= pg.CLASS_FROM_MB:
        for k, v in cl.items():
            assert v >= pg.MIN_CLASS_ROWS, (k, cl)
    for k, v in ref["e32"].items():
        assert v <= E32_MAX, (k, v)
    assert all(np.isfinite(x) for x in ref["loss"])


@pytest.mark.parametrize("name", list(pg.SHARDS))
def test_shares_add_up_to_the_minibatch(name):
    """The parts of the global loss the data-parallel ranks hold sum to it, gradient by gradient, and fp32 resolves each part."""
    whole = pg.reference(name)
    lo, total, dobs = 0, None, []
    for n in pg.SHARDS[name]:
        part = pg.reference(name, (lo, lo + n))
        lo += n
        for k, v in part["e32"].items():
            assert v <= E32_MAX, (name, n, k, v)
        dobs.append(part["g64"]["obs"])
        total = {k: (part["g64"][k] if total is None else total[k] + part["g64"][k]) for k in pg.FLAT_ORDER}
    assert lo == pg.build(name)["mb"]
    for k in pg.FLAT_ORDER:
        assert pg.rel(total[k], whole["g64"][k]) < 1e-12, k
    assert pg.rel(torch.cat(dobs), whole["g64"]["obs"]) < 1e-12


def test_every_case_has_padded_rows_and_a_mean_over_them_misses_the_bar():
    """1 / n_pad where 1 / mb is meant scales every gradient by mb / n_pad: no row count is a multiple of the 32-row tile, and the smallest
    relative error that gives, 1 / 2048 at 2047 rows, is 12 x the largest bar a case can have (4 x E32_MAX)."""
    for name, c in pg.CASES.items():
        n_pad = -(-c["mb"] // 32) * 32
        assert n_pad > c["mb"] and (n_pad - c["mb"]) / n_pad > 10 * pg.grad_bar(E32_MAX), name
    assert any(-(-c["mb"] // 32) * 32 == 2048 for c in pg.CASES.values()) and any(c["mb"] > 2048 for c in pg.CASES.values())      # both sides of the kernel switch


@pytest.mark.parametrize("name,tensor", [(n, "wc" if "novclip" in n else "wa") for n in pg.OPTIONS if pg.OPTIONS[n]["rows_kernel"] is None])
def test_an_option_taken_the_default_way_misses_the_bar(name, tensor):
    """Each option case separates its option from the default: the float64 gradient of the loss with the option left at HYPER's value is
    outside the bar the device is held to (the critic head for the value clip, the actor head for the advantage and the dual clip)."""
    case, ref = pg.build(name), pg.reference(name)
    hy = dict(case["hyper"], norm_adv=True, value_clip=True, dual_clip=None)
    assert hy != case["hyper"]
    _, g = pg.loss_and_grads(case["p"], case["cols"], hy, torch.float64)
    err = pg.rel(g[tensor], ref["g64"][tensor])
    print(f"{name}: {tensor} with the default options: relative difference {err:.2e}, bar {pg.grad_bar(ref['e32'][tensor]):.2e}")
    assert err > 100 * pg.grad_bar(ref["e32"][tensor])


# ---- the clip + Adam comparator -------------------------------------------------------------------------------------------------------
def _emulate(p0, m0, v0, g, I, k, max_grad_norm, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, trunk_pow=2, trunk_sub=2, trunk_twice_in_norm=True):
    """adam_next_kernel's element update (adam_elem, csrc/ppo.hip) in numpy fp32, one rounding per operation, the norm summed in float64."""
    f = np.float32
    n_trunk = pg.H * pg.S + pg.H + pg.H * pg.H + pg.H
    g64 = g.astype(np.float64)
    sq = (2.0 if trunk_twice_in_norm else 1.0) * np.sum(g64[:n_trunk] ** 2) + np.sum(g64[n_trunk:] ** 2)
    c = f(min(f(1.0), f(max_grad_norm) / (f(np.sqrt(sq)) + f(1e-6)))) if max_grad_norm else f(1.0)
    p, m, v = p0.copy(), m0.copy(), v0.copy()
    for sl, pw, steps in ((slice(0, n_trunk), trunk_pow, [trunk_sub * k + 1 + q for q in range(trunk_sub)]), (slice(n_trunk, len(g)), 1, [k + 1])):
        gi = g[sl].copy()
        for _ in range(pw):
            gi = gi * c
        for t in steps:
            ss = f(np.float64(f(lr)) / (1.0 - np.float64(f(b1)) ** t))
            rb2 = f(1.0 / np.sqrt(1.0 - np.float64(f(b2)) ** t))
            m[sl] = m[sl] + (f(1.0) - f(b1)) * (gi - m[sl])
            v[sl] = v[sl] * f(b2) + (f(1.0) - f(b2)) * gi * gi
            p[sl] = p[sl] - ss * (m[sl] * (f(1.0) / (np.sqrt(v[sl]) * rb2 + f(eps))))
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


@pytest.mark.parametrize("max_grad_norm", [0.5, 1e3])
def test_clip_adam_comparator_accepts_the_fp32_update_and_rejects_the_mistakes(max_grad_norm):
    I, k = 224, 7
    rng = np.random.RandomState(77)
    P = sum(int(np.prod(s)) for s in pg.shapes_of(I).values())
    g = (rng.standard_normal(P) * 0.05 * np.exp(rng.uniform(-8, 0, P))).astype(np.float32)      # magnitudes over several decades, as head gradients have
    p0 = (rng.standard_normal(P) * 0.2).astype(np.float32)
    m0 = (rng.standard_normal(P) * 1e-3).astype(np.float32)
    v0 = (rng.uniform(0, 1, P) * 1e-5).astype(np.float32)
    d = np.float64

    def check(out):
        return pg.check_clip_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), out[1].astype(d), out[2].astype(d), out[0].astype(d), I, k,
                                  max_grad_norm, what="emulation")
    coef, used = check(_emulate(p0, m0, v0, g, I, k, max_grad_norm))
    print(f"max_grad_norm {max_grad_norm}: coef {coef:.4f}, share of each bar used {({a: float('%.3f' % b) for a, b in used.items()})}")
    assert (coef < 1.0) == (max_grad_norm == 0.5)
    wrong = [dict(trunk_sub=1)]                                                  # one Adam step on the trunk instead of two
    if max_grad_norm == 0.5:
        wrong += [dict(trunk_pow=1), dict(trunk_twice_in_norm=False)]           # the coefficient once on the trunk; the trunk once in the norm
    for kw in wrong:
        with pytest.raises(AssertionError):
            check(_emulate(p0, m0, v0, g, I, k, max_grad_norm, **kw))
    # a parameter 25 ulp off
    p, m, v = _emulate(p0, m0, v0, g, I, k, max_grad_norm)
    with pytest.raises(AssertionError):
        check((p * np.float32(1.0 + 3e-6), m, v))
