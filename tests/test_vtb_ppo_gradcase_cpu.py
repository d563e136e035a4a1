"""CPU: what tests/test_gpu_vtb_ppo_grads.py stands on (tests/vtbppogradcase.py); no library needed.

1. The reference is the project's: vtb_host.policy_rows in fp32 gives what the ActorProb / Critic modules and Independent(Normal) give, and
   ppo_terms / ppo_loss in float64 give core.host_rl.ppo_objective's four terms (up to its rounding of the ratio to float32).
2. Every case keeps every row and position KINK away from every branch point (no row is left out), populates the branch classes it is meant
   to, and is one on which a plain fp32 evaluation agrees with float64 to 1e-5 in every tensor -- so the bar the device is held to
   (ppogradcase.grad_bar: 4 x the fp32 evaluation's error, at least 3e-6) never exceeds 4e-5.
3. The Adam recurrence of gradcase reproduces torch.optim.Adam in float64, and the clip + Adam comparator accepts an fp32 emulation of
   vtb_learn_adam_kernel's element update and rejects the mistakes it is there for."""
import numpy as np
import pytest
import torch

import vtbppogradcase as vc
from cirs_hip import vtb_host

E32_MAX = 1e-5


@pytest.mark.parametrize("name", ["ragged-small", "csigma-h128-S7", "unbounded-h3-S128"])
def test_policy_rows_restate_the_modules(name):
    from torch.distributions import Independent, Normal
    case = vc.build(name)
    _, pimg = vc.images(case["tracker"], case["actor"], case["critic"])
    st = torch.randn(9, case["c"]["dim_state"], generator=torch.Generator().manual_seed(1))
    act = torch.randn(9, vc.ACTION_DIM, generator=torch.Generator().manual_seed(2)) * 0.1
    with torch.no_grad():
        got = vtb_host.policy_rows({k: v.detach() for k, v in pimg.items()}, st, act, 1.0, case["c"]["unbounded"])
        (mu, sigma), _ = case["actor"](st)
        dist = Independent(Normal(mu, sigma), 1)
        torch.testing.assert_close(got["mu"], mu, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(got["sigma"], sigma, rtol=1e-6, atol=0)
        torch.testing.assert_close(got["logp"], dist.log_prob(act), rtol=2e-6, atol=1e-5)
        torch.testing.assert_close(got["ent"], dist.entropy(), rtol=1e-6, atol=1e-5)
        torch.testing.assert_close(got["value"], case["critic"](st).flatten(), rtol=1e-6, atol=1e-6)
        z = vtb_host.hidden_preactivations({k: v.detach() for k, v in pimg.items()}, st)
    assert [tuple(x.shape) for x in z] == [(9, w) for w in case["c"]["hidden"]]


@pytest.mark.parametrize("name", ["rows63", "rows64-plain", "rows65-dual", "rows129-split"])
def test_ppo_terms_restate_the_host_objective(name):
    from core.host_rl import ppo_objective
    case = vc.build(name)
    for mb in case["mbs"]:
        t, idx = vc._terms_of(case, case["cols"], mb)
        got = vc.ppo_loss(t, case["h"])
        u = case["uniq"][idx]
        rq, col = case["row64"], lambda k: case["cols"][k].double()[idx]      # noqa: E731
        want = ppo_objective(rq["logp"][u], col("logp_old"), col("adv"), rq["value"][u], col("v_s"), col("ret"), rq["ent"][u], case["h"])
        np.testing.assert_allclose([float(x) for x in got], [float(x) for x in want], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name", list(vc.CASES))
def test_case_is_off_every_branch_point_and_fp32_resolves_it(name):
    case = vc.build(name)
    c = case["c"]
    info = vc.check_case(case)
    ref = vc.reference(name)
    worst = max(ref["e32"], key=ref["e32"].get)
    print(f"{name}: {case['n']} rows, minibatches {[b - a for _, (a, b) in case['mbs']]}; moved {info['moved']}; margins "
          f"{({k: float('%.2e' % v) for k, v in info['margins'].items()})}; min |pre-activation| {info['relu']}; classes {info['classes']}; "
          f"sigma {info['sigma']}; largest e32 {ref['e32'][worst]:.2e} ({worst})")
    # the trajectory: the lengths asked for, an unfinished episode only at full length, duplicates and omissions where planned
    lens, T = case["traj"]["lens"], case["T"]
    assert tuple(lens) == c["lens"] and lens.max() <= T and all(lens[e] == T for e in c["unfinished"])
    assert case["traj"]["done"].sum() == len(lens) - len(c["unfinished"])
    counts = np.bincount(case["uniq"].numpy(), minlength=int(lens.sum()))
    if c["n_draw"]:
        assert case["n"] == c["n_draw"] and (counts == 0).sum() >= 2 and (counts >= 3).sum() >= 2
    else:
        assert (counts == 1).all()
    for p in case["perms"]:
        assert sorted(p.tolist()) == list(range(case["n"]))
    assert len(case["perms"]) == c["repeat"] and (c["repeat"] == 1 or not np.array_equal(case["perms"][0], case["perms"][1]))
    for k, v in ref["e32"].items():
        assert v <= E32_MAX, (k, v)
    assert np.isfinite(ref["losses"]).all() and ref["losses"].shape == (len(case["mbs"]), 4)
    assert all(bool(torch.isfinite(g).all()) for g in ref["g64"].values())


def test_the_cases_sit_on_the_kernels_constants():
    n = {k: vc.build(k)["n"] for k in ("one-row", "ragged-small", "rows63", "rows64-plain", "rows65-dual", "rows129-drop", "rows129-split", "dup70-of-40")}
    assert n == {"one-row": 1, "ragged-small": 7, "rows63": 63, "rows64-plain": 64, "rows65-dual": 65, "rows129-drop": 129, "rows129-split": 129,
                 "dup70-of-40": 70}
    assert [b - a for _, (a, b) in vc.build("rows129-split")["mbs"]] == [64, 65, 64, 65]
    # exact redraw: workgroups per env (make_layout of csrc/vtb_learn.hip: 1024 / B clamped to 1 .. 8) and calls per workgroup
    for name, groups in (("redraw-small", 8), ("redraw-B130", 7), ("redraw-B200", 5)):
        c = vc.CASES[name]
        B = len(c["lens"])
        assert min(8, max(1, 1024 // B)) == groups and c["redraw"] and c["dropout"] > 0
    assert vc.CASES["redraw-B200"]["T"] > 5 and max(vc.CASES["redraw-B200"]["lens"]) == 6      # calls 0 and 5 of a full episode share workgroup 0
    assert len(vc.build("redraw-B130")["mbs"]) > 2


def test_a_gradient_that_kept_the_first_pass_misses_the_bar():
    """repeat = 2 with two different permutations: the tracker gradient of both passes is about twice the last pass's."""
    from ppogradcase import grad_bar
    case, ref = vc.build("rows129-split"), vc.reference("rows129-split")
    _, gt, _ = vc.evaluate(case, torch.float64, passes=(0, 1))
    for k in ("dec_w", "user_w"):
        assert vc.err_of(gt[k], ref["g64"][k]) > 100 * grad_bar(E32_MAX), k


# ---- the Adam recurrence and the comparator -----------------------------------------------------------------------------------------
def test_float64_recurrence_reproduces_torch_adam():
    from gradcase import adam_constants, adam_moments, adam_update
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    g = torch.Generator().manual_seed(5)
    p = torch.randn(37, dtype=torch.float64, generator=g).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    rp, rm, rv = p.detach().numpy().copy(), np.zeros(37), np.zeros(37)
    for t in range(1, 6):
        grad = torch.randn(37, dtype=torch.float64, generator=g)
        p.grad = grad.clone()
        opt.step()
        b1, b2, e, ss, bc2s = adam_constants(t, lr, betas, eps, as_device=False)
        rm, rv = adam_moments(rm, rv, grad.numpy(), b1, b2)
        rp, _ = adam_update(rp, rm, rv, ss, bc2s, e)
        np.testing.assert_allclose(rp, p.detach().numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(rm, opt.state[p]["exp_avg"].numpy(), rtol=1e-13, atol=1e-18)
        np.testing.assert_allclose(rv, opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-20)


def _emulate(p0, m0, v0, g, n_trunk, k, max_grad_norm, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, trunk_pow=2, trunk_sub=2, trunk_twice_in_norm=True):
    """vtb_learn_adam_kernel's element update (adam_one, csrc/vtb_learn.hip) in numpy fp32, one rounding per operation and one for the fused
    second moment, the norm summed in float64."""
    f = np.float32
    g64 = g.astype(np.float64)
    sq = (2.0 if trunk_twice_in_norm else 1.0) * np.sum(g64[:n_trunk] ** 2) + np.sum(g64[n_trunk:] ** 2)
    c = f(min(f(1.0), f(max_grad_norm) / (f(np.sqrt(sq)) + f(1e-6))))
    p, m, v = p0.copy(), m0.copy(), v0.copy()
    for sl, pw, steps in ((slice(0, n_trunk), trunk_pow, [trunk_sub * k + 1 + q for q in range(trunk_sub)]), (slice(n_trunk, len(g)), 1, [k + 1])):
        gi = g[sl].copy()
        for _ in range(pw):
            gi = gi * c
        for t in steps:
            ss = f(np.float64(f(lr)) / (1.0 - np.float64(f(b1)) ** t))
            bc2s = f(np.sqrt(1.0 - np.float64(f(b2)) ** t))
            m[sl] = m[sl] + (f(1.0) - f(b1)) * (gi - m[sl])
            v[sl] = vtb_host.fmaf(v[sl], f(b2), (f(1.0) - f(b2)) * gi * gi)
            p[sl] = p[sl] + (-ss) * (m[sl] / (np.sqrt(v[sl]) / bc2s + f(eps)))
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


@pytest.mark.parametrize("max_grad_norm", [0.5, 1e3])
def test_clip_adam_comparator_accepts_the_fp32_update_and_rejects_the_mistakes(max_grad_norm):
    n_trunk, P, k = 5500, 9000, vc.ADAM_K
    rng = np.random.RandomState(77)
    g = (rng.standard_normal(P) * 0.05 * np.exp(rng.uniform(-8, 0, P))).astype(np.float32)      # magnitudes over several decades
    p0 = (rng.standard_normal(P) * 0.2).astype(np.float32)
    m0 = (rng.standard_normal(P) * 1e-3).astype(np.float32)
    v0 = (rng.uniform(0, 1, P) * 1e-5).astype(np.float32)
    d = np.float64

    def check(out):
        return vc.check_clip_adam(p0.astype(d), m0.astype(d), v0.astype(d), g.astype(d), out[1].astype(d), out[2].astype(d), out[0].astype(d),
                                  n_trunk, k, max_grad_norm, 1e-3, (0.9, 0.999), 1e-8, what="emulation")
    norm, coef, used = check(_emulate(p0, m0, v0, g, n_trunk, k, max_grad_norm))
    print(f"max_grad_norm {max_grad_norm}: norm {norm:.4f} coef {coef:.4f}, share of each bar used {({a: float('%.3f' % b) for a, b in used.items()})}")
    assert (coef < 1.0) == (max_grad_norm == 0.5)
    wrong = [dict(trunk_sub=1)]                                                  # one Adam step on the trunk instead of two
    if max_grad_norm == 0.5:
        wrong += [dict(trunk_pow=1), dict(trunk_twice_in_norm=False)]           # the coefficient once on the trunk; the trunk once in the norm
    for kw in wrong:
        with pytest.raises(AssertionError):
            check(_emulate(p0, m0, v0, g, n_trunk, k, max_grad_norm, **kw))
    p, m, v = _emulate(p0, m0, v0, g, n_trunk, k, max_grad_norm)
    with pytest.raises(AssertionError):
        check((p * np.float32(1.0 + 3e-6), m, v))      # a parameter 25 ulp off


@pytest.mark.parametrize("name", vc.ADAM_CASES)
def test_the_clip_binds_at_half_and_not_at_a_thousand(name):
    """From the float64 gradient, not the device's: the norm with the trunk counted twice is well above 0.5 and far below 1e3."""
    case, ref = vc.build(name), vc.reference(name)
    assert len(case["mbs"]) == 1      # one minibatch: the run with lr = 0 and the Adam run see the same gradient bits
    g = np.concatenate([ref["g64"][k].reshape(-1).numpy() for k in ref["policy_names"]])
    norm, coef = vc.clip_coef(g, vc.n_trunk_floats(vc.images(case["tracker"], case["actor"], case["critic"])[1]), 0.5)
    print(f"{name}: norm {norm:.4f} coef at 0.5 {coef:.4f}")
    assert 0.6 < norm < 500.0
