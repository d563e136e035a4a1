"""GPU: the VirtualTaobao PPO update (csrc/vtb_learn.hip: cirs_vtb_learn_prepare / _update and their _redraw twins) against float64 autograd
at edge shapes, through cirs_hip.vtb_learn.DeviceVtbLearner on the fabricated trajectories of tests/vtbppogradcase.py -- what the host-parity
tests of tests/test_gpu_vtb_learn.py cannot see, since one Adam step lr g / (|g| + eps) hides the gradient's magnitude.

The device hands out no gradient buffer: it is read from the optimiser state.  Fresh optimisers with betas = (0, 0.999) and lr = 0 leave
exp_avg = the raw gradient (the policy's of the last minibatch, the tracker's summed over the last pass) and every parameter bit for bit.

a. every tensor of the tracker and policy images: max |got - want| / max |want| within ppogradcase.grad_bar of the error a float32 torch
   evaluation of the same restatement shows (tests/test_vtb_ppo_gradcase_cpu.py holds that under 1e-5, so the bar never exceeds 4e-5);
b. every minibatch's row of the loss record against the float64 terms;
c. clip_grad_norm_ + Adam as a float64 recurrence fed the device's own gradient (trunk counted twice in the norm, coefficient squared and two
   sub-steps on the trunk, one tracker step), with a coefficient that binds and one that does not, from preloaded moments and step counts;
d. after the lr = 0 run: parameters bit-equal, the three step counts, nothing NaN.
The dropout masks of the reference are the numpy Philox's; they are held to cirs_vtb_rollout_masks bit for bit here.

Largest shares of the gradient bar used on an MI355X (device error / bar, the tensor it fell on):
  one-row              0.145  trunk1_w         device 4.35e-07 / e32 4.99e-07 / bar 3.00e-06
  ragged-small         0.206  trunk1_w         device 1.17e-06 / e32 1.42e-06 / bar 5.69e-06
  rows63               0.597  layer0.norm2_w   device 1.94e-06 / e32 8.10e-07 / bar 3.24e-06
  rows64-plain         0.481  user_b           device 2.00e-06 / e32 1.04e-06 / bar 4.15e-06
  rows65-dual          0.705  sigma_param      device 2.90e-06 / e32 1.03e-06 / bar 4.12e-06
  rows129-drop         0.358  trunk0_b         device 4.39e-06 / e32 3.06e-06 / bar 1.23e-05
  rows129-split        0.334  layer1.in_b      device 2.02e-06 / e32 1.51e-06 / bar 6.04e-06
  dup70-of-40          0.305  gate_b           device 1.28e-06 / e32 1.05e-06 / bar 4.19e-06
  csigma-h128-S7       0.726  mu_w             device 5.57e-06 / e32 1.92e-06 / bar 7.67e-06
  unbounded-h3-S128    0.565  layer1.in_w      device 1.82e-06 / e32 8.05e-07 / bar 3.22e-06
  nhead27-drop         0.614  gate_b           device 2.82e-06 / e32 1.15e-06 / bar 4.59e-06
  redraw-small         0.818  layer1.lin1_b    device 2.45e-06 / e32 6.54e-07 / bar 3.00e-06
  redraw-B130          0.634  gate_w           device 1.90e-06 / e32 6.84e-07 / bar 3.00e-06
  redraw-B200          0.524  layer1.norm2_b   device 1.72e-06 / e32 8.21e-07 / bar 3.29e-06
Largest share of each clip + Adam bar used over the six runs of c: trunk m 0.106, v 0.099, p 0.466; heads m 0.116, v 0.154, p 0.488;
tracker m 0.120, v 0.125, p 0.494 (p: the half ulp of the parameter's own rounding against a bar of one ulp per rounding)."""
import functools

import numpy as np
import pytest
import torch

import vtbppogradcase as vc
from conftest import close
from ppogradcase import grad_bar

pytestmark = pytest.mark.gpu

LOSS_RTOL, LOSS_ATOL = 2e-5, 2e-6      # tests/test_gpu_ppo_step_grads.py's


def _params(tracker, actor, critic):
    timg, pimg = vc.images(tracker, actor, critic)
    return list(timg), list(timg.values()), list(pimg), list(pimg.values())


def _library_masks(c, n_pos, env0=0):
    """vc.masks_for from cirs_vtb_rollout_masks."""
    from cirs_hip import abi
    from cirs_hip.vtb_host import DROP_ATTN, DROP_FF, DROP_POS, DROP_RES1, DROP_RES2
    lib, B = abi.lib(), len(c["lens"])

    def one(layer, site, n_elem):
        out = torch.empty((B, n_pos, n_elem), dtype=torch.float32, device="cuda")
        abi.check(lib.cirs_vtb_rollout_masks(vc.DROP_SEED, float(c["dropout"]), vc.DROP_BASE + env0, B, 0, n_pos, layer, site, n_elem, out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "cirs_vtb_rollout_masks")
        return out.cpu()
    m = {"pos": one(0, DROP_POS, vc.ACTION_DIM)}
    for l in range(c["nlayers"]):
        for site, n_elem in ((DROP_ATTN, n_pos * c["nhead"]), (DROP_RES1, vc.ACTION_DIM), (DROP_FF, c["d_hid"]), (DROP_RES2, vc.ACTION_DIM)):
            m[(l, site)] = one(l, site, n_elem)
    return m


@functools.lru_cache(maxsize=None)
def _gradient_run(name):
    """The update with lr = 0 and beta1 = 0 from fresh optimisers, once per case.  -> dict(losses, g {name: float64 tensor} over both images,
    the parameters before and after, the optimisers)."""
    case = vc.build(name)
    policy, tracker, actor, critic = vc.make_policy(case, lr=0.0, betas=(0.0, 0.999), max_grad_norm=None)
    assert vc.hyper_of(case["c"]["hyper"]) == policy.hyper
    tn, tp, pn, pp = _params(tracker, actor, critic)
    before = [p.detach().clone() for p in tp + pp]
    losses = vc.run_update(case, policy, tracker, actor, critic)
    torch.cuda.synchronize()
    g = {k: policy.optim[1].state[p]["exp_avg"].detach().double().clone() for k, p in zip(tn, tp)}
    g.update({k: policy.optim[0].state[p]["exp_avg"].detach().double().clone() for k, p in zip(pn, pp)})
    return dict(losses=losses, g=g, before=before, after=[p.detach().clone() for p in tp + pp], policy=policy, names=(tn, pn), params=(tp, pp))


@pytest.mark.parametrize("name", [k for k, c in vc.CASES.items() if c["dropout"] > 0])
def test_reference_masks_are_the_librarys(name):
    c = vc.CASES[name]
    B, T = len(c["lens"]), c["T"]
    calls = [(T + 1, 0)] + ([(k + 1, k * B) for k in (1, T)] if c["redraw"] else [])
    for n_pos, env0 in calls:
        want, got = vc.masks_for(c, n_pos, env0), _library_masks(c, n_pos, env0)
        assert list(want) == list(got)
        for k in want:
            assert torch.equal(want[k], got[k]), (name, n_pos, env0, k)


@pytest.mark.parametrize("name", list(vc.CASES))
def test_update_gradient_and_losses_against_float64(name):
    case, ref = vc.build(name), vc.reference(name)
    vc.check_case(case)
    run = _gradient_run(name)
    tn, pn = run["names"]
    tp, pp = run["params"]
    # d. untouched state
    for nm, a, b in zip(tn + pn, run["before"], run["after"]):
        assert torch.equal(a, b), f"{name}: {nm} moved under lr = 0"
    n_mb = len(case["mbs"])
    n_trunk = sum(1 for k in pn if k.startswith("trunk"))
    opt_p, opt_t = run["policy"].optim
    assert [int(float(opt_p.state[p]["step"])) for p in pp] == [2 * n_mb] * n_trunk + [n_mb] * (len(pp) - n_trunk)
    assert [int(float(opt_t.state[p]["step"])) for p in tp] == [1] * len(tp)
    for opt in (opt_p, opt_t):
        for st in opt.state.values():
            assert bool(torch.isfinite(st["exp_avg"]).all()) and bool(torch.isfinite(st["exp_avg_sq"]).all()), f"{name}: NaN in the moments"
    # a. gradients
    assert list(ref["g64"]) == tn + pn
    used, line = {}, []
    for k, want in ref["g64"].items():
        e_dev, e32 = vc.err_of(run["g"][k], want), ref["e32"][k]
        bar = grad_bar(e32)
        used[k] = e_dev / bar
        line.append(f"{k} {e_dev:.2e} / {e32:.2e} / {bar:.2e}")
    worst = max(used, key=used.get)
    print(f"{name}: device / e32 / bar: " + "; ".join(line))
    print(f"{name}: largest share of the bar used {used[worst]:.3f} ({worst})")
    # b. the loss record
    print(f"{name}: loss record device {run['losses'].tolist()} float64 {ref['losses'].tolist()}")
    for k, v in used.items():
        assert v <= 1.0, (name, k, v)
    close(run["losses"], ref["losses"], LOSS_RTOL, LOSS_ATOL, f"vtb ppo grads {name}: loss, clip, vf, ent per minibatch")
    close(np.array(list(used.values())), np.zeros(len(used)), 0, 1.0, f"vtb ppo grads {name}: share of the bar used {list(used)}")


def _preload(opt, params, steps, rng):
    for p, s in zip(params, steps):
        opt.state[p] = dict(step=torch.tensor(float(s)), exp_avg=torch.as_tensor((rng.standard_normal(tuple(p.shape)) * 1e-3).astype(np.float32)),
                            exp_avg_sq=torch.as_tensor((rng.uniform(1e-3, 1.0, tuple(p.shape)) * 1e-5).astype(np.float32)))


@pytest.mark.parametrize("max_grad_norm", [0.5, 1e3])
@pytest.mark.parametrize("name", vc.ADAM_CASES)
def test_clip_and_adam_follow_the_float64_recurrence_from_the_device_gradient(name, max_grad_norm):
    from gradcase import check_adam
    case = vc.build(name)
    assert len(case["mbs"]) == 1
    run = _gradient_run(name)
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    policy, tracker, actor, critic = vc.make_policy(case, lr=lr, betas=betas, max_grad_norm=max_grad_norm)
    tn, tp, pn, pp = _params(tracker, actor, critic)
    n_trunk_t = sum(1 for k in pn if k.startswith("trunk"))
    n_trunk = vc.n_trunk_floats(dict(zip(pn, pp)))
    rng = np.random.RandomState(case["n"])
    opt_p, opt_t = policy.optim
    k, kt = vc.ADAM_K, vc.ADAM_KT
    _preload(opt_p, pp, [2 * k] * n_trunk_t + [k] * (len(pp) - n_trunk_t), rng)
    _preload(opt_t, tp, [kt] * len(tp), rng)
    flat = lambda names: np.concatenate([run["g"][q].reshape(-1).numpy() for q in names])      # noqa: E731
    g_p, g_t = flat(pn), flat(tn)
    p0, m0, v0 = vc.flat_state(pp, opt_p), vc.flat_state(pp, opt_p, "exp_avg"), vc.flat_state(pp, opt_p, "exp_avg_sq")
    t0, tm0, tv0 = vc.flat_state(tp, opt_t), vc.flat_state(tp, opt_t, "exp_avg"), vc.flat_state(tp, opt_t, "exp_avg_sq")
    vc.run_update(case, policy, tracker, actor, critic)
    torch.cuda.synchronize()
    p1, m1, v1 = vc.flat_state(pp, opt_p), vc.flat_state(pp, opt_p, "exp_avg"), vc.flat_state(pp, opt_p, "exp_avg_sq")
    t1, tm1, tv1 = vc.flat_state(tp, opt_t), vc.flat_state(tp, opt_t, "exp_avg"), vc.flat_state(tp, opt_t, "exp_avg_sq")
    assert all(np.isfinite(z).all() for z in (p1, m1, v1, t1, tm1, tv1))
    assert [int(float(opt_p.state[p]["step"])) for p in pp] == [2 * (k + 1)] * n_trunk_t + [k + 1] * (len(pp) - n_trunk_t)
    assert [int(float(opt_t.state[p]["step"])) for p in tp] == [kt + 1] * len(tp)
    what = f"{name} max_grad_norm {max_grad_norm}"
    norm, coef, used = vc.check_clip_adam(p0, m0, v0, g_p, m1, v1, p1, n_trunk, k, max_grad_norm, lr, betas, eps, what=what)
    used_t = check_adam(t0, tm0, tv0, g_t, tm1, tv1, t1, kt + 1, lr, betas, eps, what=what + " (tracker)")
    used.update(dict(zip(("tracker_m", "tracker_v", "tracker_p"), used_t)))
    print(f"{what}: norm {norm:.4f} coef {coef:.6f}; share of each bar used {({a: float('%.3f' % b) for a, b in used.items()})}")
    assert (coef < 1.0) == (max_grad_norm == 0.5), f"{what}: the clip must bind at 0.5 and only there (norm {norm})"
    close(np.array(list(used.values())), np.zeros(len(used)), 0, 1.0, f"vtb ppo grads {what}: share of the Adam bars used {list(used)}")
