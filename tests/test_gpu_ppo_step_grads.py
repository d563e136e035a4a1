"""GPU: the PPO minibatch step (csrc/ppo.hip, trunk_adv_kernel .. adam_next_kernel) against float64 autograd of the loss at ragged row counts,
through an index list, with every loss option -- what the bit-identity tests of the step cannot see, since they compare the device with itself.

a. the raw gradient of the eight tensors, d loss / d obs scattered to the tracker-gradient tensor, and the four loss terms, per case of
   tests/ppogradcase.py (row counts on the step's own tile / workgroup / kernel-switch constants; 37 rows of NaN around the minibatch's rows);
b. the data-parallel split: every rank's gradient is its rows' share of the GLOBAL loss, the shares sum to the single-device gradient;
c. clip_grad_norm_ + Adam as a float64 recurrence fed the device's own gradient (trunk counted twice in the norm, coefficient squared and two
   sub-steps on the trunk), with a coefficient that binds and one that does not.

The gradient rule is test_gpu_head_precision's: relative error at most 4 x what a float32 torch evaluation loses against float64, at least 3e-6
(tests/test_ppo_gradcase_cpu.py holds that evaluation's error under 1e-5, so the bar never exceeds 4e-5)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppogradcase as pg
from conftest import close

pytestmark = pytest.mark.gpu

FILL = 7.0             # the tracker-gradient tensor before the step: the kernels store their rows, they do not add
LOSS_RTOL, LOSS_ATOL = 2e-5, 2e-6      # test_learner_benchmark_workload_1024_envs' tolerance


def _env(monkeypatch, case):
    if case["rows_kernel"] is None:
        monkeypatch.delenv("CIRS_PPO_ROWS_KERNEL", raising=False)
    else:
        monkeypatch.setenv("CIRS_PPO_ROWS_KERNEL", case["rows_kernel"])      # (read per call)


def _phase1(case, lo, hi):
    """Phase 1 of rows lo .. hi - 1 of the index list as one rank's shard of the whole list, on a fresh learner, every byte of the workspace 0xff,
    the gradient NaN and the tracker gradient FILL beforehand.  -> (learner, flat gradient + loss partials [P + 4], dobs [cells, S]) on the host."""
    ln = pg.make_learner(case)
    idx_g = torch.as_tensor(case["idx"]).cuda()
    idx_l = idx_g[lo:hi].clone()
    ln.workspace(max(hi - lo, 2)).fill_(255)      # fp32: NaN, int32: -1 -- whatever a kernel reads without anybody having written it shows
    ln.grads[:ln.P + 4].fill_(float("nan"))
    ln.dobs.fill_(FILL)
    slot = torch.zeros(4, dtype=torch.float32, device="cuda")
    ln.mb_phase1(idx_l, idx_g, True, slot)
    torch.cuda.synchronize()
    return ln, ln.grads[:ln.P + 4].double().cpu(), ln.dobs.double().cpu().view(-1, pg.S)


def _check_grads(case, flat, dobs, ref, lo, hi, what):
    """The gradient rule on the eight tensors and on the rows of d obs; every other row of dobs untouched.  -> {name: share of its bar used}."""
    I = case["I"]
    assert not bool(torch.isnan(flat).any()), f"{what}: NaN in the gradient"
    got = dict(pg.split_flat(flat[:-4], I))
    cells = case["b_t"].astype(np.int64) * case["n_env"] + case["b_env"]
    mine = torch.as_tensor(cells[case["idx"][lo:hi].astype(np.int64)])
    got["obs"] = dobs[mine]
    others = torch.ones(dobs.shape[0], dtype=torch.bool)
    others[mine] = False
    assert bool((dobs[others] == FILL).all()), f"{what}: {int((dobs[others] != FILL).any(1).sum())} rows of dobs outside the shard were written"
    used, line = {}, []
    for k, want in ref["g64"].items():
        e_dev, e32 = pg.rel(got[k], want), ref["e32"][k]
        bar = pg.grad_bar(e32)
        line.append(f"{k} {e_dev:.2e} / {e32:.2e} / {bar:.2e}")
        used[k] = e_dev / bar
    print(f"{what}: device / e32 / bar: " + "; ".join(line))
    for k, v in used.items():
        assert v <= 1.0, (what, k, v)
    hb = pg.head_bar(ref["e32"])
    for k in ("wa", "ba"):
        assert pg.rel(got[k], ref["g64"][k]) < hb, (what, k, hb)
    return used, got


@pytest.mark.parametrize("name", list(pg.CASES))
def test_step_gradient_dobs_and_losses_against_float64(name, monkeypatch):
    from cirs_hip import abi
    case, ref = pg.build(name), pg.reference(name)
    _env(monkeypatch, case)
    mb = case["mb"]
    ln, flat, dobs = _phase1(case, 0, mb)
    used, _ = _check_grads(case, flat, dobs, ref, 0, mb, name)
    # the four loss terms from one whole step on a second, identical learner
    ln2 = pg.make_learner(case)
    idx = torch.as_tensor(case["idx"]).cuda()
    ws = ln2.workspace(mb)
    ws.fill_(255)
    losses = torch.zeros(4, dtype=torch.float32, device="cuda")
    abi.check(ln2._lib.cirs_ppo_minibatch(C.byref(ln2.cfg), ln2.params.data_ptr(), ln2.grads.data_ptr(), ln2.adam_m.data_ptr(), ln2.adam_v.data_ptr(),
                                          ln2.opt_step, C.byref(ln2.batch), idx.data_ptr(), mb, None, ln2.n_env, losses.data_ptr(), ws.data_ptr(),
                                          ws.numel(), ln2._stream()), "cirs_ppo_minibatch")
    torch.cuda.synchronize()
    got = losses.double().cpu().numpy()
    print(f"{name}: loss terms device {got.tolist()} float64 {ref['loss']}")
    close(got, np.array(ref["loss"]), LOSS_RTOL, LOSS_ATOL, f"ppo step grads {name}: loss, clip, vf, ent")
    # the partials phase 1 left behind the gradient are the same terms
    close(flat[-4:-1].numpy(), np.array(ref["loss"][1:]), LOSS_RTOL, LOSS_ATOL, f"ppo step grads {name}: loss partials of phase 1")
    assert bool(torch.isfinite(ln2.params).all())
    ln.check_handoffs(); ln2.check_handoffs()
    close(np.array(list(used.values())), np.zeros(len(used)), 0, 1.0, f"ppo step grads {name}: share of the bar used {list(used)}")


@pytest.mark.parametrize("name", list(pg.SHARDS))
def test_data_parallel_shards_hold_their_share_of_the_global_loss(name, monkeypatch):
    case, whole = pg.build(name), pg.reference(name)
    _env(monkeypatch, case)
    lo, total, dobs_rows = 0, None, []
    for n in pg.SHARDS[name]:
        ref = pg.reference(name, (lo, lo + n))
        what = f"{name} rows {lo}..{lo + n - 1}"
        _, flat, dobs = _phase1(case, lo, lo + n)
        used, got = _check_grads(case, flat, dobs, ref, lo, lo + n, what)
        close(flat[-4:-1].numpy(), np.array(ref["loss"][1:]), LOSS_RTOL, LOSS_ATOL, f"ppo step grads {what}: loss partials")
        close(np.array(list(used.values())), np.zeros(len(used)), 0, 1.0, f"ppo step grads {what}: share of the bar used {list(used)}")
        total = {k: (got[k] if total is None else total[k] + got[k]) for k in pg.FLAT_ORDER}
        dobs_rows.append(got["obs"])
        lo += n
    assert lo == case["mb"]
    total["obs"] = torch.cat(dobs_rows)
    for k, want in whole["g64"].items():
        e_dev, bar = pg.rel(total[k], want), pg.grad_bar(whole["e32"][k])
        print(f"{name} sum of the shards: {k} {e_dev:.2e} / {whole['e32'][k]:.2e} / {bar:.2e}")
        assert e_dev <= bar, (k, e_dev, bar)
    hb = pg.head_bar(whole["e32"])
    assert pg.rel(total["wa"], whole["g64"]["wa"]) < hb and pg.rel(total["ba"], whole["g64"]["ba"]) < hb


@pytest.mark.parametrize("max_grad_norm", [0.5, 1e3])
@pytest.mark.parametrize("name", pg.ADAM_CASES)
def test_clip_and_adam_follow_the_float64_recurrence_from_the_device_gradient(name, max_grad_norm, monkeypatch):
    case = pg.build(name)
    _env(monkeypatch, case)
    mb, k = case["mb"], 7
    ln = pg.make_learner(case, max_grad_norm=max_grad_norm)
    idx = torch.as_tensor(case["idx"]).cuda()
    slot = torch.zeros(4, dtype=torch.float32, device="cuda")
    ln.mb_phase1(idx, idx, False, slot)
    rng = np.random.RandomState(case["mb"])
    ln.adam_m.copy_(torch.as_tensor((rng.standard_normal(ln.P) * 1e-3).astype(np.float32)))
    ln.adam_v.copy_(torch.as_tensor((rng.uniform(1e-3, 1.0, ln.P) * 1e-5).astype(np.float32)))
    ln.opt_step = k
    d = lambda t: t[:ln.P].double().cpu().numpy()
    g, p0, m0, v0 = d(ln.grads), d(ln.params), d(ln.adam_m), d(ln.adam_v)
    ln.mb_phase2(mb, mb, slot)
    torch.cuda.synchronize()
    assert ln.opt_step == k + 1 and np.array_equal(d(ln.grads), g)
    m1, v1, p1 = d(ln.adam_m), d(ln.adam_v), d(ln.params)
    assert all(np.isfinite(z).all() for z in (g, m1, v1, p1))
    norm, _ = pg.adam_reference(g, case["I"], max_grad_norm)
    what = f"{name} max_grad_norm {max_grad_norm}"
    coef, used = pg.check_clip_adam(p0, m0, v0, g, m1, v1, p1, case["I"], k, max_grad_norm, what=what)
    print(f"{what}: norm {norm:.4f} coef {coef:.6f}; share of each bar used {({a: float('%.3f' % b) for a, b in used.items()})}")
    assert (coef < 1.0) == (max_grad_norm == 0.5), f"{what}: the clip must bind at 0.5 and only there (norm {norm})"
    ln.check_handoffs()
    close(np.array(list(used.values())), np.zeros(len(used)), 0, 1.0, f"ppo step grads {what}: share of the Adam bars used {list(used)}")
