"""GPU: the one-launch evaluation of the VirtualTaobao static baselines (csrc/vtb_static.hip, cirs_hip/vtb_static.py,
evaluation.test_taobao(device="cuda")).

  (a) env side     the device's recorded actions and exported noise through the CPU mirror (tests/vtbcase.py): exits, lengths, states,
                   user draws and epsilon decisions exact; click / second draws under the top-2 margin protocol of
                   tests/test_gpu_virtualtb.py, at most 0.1 % of the draws excused (tests/test_vtb_static_cpu.py checks on the CPU
                   that the mirror against its own float64 restatement stays inside that cap for these inputs)
  (b) policy side  the device's recorded states through the host model: rtol 1e-5 / atol 1e-4 (the MMoE-forward bar of
                   tests/test_gpu_mmoe_train.py), and the device's error against a float64 run no larger than 4 x torch-fp32's own
                   error against it (the multiple tests/test_gpu_head_precision.py grants)
  (c) metrics      the kernel's four metrics against numpy float64 from trajectory(): rtol 1e-12, integers exact
  (d) determinism  same seed -> same bits; another seed -> other users; epsilon = 0 explores nowhere and agrees with the
                   epsilon = 0.3 run wherever that run has not yet diverged
  (e) the public entry returns DeviceVtbStaticEval.run's dict"""
import functools

import numpy as np
import pytest
import torch

import vtbcase
import vtbstaticcase as case
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

N_LEAVE, T, SHAPES, CASES = case.GPU_N_LEAVE, case.GPU_T, case.GPU_SHAPES, case.GPU_CASES
MMOE_TOL = dict(rtol=1e-5, atol=1e-4)      # tests/test_gpu_mmoe_train.py:166
FP32_MULTIPLE = 4.0                        # tests/test_gpu_head_precision.py


@functools.lru_cache(maxsize=None)
def _setup(shape):
    s = SHAPES[shape]
    model = case.two_task_model(s["dnn"], s["num_experts"], s["expert_dim"])
    env = vtbcase.base_vtb(GOLDEN, N_LEAVE, s["thr"], T)
    env.set_state_mode(True)
    return model, env


@functools.lru_cache(maxsize=None)
def _run(shape, n, eps, seed=case.GPU_SEED):
    from cirs_hip.vtb_static import DeviceVtbStaticEval
    model, env = _setup(shape)
    ev = DeviceVtbStaticEval(env, model, n, seed=seed, device="cuda")
    res = ev.run(eps)
    return ev, res, ev.trajectory()


@pytest.mark.parametrize("eps", case.GPU_EPS)
@pytest.mark.parametrize("shape,n", CASES)
def test_env_side_teacher_forced(shape, n, eps):
    ev, _, tr = _run(shape, n, eps)
    _, env = _setup(shape)
    noise = case.fetch_noise(ev, tr["len"])
    draws, forced = case.replay_env_side(env, tr, noise, eps)
    exits = int((tr["len"] < T).sum())
    print(f"{shape} n={n} eps={eps}: turns {int(tr['len'].sum())}, exits {exits}, max_turn ends {n - exits}, explored "
          f"{int(tr['explore'].sum())}, draws {draws}, excused by the margin {forced}, smallest CPU margin {vtbcase.STATS['min_gap']:.3g}")
    assert len(set(tr["len"].tolist())) > 1, "the case should mix short and long trajectories"
    assert forced <= 0.001 * draws
    if eps == 0:
        assert not tr["explore"].any()
    else:
        share = tr["explore"].sum() / tr["len"].sum()
        assert abs(share - eps) < 5 * np.sqrt(eps * (1 - eps) / tr["len"].sum()), share


@pytest.mark.parametrize("eps", case.GPU_EPS)
@pytest.mark.parametrize("shape,n", CASES)
def test_policy_side_teacher_forced(shape, n, eps):
    _, _, tr = _run(shape, n, eps)
    model, _ = _setup(shape)
    live = np.arange(T)[None, :] < tr["len"][:, None]
    x = torch.from_numpy(tr["state"][live])
    with torch.no_grad():
        y32 = model(x).numpy()
    y64 = case.forward64(model, x.numpy())
    own = ~tr["explore"][live]                       # the action is the prediction only where the epsilon branch did not fire
    dev_a, dev_p = tr["action"][live][own], tr["reward_pred"][live]
    from conftest import close
    close(dev_a, y32[own, :27], what=f"vtb static {shape} n={n} eps={eps}: actions vs torch fp32", **MMOE_TOL)
    close(dev_p, y32[:, 27], what=f"vtb static {shape} n={n} eps={eps}: reward_pred vs torch fp32", **MMOE_TOL)
    for name, dev, t32, t64 in (("actions", dev_a, y32[own, :27], y64[own, :27]), ("reward_pred", dev_p, y32[:, 27], y64[:, 27])):
        e_dev, e_t32 = float(np.abs(dev - t64).max()), float(np.abs(t32.astype(np.float64) - t64).max())
        print(f"{shape} n={n} eps={eps} {name}: device vs float64 {e_dev:.3g}, torch fp32 vs float64 {e_t32:.3g}, ratio {e_dev / e_t32:.3f}")
        assert e_dev <= FP32_MULTIPLE * e_t32, (name, e_dev, e_t32)


@pytest.mark.parametrize("eps", case.GPU_EPS)
@pytest.mark.parametrize("shape,n", CASES)
def test_metrics_match_the_trajectory(shape, n, eps):
    ev, res, tr = _run(shape, n, eps)
    want, (clicks, turns) = case.metrics_from_trajectory(tr)
    assert ev.totals == (clicks, turns)
    assert tr["done"].sum() == n and (tr["done"][np.arange(n), tr["len"] - 1]).all()
    for k in case.KEYS:
        np.testing.assert_allclose(res[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    assert res["len_tra"] == turns / n and res["R_tra"] == clicks / n and res["ctr"] == clicks / turns


def test_determinism_and_epsilon_contract():
    from cirs_hip.vtb_static import DeviceVtbStaticEval
    model, env = _setup("script")
    _, res0, tr0 = _run("script", 100, 0.3)
    ev = DeviceVtbStaticEval(env, model, 100, seed=case.GPU_SEED, device="cuda")
    res1 = ev.run(0.3)
    tr1 = ev.trajectory()
    assert res0 == res1
    for k in tr0:
        np.testing.assert_array_equal(tr0[k], tr1[k], err_msg=k)
    ev.seed(1235)
    ev.run(0.3)
    assert not np.array_equal(ev.trajectory()["user"], tr0["user"])
    # epsilon = 0: no exploration anywhere; identical to the epsilon = 0.3 run while that run has not explored
    _, _, trz = _run("script", 100, 0.0)
    assert not trz["explore"].any()
    np.testing.assert_array_equal(trz["user"], tr0["user"])
    same = 0
    for i in range(100):
        for t in range(int(min(trz["len"][i], tr0["len"][i]))):      # every common step, also after the runs have parted and met again
            if tr0["explore"][i, t] or not np.array_equal(trz["state"][i, t], tr0["state"][i, t]):
                continue
            np.testing.assert_array_equal(trz["action"][i, t], tr0["action"][i, t])
            assert trz["reward_pred"][i, t] == tr0["reward_pred"][i, t] and trz["reward"][i, t] == tr0["reward"][i, t]
            same += 1
    assert same >= 50      # turn 0 alone is unexplored with probability 0.7: 70 of 100 expected, sigma 4.6


def test_public_entry_returns_the_same_dict():
    import evaluation
    model, env = _setup("odd")
    _, res, tr = _run("odd", 37, 0.3)
    got = evaluation.test_taobao(model, env, 0.3, device="cuda", num_trajectory=37, seed=case.GPU_SEED)
    assert got == res and set(got) == set(case.KEYS)
    # the defaults: 100 trajectories, seed 0, epsilon 0
    from cirs_hip.vtb_static import DeviceVtbStaticEval
    assert evaluation.test_taobao(model, env, device="cuda") == DeviceVtbStaticEval(env, model, 100, seed=0, device="cuda").run(0.0)
