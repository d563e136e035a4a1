"""GPU: the sampled policy step -- cirs_actor_sample (counter-based two-level draw and the harness-noise path) and the fused rollout's three
sampler forms -- against the float64 restatement (cirs_hip/policy_host.py: sample64 / logp64_at / sample_with_noise64), not the C oracle: a
design error shared by kernel and oracle, a wrong log-prob on a draw whose id differs from the reference's, and a draw in the wrong chunk all
show here.  Ids go under the level-classified rule of tests/samplecase.py; log-probs are compared at the DEVICE's own id, on every live row."""
import functools

import numpy as np
import pytest
import torch

import greedycase
import rolloutcase
import samplecase
from cirs_hip import policy_host

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def _policy(arrs, I):
    from cirs_hip.policy import DevicePolicy
    return DevicePolicy({rolloutcase.POLICY_NAMES[k]: _dev(v) for k, v in arrs.items()}, I)


def _dev_inputs(c):
    return dict(env_ids=_dev(c["env_ids"]), visited=_dev(None if c["visited"] is None else c["visited"].view(np.int32)), skip=_dev(c["skip"]))


def _check_logp_value(c, act, logp, value, w_value, what):
    """log-prob of EVERY row at the device's own id (0 where it drew nothing), value of every row the trunk ran on; no masked id"""
    n, I = c["state"].shape[0], c["arrs"]["wa"].shape[0]
    want = policy_host.logp64_at(c["arrs"], c["state"], act, c["env_ids"], c["visited"])
    np.testing.assert_allclose(logp, want, rtol=1e-4, atol=1e-4, err_msg=what)
    assert (logp[act < 0] == 0).all(), what
    ran = np.ones(n, bool) if c["skip"] is None else c["skip"] == 0
    np.testing.assert_allclose(value[ran], w_value[ran], rtol=1e-5, atol=1e-5, err_msg=what)
    assert ((act >= -1) & (act < I)).all(), what
    if c["visited"] is not None:
        rows = np.flatnonzero(act >= 0)
        assert not policy_host.mask_from_bitmap(c["visited"], c["env_ids"], n, I)[rows, act[rows]].any(), (what, "a masked item was chosen")


@pytest.mark.parametrize("key", samplecase.CASES, ids=samplecase.IDS)
def test_counter_sampler_against_float64(key):
    kind, n, I, masked, hs = key
    c = samplecase.case(key)
    pol, d = _policy(c["arrs"], I), _dev_inputs(c)
    seed = samplecase.seed_of(key)
    state = _dev(c["state"])
    for step in samplecase.RNG_STEPS:
        what = f"{samplecase.case_id(key)} step {step}"
        act, logp, value = (x.cpu().numpy() for x in pol.sample(state, seed=seed, rng_step=step, **d))
        ref = samplecase.draw64(key, seed, step)
        inside = samplecase.check_sampled_ids(act, ref, what)
        assert inside == 0, "the seeds were chosen with no row inside a margin (tests/test_sample_host_cpu.py)"
        _check_logp_value(c, act, logp, value, ref["value"], what)
        if c["skip"] is not None:
            assert (act[c["skip"] != 0] == -1).all()
        if kind == "one_left":
            assert logp[2] == pytest.approx(np.log(1.0 - policy_host.EPS32), abs=1e-6) and act[2] >= 0
        if kind == "exhausted":
            assert act[3] == -1 and logp[3] == 0


@pytest.mark.parametrize("n,I,masked", [(n, I, m) for n in greedycase.ROWS for I in greedycase.CATALOGUES for m in (False, True)])
def test_harness_noise_sampler_against_float64(n, I, masked):
    c = greedycase.case(n, I, masked)
    rng = np.random.RandomState(50000 + 1000 * n + I + masked)
    u = (rng.randint(0, 1 << 23, size=(n, I)) + 0.5) * 2.0 ** -23      # the open interval: g is finite
    g = (-np.log(-np.log(u))).astype(np.float32)
    pol = _policy(c["arrs"], I)
    act, logp, value = (x.cpu().numpy() for x in pol.sample(_dev(c["state"]), gumbel=_dev(g), **_dev_inputs(c)))
    w_act, w_value, gap, ru, score = policy_host.sample_with_noise64(c["arrs"], c["state"], g, c["env_ids"], c["visited"], c["skip"])
    live = w_act >= 0
    assert np.array_equal(act >= 0, live) and (act[~live] == -1).all()
    greedycase.check_greedy_ids(act[live], w_act[live], gap[live], ru[live], score[live], f"harness noise {n}x{I}")
    _check_logp_value(c, act, logp, value, w_value, f"harness noise {n}x{I}")


# ---- the fused rollout's sampler forms -------------------------------------------------------------------------------------------
U = 60
RNG_BASE = 100
# name: (B, I, T, head_scale, env switches, rollout keywords) -> the sampler form the fused steps take
ROLLOUTS = {
    "mass_small+store": (5, 300, 6, 1.0, {}, {}),                                                      # n_pad 32 <= 128
    "mass_generic+store": (130, 300, 6, 2.0, {}, {}),                                                  # n_pad 160 > 128
    "switched_off": (5, 300, 6, 1.0, {"CIRS_ROLLOUT_ZSTORE": "0", "CIRS_ROLLOUT_MASS_SMALL": "0"}, {}),   # generic mass kernel, recomputed chunk
    "store_off_by_size": (130, 6700, 3, 1.0, {}, {}),                                                  # 160 * 53 * 128 floats > 2^20
    "masked": (130, 300, 6, 2.0, {}, dict(remove_recommended_ids=True)),
}


@pytest.mark.parametrize("name", list(ROLLOUTS))
def test_rollout_sampler_against_float64(name, monkeypatch):
    from cirs_hip.synthetic import make_tables
    B, I, T, hs, env, kw = ROLLOUTS[name]
    for k in ("CIRS_ROLLOUT_ZSTORE", "CIRS_ROLLOUT_MASS_SMALL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tab = make_tables(U, I, seed=0, build_dist=False)
    users = torch.as_tensor(np.random.RandomState(3).randint(0, U, B))
    ro, tp, arrs, envp = rolloutcase.build_device_stack(tab, B, T, N=3, thr=1, head_scale=hs, **kw)
    arrs = {k: np.asarray(v, np.float32) for k, v in arrs.items()}      # the weights as the device holds them
    seed = samplecase.SEED0 + 5
    L = ro.collect(users, seed=seed, rng_base=RNG_BASE).cpu().numpy()
    tr = ro.traj
    act, obs, logp, value = tr.act.cpu().numpy(), tr.obs.cpu().numpy(), tr.logp.cpu().numpy(), tr.value.cpu().numpy()
    assert L.min() >= 1 and L.max() <= T
    assert np.array_equal(act >= 0, np.arange(T)[:, None] < L[None, :])
    # teacher-forced, step by step: the float64 draw on the stored state, env id = column, under the ids the device has drawn so far
    masked = bool(kw.get("remove_recommended_ids"))
    bm = np.zeros((B, (I + 31) // 32), np.uint32)
    inside = 0
    for t in range(int(L.max())):
        live = act[t] >= 0
        vis = bm.copy() if masked else None
        ref = policy_host.sample64(arrs, obs[t], seed, RNG_BASE + t, None, vis, (~live).astype(np.uint8))
        what = f"{name} step {t}"
        inside += samplecase.check_sampled_ids(act[t], ref, what)
        want = policy_host.logp64_at(arrs, obs[t], act[t], None, vis)
        np.testing.assert_allclose(logp[t][live], want[live], rtol=1e-4, atol=1e-4, err_msg=what)
        np.testing.assert_allclose(value[t][live], ref["value"][live], rtol=1e-5, atol=1e-5, err_msg=what)
        rows, a = np.flatnonzero(live), act[t][live]
        if masked:
            assert not policy_host.mask_from_bitmap(vis, None, B, I)[rows, a].any(), (what, "a masked item was chosen")
        np.bitwise_or.at(bm, (rows, a >> 5), np.uint32(1) << (a & 31).astype(np.uint32))
    print(f"rollout {name}: {int(L.sum())} draws, {inside} rows inside a margin")
    assert inside <= 0.01 * L.sum()
