"""GPU: deterministic evaluation of the KuaishouEnv policy -- cirs_actor_greedy, cirs_actor_topk and the fused greedy rollout -- against the
float64 restatement (cirs_hip/policy_host.py) of the reference's rule (core/policy/ppo.py:149-151: logits_masked.argmax(-1), ties to the
lowest id).  Shapes: 130 items = one full 128-item chunk + 2, 300 = three chunks with a partial last one; rows 1 / 5 / 37 / 130 = one row,
a partial 32-row tile, two tiles, more than the 128-row small-count threshold."""
import functools

import numpy as np
import pytest
import torch

import greedycase
import rolloutcase
from cirs_hip import policy_host

pytestmark = pytest.mark.gpu

SHAPES = [(n, I, masked) for n in greedycase.ROWS for I in greedycase.CATALOGUES for masked in (False, True)]


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


@functools.lru_cache(maxsize=None)
def _run(n, I, masked):
    """One case on the device and in float64: computed once, shared by the tests (never modified)."""
    from cirs_hip.policy import DevicePolicy
    c = greedycase.case(n, I, masked)
    pol = DevicePolicy({rolloutcase.POLICY_NAMES[k]: _dev(v) for k, v in c["arrs"].items()}, I)
    dev = dict(state=_dev(c["state"]), env_ids=_dev(c["env_ids"]), visited=_dev(None if c["visited"] is None else c["visited"].view(np.int32)),
               skip=_dev(c["skip"]))
    act, logp, value = pol.greedy(dev["state"], env_ids=dev["env_ids"], visited=dev["visited"], skip=dev["skip"])
    want = policy_host.greedy64(c["arrs"], c["state"], c["env_ids"], c["visited"], c["skip"])
    return c, pol, dev, (act, logp, value), want


@pytest.mark.parametrize("n,I,masked", SHAPES)
def test_actor_greedy_against_float64(n, I, masked):
    c, pol, dev, (act, logp, value), (w_act, w_logp, w_value, gap, ru) = _run(n, I, masked)
    act, logp, value = act.cpu().numpy(), logp.cpu().numpy(), value.cpu().numpy()
    live = w_act >= 0
    assert np.array_equal(act >= 0, live) and (act[~live] == -1).all()          # skipped rows
    z, _ = policy_host.forward64(c["arrs"], c["state"])
    rows = np.flatnonzero(live)
    inside = greedycase.check_greedy_ids(act[live], w_act[live], gap[live], ru[live], z[rows, w_act[live]], f"greedy {n}x{I}")
    assert inside == 0, "the seeds were chosen with no row inside the margin (tests/test_greedy_cpu.py)"
    np.testing.assert_allclose(logp[live], w_logp[live], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(value[live], w_value[live], rtol=1e-5, atol=1e-5)
    if masked:
        mk = policy_host.mask_from_bitmap(c["visited"], c["env_ids"], n, I)
        assert not mk[rows, act[live]].any(), "a masked item was chosen"


@pytest.mark.parametrize("k", [1, 7, 32])
@pytest.mark.parametrize("n,I,masked", SHAPES)
def test_actor_topk_against_float64(n, I, masked, k):
    c, pol, dev, (act, logp, _), _ = _run(n, I, masked)
    ids, lp = pol.topk(dev["state"], k, env_ids=dev["env_ids"], visited=dev["visited"], skip=dev["skip"])
    assert ids.shape == (n, k) and ids.dtype == torch.int64 and lp.shape == (n, k) and lp.dtype == torch.float32
    if k == 1:      # the same head kernel and merge: cirs_actor_greedy's bits
        assert torch.equal(ids[:, 0], act)
        live = act >= 0
        assert torch.equal(lp[:, 0][live], logp[live]) and bool(torch.isneginf(lp[:, 0][~live]).all())
    ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
    w_ids, w_lp, gaps, z = policy_host.topk64(c["arrs"], c["state"], k + 1, c["env_ids"], c["visited"], c["skip"])
    greedycase.check_topk_ids(ids, w_ids, gaps, z, f"topk {n}x{I} k={k}")
    mk = policy_host.mask_from_bitmap(c["visited"], c["env_ids"], n, I)
    for j in range(n):
        got = ids[j][ids[j] >= 0]
        n_live = 0 if (c["skip"] is not None and c["skip"][j]) else int((~mk[j]).sum())
        assert len(got) == min(k, n_live) and (ids[j, len(got):] == -1).all() and np.isneginf(lp[j, len(got):]).all(), j
        assert len(set(got.tolist())) == len(got), f"row {j}: duplicate ids"
        assert not mk[j, got].any(), f"row {j}: a masked id in the list"
        same = ids[j] == w_ids[j, :k]
        np.testing.assert_allclose(lp[j][same & (ids[j] >= 0)], w_lp[j, :k][same & (ids[j] >= 0)], rtol=1e-4, atol=1e-4)
        assert (np.diff(lp[j, :len(got)]) <= 1e-6).all(), f"row {j}: log-probs not descending"
    if masked:
        assert (ids[n - 1] >= 0).sum() == min(k, 3)                       # the row with 3 items left: k = 7 gives four fills
        if n > 1:
            assert (ids[1] == -1).all()                                   # a skipped row


# ---- fused greedy rollout --------------------------------------------------------------------------------------------------------
U, I_RO, T_RO = 60, 300, 6
MODES = {"plain": {}, "masked": dict(remove_recommended_ids=True), "masked_forced": dict(remove_recommended_ids=True, force_length=4)}


def _snapshot(ro, lens):
    tr = ro.traj
    return dict(lens=lens.clone(), act=tr.act.clone(), rew=tr.rew.clone(), done=tr.done.clone(), logp=tr.logp.clone(), value=tr.value.clone(),
                ctr=tr.ctr.clone(), obs=tr.obs.clone(), x_hist=ro.tracker.x_hist.clone(), tlen=ro.tracker.len.clone(), turn=ro.env.turn.clone(),
                edone=ro.env.done.clone())


def _assert_same_collect(a, b):
    for k in ("lens", "act", "rew", "done", "logp", "ctr", "tlen", "turn", "edone"):
        assert torch.equal(a[k], b[k]), k
    live = a["act"] >= 0
    assert torch.equal(a["value"][live], b["value"][live])
    lens = a["lens"].cpu().numpy()
    for e in range(len(lens)):
        assert torch.equal(a["obs"][:lens[e] + 1, e], b["obs"][:lens[e] + 1, e]), e
        assert torch.equal(a["x_hist"][e, :lens[e] + 1], b["x_hist"][e, :lens[e] + 1]), e


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [5, 130])
def test_greedy_rollout(B, mode):
    from cirs_hip.synthetic import make_tables
    kw = MODES[mode]
    tab = make_tables(U, I_RO, seed=0, build_dist=False)
    users = torch.as_tensor(np.random.RandomState(3).randint(0, U, B))
    build = lambda: rolloutcase.build_device_stack(tab, B, T_RO, N=3, thr=1, **kw)      # noqa: E731
    ro, tp, arrs, envp = build()
    arrs = {k: np.asarray(v, np.float32) for k, v in arrs.items()}      # the weights as the device holds them
    lens = ro.collect(users, seed=5, rng_base=0, greedy=True)
    one = _snapshot(ro, lens)
    act, obs = one["act"].cpu().numpy(), one["obs"].cpu().numpy()
    logp, value, L = one["logp"].cpu().numpy(), one["value"].cpu().numpy(), lens.cpu().numpy()
    assert L.min() >= 1 and L.max() <= T_RO
    tt = np.arange(T_RO)[:, None]
    assert np.array_equal(act >= 0, tt < L[None, :])
    if kw.get("force_length"):
        assert (L == 4).all()
    # teacher-forced, step by step: the float64 arg-max of the stored state under the ids the env has drawn so far
    words = (I_RO + 31) // 32
    bm = np.zeros((B, words), np.uint32)
    inside = 0
    for t in range(int(L.max())):
        live = act[t] >= 0
        w_act, w_logp, w_value, gap, ru = policy_host.greedy64(arrs, obs[t], None, bm if kw.get("remove_recommended_ids") else None,
                                                               (~live).astype(np.uint8))
        z, _ = policy_host.forward64(arrs, obs[t])
        rows = np.flatnonzero(live)
        inside += greedycase.check_greedy_ids(act[t][live], w_act[live], gap[live], ru[live], z[rows, w_act[live]], f"step {t}")
        same = live & (act[t] == w_act)
        np.testing.assert_allclose(logp[t][same], w_logp[same], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(value[t][live], w_value[live], rtol=1e-5, atol=1e-5)
        a = act[t][live]
        np.bitwise_or.at(bm, (rows, a >> 5), np.uint32(1) << (a & 31).astype(np.uint32))
    assert inside <= 0.01 * L.sum()
    if kw.get("remove_recommended_ids"):
        for b in range(B):
            a = act[:L[b], b]
            assert len(set(a.tolist())) == len(a), f"env {b}: an id repeats inside the episode"
    # cirs_rollout_collect_greedy == reset + one cirs_rollout_steps_greedy(t, t + 1) per step, bit for bit
    ro2, *_ = build()
    ro2.reset(users)
    for t in range(T_RO):
        ro2.run_steps(t, t + 1, 0, 0, greedy=True)
    _assert_same_collect(one, _snapshot(ro2, ro2.env.turn.clone()))
    # no noise is drawn: another sampler seed changes nothing
    lens3 = ro2.collect(users, seed=991, rng_base=77, greedy=True)
    _assert_same_collect(one, _snapshot(ro2, lens3))
    # ... and a greedy collect leaves nothing behind that a later sampled collect could see
    lens_s = ro.collect(users, seed=5, rng_base=12)
    after = _snapshot(ro, lens_s)
    ro4, *_ = build()
    fresh = _snapshot(ro4, ro4.collect(users, seed=5, rng_base=12))
    _assert_same_collect(after, fresh)
    assert not torch.equal(after["act"], one["act"])      # (the sampled rollout is a different one)


def test_greedy_rollout_refusals():
    from cirs_hip.synthetic import make_tables
    tab = make_tables(U, I_RO, seed=0, build_dist=False)
    ro, *_ = rolloutcase.build_device_stack(tab, 5, T_RO, N=3, thr=1)
    users = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError):
        ro.collect(users, greedy=True, gumbel=np.zeros((T_RO, 5, I_RO), np.float32))
    with pytest.raises(ValueError):
        ro.run_steps(0, 1, 0, 0, gumbel=torch.zeros((T_RO, 5, I_RO)), greedy=True)
