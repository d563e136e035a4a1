"""CPU: the float64 restatement of the sampled policy step (cirs_hip/policy_host.py: sample64, logp64_at, sample_with_noise64) and the
level-classified id rule (tests/samplecase.py), before the GPU tests rely on either:
  - sample64 against the C oracle's fp32 two-level draw over more than 1e5 draws: pins the Philox counters, the chunk layout and the mask
    handling of the new restatement to the existing one, and measures from the reference side that an fp32 evaluation of this design stays
    inside greedycase.MARGIN of float64;
  - the restatement samples the distribution it claims (chi-square against the float64 masked soft-max);
  - the recorded seeds leave no row inside a margin; the rule rejects a wrong-chunk draw that the former min() rule accepted."""
import os

import numpy as np
import pytest

import greedycase
import policycase
import samplecase
from cirs_hip import policy_host

STEPS_PER_CASE = 90      # rng_steps per case in the oracle comparison: 1295 live rows over all cases x 90 > 1e5 draws


def test_philox_known_answers():
    """Random123's known-answer vectors of Philox4x32-10 (kat_vectors: zero counter / key, all-ones, the digits of pi)."""
    ff = 0xFFFFFFFF
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((ff, ff, ff, ff), (ff, ff), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
                            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = policy_host.philox4x32_10(*ctr, *key)
        assert tuple(int(x) for x in got) == want


def test_sample64_against_the_c_oracle():
    draws = differ = inside = 0
    worst = 0.0      # the largest (float64 gap) / margin among the draws where the fp32 oracle and float64 disagree: <= 1 by the rule
    closest = np.inf      # the smallest gap / margin of any level of any draw: how close the closest decision was
    for key in samplecase.CASES:
        c = samplecase.case(key)
        for k in range(STEPS_PER_CASE):
            seed, step = samplecase.SEED0 + 977 * k, 3 * k + (k & 1)
            ref = policy_host.sample64(c["arrs"], c["state"], seed, step, c["env_ids"], c["visited"], c["skip"])
            act, logp, value, _ = policycase.oracle_sample(c["arrs"], c["state"], seed=seed, rng_step=step, env_ids=c["env_ids"],
                                                           visited=c["visited"], skip=c["skip"])
            what = f"{samplecase.case_id(key)} seed {seed:#x} step {step}"
            inside += samplecase.check_sampled_ids(act, ref, what)
            live = ref["act"] >= 0
            draws += int(live.sum())
            drawn = np.maximum(ref["chunk"], 0)[:, None]
            with np.errstate(invalid="ignore"):      # (rows and chunks with no candidate: inf / inf)
                ratios = np.minimum(ref["chunk_gap"] / greedycase.margin_of(ref["chunk_score"]),
                                    np.take_along_axis(ref["item_gap"] / greedycase.margin_of(ref["item_score"]), drawn, axis=1)[:, 0])
            closest = min(closest, ratios[live].min(initial=np.inf))
            diff = np.flatnonzero(act != ref["act"])
            differ += len(diff)
            for j in diff:      # which level flipped, and how far inside the margin it was
                cw = ref["chunk"][j]
                if act[j] // samplecase.CHUNK == cw:
                    worst = max(worst, ref["item_gap"][j, cw] / greedycase.margin_of(ref["item_score"][j, cw]))
                else:
                    worst = max(worst, ref["chunk_gap"][j] / greedycase.margin_of(ref["chunk_score"][j]))
            same = live & (act == ref["act"])
            want_logp = policy_host.logp64_at(c["arrs"], c["state"], ref["act"], c["env_ids"], c["visited"])
            np.testing.assert_allclose(logp[same], want_logp[same], rtol=1e-4, atol=1e-4, err_msg=what)
            np.testing.assert_allclose(value[live], ref["value"][live], rtol=1e-5, atol=1e-5, err_msg=what)
            assert (want_logp[~live] == 0).all()
    print(f"sample64 vs the C oracle: {draws} draws, {differ} ids differ (all by the rule), {inside} rows inside a margin, "
          f"largest gap / margin of a differing draw {worst:.3g}, smallest gap / margin of any draw {closest:.3g}")
    assert draws >= 100000


def test_logp64_at_clamps_and_ignores_the_draw():
    key = ("one_left", 5, 300, True, 1.0)
    c = samplecase.case(key)
    ref = samplecase.draw64(key, samplecase.seed_of(key), 0)
    lp = policy_host.logp64_at(c["arrs"], c["state"], ref["act"], c["env_ids"], c["visited"])
    assert lp[2] == np.log(1.0 - policy_host.EPS32)                       # one item left: probability 1, clamped
    masked = policy_host.mask_from_bitmap(c["visited"], c["env_ids"], 5, 300)
    ids = np.array([np.flatnonzero(masked[j])[0] for j in range(5)])      # a masked id: probability 0, clamped
    assert (policy_host.logp64_at(c["arrs"], c["state"], ids, c["env_ids"], c["visited"]) == np.log(policy_host.EPS32)).all()
    # unmasked: the plain log-soft-max
    z, _ = policy_host.forward64(c["arrs"], c["state"])
    want = z[:, 17] - np.log(np.exp(z).sum(axis=1))
    np.testing.assert_allclose(policy_host.logp64_at(c["arrs"], c["state"], np.full(5, 17)), want, rtol=1e-12)
    assert (policy_host.logp64_at(c["arrs"], c["state"], np.full(5, -1)) == 0).all()


def test_special_cases_are_what_they_claim():
    for key in samplecase.SPECIAL:
        kind, n, I, _, _ = key
        c = samplecase.case(key)
        left = (~policy_host.mask_from_bitmap(c["visited"], c["env_ids"], n, I)).sum(axis=1)
        assert c["env_ids"].max() >= n and len(set(c["env_ids"].tolist())) == n
        ref = samplecase.draw64(key, samplecase.seed_of(key), 7)
        if kind == "one_left":
            assert left[2] == 1 and ref["act"][2] >= 0 and np.isinf(ref["chunk_gap"][2]) and np.isinf(ref["item_gap"][2, ref["chunk"][2]])
        elif kind == "exhausted":
            assert left[3] == 0 and ref["act"][3] == -1 and (np.delete(ref["act"], 3) >= 0).all()
        elif kind == "last_word":
            assert (left >= 2).all() and (ref["act"] >= 288).all() and (ref["chunk"] == 2).all()
        else:      # lane0_chunks: every draw in chunk 0, 64 or 128, and the third one is reached
            chunks = np.concatenate([samplecase.draw64(key, samplecase.seed_of(key), s)["chunk"] for s in samplecase.RNG_STEPS])
            assert set(chunks.tolist()) <= {0, 64, 128} and (chunks == 128).sum() >= 2


def test_sample_with_noise64_reproduces_the_reference_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "policy.npz"))
    arrs = policycase.weights_from_golden(z)
    g = (-np.log(z["q"])).astype(np.float32)
    act, value, gap, ru, score = policy_host.sample_with_noise64(arrs, z["s"], g)
    assert np.array_equal(act, z["act"])
    np.testing.assert_allclose(policy_host.logp64_at(arrs, z["s"], act), z["logp"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(value, z["value"], rtol=1e-5, atol=1e-5)
    n, I = len(z["s"]), arrs["wa"].shape[0]
    bm = policycase.visited_bitmap(z["visited"], n, I)
    act_m, *_ = policy_host.sample_with_noise64(arrs, z["s"], g, visited=bm)
    assert np.array_equal(act_m, z["act_masked"])


def _chi2_quantile(dof, z):
    """Wilson-Hilferty: the chi-square quantile at the normal deviate z"""
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3


def test_sample64_draws_the_masked_softmax():
    """2e5 draws of ONE state over consecutive env ids and rng_steps against the float64 masked soft-max.  Integer-keyed noise and a fixed
    seed: the statistic is the same number on every machine."""
    I, n_env, steps = 300, 2000, 100
    rng = np.random.RandomState(11)
    arrs = policycase.random_weights(rng, I, head_scale=1.0)
    state = np.repeat(rng.normal(0, 1, (1, 20)), n_env, axis=0).astype(np.float32)
    bits = rng.uniform(size=320) < 0.3
    row = np.packbits(bits.reshape(10, 32), axis=-1, bitorder="little").view(np.uint32).reshape(1, 10)
    visited = np.repeat(row, n_env, axis=0)
    counts = np.zeros(I, np.int64)
    for t in range(steps):
        act = policy_host.sample64(arrs, state, samplecase.SEED0, 50 + t, np.arange(n_env, dtype=np.int32), visited)["act"]
        assert (act >= 0).all()
        counts += np.bincount(act, minlength=I)
    assert counts[bits[:I]].sum() == 0, "a masked id was drawn"
    zl, _ = policy_host.forward64(arrs, state[:1])
    zl = np.where(bits[:I], -np.inf, zl[0])
    p = np.exp(zl - zl.max()); p /= p.sum()
    expect = counts.sum() * p
    big = expect >= 5                                   # items of expected count below 5 (masked ones: 0) are pooled into one cell
    obs, exp = counts[big].astype(np.float64), expect[big]
    if (~big).any() and expect[~big].sum() > 0:
        obs, exp = np.append(obs, counts[~big].sum()), np.append(exp, expect[~big].sum())
    chi2 = ((obs - exp) ** 2 / exp).sum()
    dof = len(exp) - 1
    bound = _chi2_quantile(dof, 4.753424)               # the 1 - 1e-6 quantile
    print(f"chi-square {chi2:.1f} at {dof} degrees of freedom, 1 - 1e-6 quantile {bound:.1f}")
    assert dof >= 30 and chi2 < bound
    # the first stage alone: the chunk counts against the chunk masses
    pc, cc = np.add.reduceat(p, [0, 128, 256]), np.add.reduceat(counts, [0, 128, 256])
    chi2_c = ((cc - counts.sum() * pc) ** 2 / (counts.sum() * pc)).sum()
    assert chi2_c < _chi2_quantile(2, 4.753424)


@pytest.mark.parametrize("key", samplecase.CASES, ids=samplecase.IDS)
def test_recorded_seeds_leave_no_row_inside_a_margin(key):
    seed = samplecase.seed_of(key)
    assert seed >> 32, "both key words must be live"
    for step in samplecase.RNG_STEPS:
        assert samplecase.rows_inside(samplecase.draw64(key, seed, step)) == 0
    assert samplecase.find_seed(key) == seed, "SEEDS must hold the FIRST clean seed from SEED0 upwards"


def _hand_made():
    """One row, two chunks: float64 draws item 5 of chunk 0 with a comfortable chunk-level gap and a tiny item-level gap; chunk 1's winner is 130."""
    return dict(act=np.array([5]), chunk=np.array([0]), chunk_score=np.array([1.5]), chunk_gap=np.array([0.5]), chunk_runner_up=np.array([1]),
                item_win=np.array([[5, 130]]), item_runner_up=np.array([[9, 131]]), item_score=np.array([[2.0, 1.0]]),
                item_gap=np.array([[1e-9, 0.7]]))


def test_level_rule_rejects_a_wrong_chunk_draw_the_min_rule_accepted(monkeypatch):
    monkeypatch.setattr(policycase, "DRAW_STATS", dict(policycase.DRAW_STATS))      # the session's totals count device draws only
    ref = _hand_made()
    margins = np.array([[ref["chunk_gap"][0], ref["item_gap"][0, 0]]])
    assert margins.min(axis=1)[0] <= policycase.DRAW_MARGIN          # the former rule: min(chunk margin, item margin) <= 1e-6 accepts ANY id
    with pytest.raises(AssertionError):
        samplecase.check_sampled_ids(np.array([130]), ref)           # the wrong chunk, far outside the chunk-level margin
    with pytest.raises(AssertionError):
        policycase.assert_draws_match(np.array([130]), ref["act"], margins)
    # what the rule does accept: the id itself and the item-level runner-up of the same chunk; the row counts as inside a margin
    assert samplecase.check_sampled_ids(np.array([5]), ref) == 1
    assert samplecase.check_sampled_ids(np.array([9]), ref) == 1
    policycase.assert_draws_match(np.array([9]), ref["act"], margins)
    with pytest.raises(AssertionError):
        samplecase.check_sampled_ids(np.array([7]), ref)             # same chunk, but not the runner-up
    with pytest.raises(AssertionError):
        samplecase.check_sampled_ids(np.array([-1]), ref)
    # a close chunk level: the runner-up chunk's winner passes, its runner-up (item gap 0.7) and another chunk's item do not
    ref["chunk_gap"] = np.array([1e-6])
    assert samplecase.check_sampled_ids(np.array([130]), ref) == 1
    with pytest.raises(AssertionError):
        samplecase.check_sampled_ids(np.array([131]), ref)
    ref["item_gap"][0, 1] = 1e-7
    assert samplecase.check_sampled_ids(np.array([131]), ref) == 1
    with pytest.raises(AssertionError):
        policycase.assert_draws_match(np.array([130]), ref["act"], np.array([[0.5, 1e-9]]), "chunk margin 0.5")
    with pytest.raises(AssertionError):
        policycase.assert_draws_match(np.array([9]), ref["act"], np.array([[1e-9, 0.5]]), "item margin 0.5")
