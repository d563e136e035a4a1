"""Shared cases and the id rule of the sampled-policy tests (cirs_actor_sample and the fused rollout's sampler against policy_host.sample64):
a helper, not a test.  The cases the CPU tests vet (no row of the float64 reference inside a margin, tests/test_sample_host_cpu.py) are the
ones the GPU tests run (tests/test_gpu_sample_f64.py).

Operands are O(1): policycase.random_weights with head_scale 1 and 2, states N(0, 1), dim_state 20.  Every sampler seed has bits above 31 set,
so both Philox key words are live; every case is drawn at the two RNG_STEPS.  Masked cases take their env ids from a permutation that reaches
beyond n (greedycase.case's layout: n + 3 bitmap rows)."""
import functools
import itertools

import numpy as np

import greedycase
import policycase
from cirs_hip import policy_host

CHUNK = policy_host.CHUNK
RNG_STEPS = (0, 7)
HEAD_SCALES = (1.0, 2.0)
SEED0 = (0x5EED << 32) | 0x00C0FFEE      # the search for a case's seed starts here and goes upwards

# (kind, n, I, masked, head_scale).  "grid": greedycase.case (0.3 bit rate, skipped rows, a row with 3 items left); "edge": n = 5 at the catalogue
# sizes where the two-level layout changes -- 1 item, a partial 32-item tile, exactly one chunk, a chunk plus one, 65 chunks (a lane of the
# pick's 64-lane chunk arg-max holds a second chunk), 129 chunks (a third one, which is not prefetched); "one_left" / "exhausted" / "last_word":
# masked, row 2 with exactly one item left / row 3 with every item visited / every row with valid items only in the last, partial bitmap word;
# "lane0_chunks": 129 chunks of which only 0, 64 and 128 -- the three chunks of lane 0 of the pick's chunk arg-max -- have valid items, so that about
# a third of the draws land in the chunk whose mass and noise are not prefetched (among all 129 chunks, "edge" 5 x 16500 draws it once in 129 times).
GRID = [("grid", n, I, m, hs) for n in greedycase.ROWS for I in greedycase.CATALOGUES for m in (False, True) for hs in HEAD_SCALES]
EDGE = [("edge", 5, I, False, hs) for I in (1, 31, 128, 129, 8200, 16500) for hs in HEAD_SCALES]
SPECIAL = [("one_left", 5, 300, True, 1.0), ("exhausted", 5, 300, True, 2.0), ("last_word", 5, 300, True, 1.0),
           ("lane0_chunks", 5, 16500, True, 1.0)]
CASES = GRID + EDGE + SPECIAL


def case_id(key):
    kind, n, I, masked, hs = key
    return f"{kind}-{n}x{I}" + ("-masked" if masked else "") + f"-hs{hs:g}"


IDS = [case_id(k) for k in CASES]

# Per case the first seed >= SEED0 at which no row of the float64 reference, at either rng_step, has its chunk-level gap or the item-level gap
# of its drawn chunk inside the margin (find_seed below; tests/test_sample_host_cpu.py checks every entry, and that it is the FIRST such seed).
# The search (python tests/samplecase.py) found SEED0 itself clean for all 48 cases: about 7 rows in 1e4 lie inside a margin (80 of 116 550 in the
# oracle comparison), and the largest case draws 2 x 130 rows.
SEEDS = {i: SEED0 for i in IDS}


def seed_of(key):
    return SEEDS[case_id(key)]


@functools.lru_cache(maxsize=None)
def case(key):
    """-> dict(arrs, state [n, 20] f32, env_ids, visited, skip, n, n_items), shared and never modified."""
    kind, n, I, masked, hs = key
    if kind == "grid":
        c = greedycase.case(n, I, masked)
        c["arrs"]["wa"] = c["arrs"]["wa"] * np.float32(hs)      # random_weights(head_scale = hs): the factor is exact for 1 and 2
        return c
    rng = np.random.RandomState(7000 + 31 * I + n + sum(map(ord, kind)))
    arrs = {k: np.asarray(v, np.float32) for k, v in policycase.random_weights(rng, I, head_scale=hs).items()}
    c = dict(arrs=arrs, state=rng.normal(0, 1, (n, 20)).astype(np.float32), env_ids=None, visited=None, skip=None, n=n, n_items=I)
    if masked:
        B, words = n + 3, (I + 31) // 32
        bits = rng.uniform(size=(B, words * 32)) < 0.3
        env_ids = rng.permutation(B)[:n].astype(np.int32)
        if kind == "one_left":
            bits[env_ids[2]] = True
            bits[env_ids[2], rng.randint(I)] = False
        elif kind == "exhausted":
            bits[env_ids[3], :I] = True      # (the bits past I in the last word stay random: they belong to no item)
        elif kind == "last_word":
            first = (words - 1) * 32
            bits[:, :first] = True
            for e in range(B):      # at least two valid items in the partial word
                bits[e, first + rng.permutation(I - first)[:2]] = False
        elif kind == "lane0_chunks":
            keep = np.zeros(words * 32, bool)
            for ch in (0, 64, 128):
                keep[ch * CHUNK:(ch + 1) * CHUNK] = True
            bits[:, ~keep] = True
        c["visited"] = np.packbits(bits.reshape(B, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(B, words)
        c["env_ids"] = env_ids
    return c


def draw64(key, seed, rng_step):
    c = case(key)
    return policy_host.sample64(c["arrs"], c["state"], seed, rng_step, c["env_ids"], c["visited"], c["skip"])


# ---- the id rule, classified by level ------------------------------------------------------------------------------------------
def close_levels(ref):
    """(chunk_close [n], item_close [n, C]): the float64 top-2 gap of the level is inside greedycase's margin of its noisy winning score."""
    with np.errstate(invalid="ignore"):
        return (ref["chunk_gap"] <= greedycase.margin_of(ref["chunk_score"]),
                ref["item_gap"] <= greedycase.margin_of(ref["item_score"]))


def rows_inside(ref):
    """the number of drawn rows whose chunk-level gap, or whose drawn chunk's item-level gap, is inside the margin"""
    chunk_close, item_close = close_levels(ref)
    live = ref["act"] >= 0
    drawn = np.take_along_axis(item_close, np.maximum(ref["chunk"], 0)[:, None], axis=1)[:, 0]
    return int((live & (chunk_close | drawn)).sum())


def check_sampled_ids(got, ref, what=""):
    """Device ids `got` [n] against policy_host.sample64's dict.  With d the device's id and w the float64 one:
      same chunk      -> d == w, unless that chunk's item-level gap is inside the margin: then d may be its item-level runner-up;
      another chunk   -> the chunk-level gap is inside the margin, d's chunk is the runner-up chunk, and d is that chunk's float64 item-level
                         winner (or its runner-up, if that chunk's item-level gap is inside the margin);
      a -1 on one side only is never a margin effect.
    Raises AssertionError on the first row that breaks the rule; returns the number of rows inside a margin (rows_inside)."""
    got = np.asarray(got).reshape(-1)
    want = ref["act"]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    chunk_close, item_close = close_levels(ref)
    for j in np.flatnonzero(got != want):
        d, w = int(got[j]), int(want[j])
        assert d >= 0 and w >= 0, (what, f"row {j}: {d} on the device, {w} in float64")
        cd, cw = d // CHUNK, w // CHUNK
        assert cd < ref["item_win"].shape[1], (what, f"row {j}: id {d} beyond the catalogue")
        if cd == cw:
            assert item_close[j, cw] and d == ref["item_runner_up"][j, cw], \
                (what, f"row {j}: item {d} instead of {w} in chunk {cw}, item gap {ref['item_gap'][j, cw]:.3g}, runner-up {ref['item_runner_up'][j, cw]}")
        else:
            assert chunk_close[j] and cd == ref["chunk_runner_up"][j], \
                (what, f"row {j}: chunk {cd} (item {d}) instead of chunk {cw} (item {w}), chunk gap {ref['chunk_gap'][j]:.3g}, "
                       f"runner-up chunk {ref['chunk_runner_up'][j]}")
            assert d == ref["item_win"][j, cd] or (item_close[j, cd] and d == ref["item_runner_up"][j, cd]), \
                (what, f"row {j}: item {d} of the runner-up chunk {cd}, whose float64 winner is {ref['item_win'][j, cd]} "
                       f"(item gap {ref['item_gap'][j, cd]:.3g})")
    return rows_inside(ref)


def find_seed(key, start=SEED0, tries=200):
    """the first seed >= start whose float64 draws of the case leave no row inside either margin at both RNG_STEPS"""
    for seed in itertools.islice(itertools.count(start), tries):
        if all(rows_inside(draw64(key, seed, step)) == 0 for step in RNG_STEPS):
            return seed
    raise AssertionError(f"{case_id(key)}: no seed in {tries} tries")


if __name__ == "__main__":      # prints the SEEDS table: python tests/samplecase.py (with tests/ and cirs-codes_amd/ on the path)
    for k in CASES:
        print(f'    "{case_id(k)}": SEED0 + {find_seed(k) - SEED0},')
