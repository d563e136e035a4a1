"""Shared inputs and checks of the deterministic-evaluation tests (cirs_actor_greedy / cirs_actor_topk / the greedy rollouts): the cases the
CPU tests vet (top-2 gaps of the float64 reference) are the ones the GPU tests run."""
import numpy as np

import policycase
from cirs_hip import policy_host

ROWS, CATALOGUES = (1, 5, 37, 130), (130, 300)
# Ids must agree wherever the float64 top-2 gap exceeds MARGIN * max(1, |logit|): about ten times the worst fp32 error of a 64-term dot
# product of O(1) operands (64 * 2^-24 * |terms| ~ 4e-6 per unit of magnitude, and the trunk's own error in front of it).
MARGIN = 1e-4


def case(n, n_items, masked, seed=None):
    """-> dict(arrs, state [n, 20] f32, env_ids, visited (uint32 bitmap, about 30 % set), skip): `masked` adds the last three."""
    seed = 1000 * n + n_items + (7 if masked else 0) if seed is None else seed
    rng = np.random.RandomState(seed)
    arrs = {k: np.asarray(v, np.float32) for k, v in policycase.random_weights(rng, n_items).items()}
    state = rng.normal(0, 1, (n, 20)).astype(np.float32)
    c = dict(arrs=arrs, state=state, env_ids=None, visited=None, skip=None, n=n, n_items=n_items)
    if masked:
        B = n + 3
        words = (n_items + 31) // 32
        bits = rng.uniform(size=(B, words * 32)) < 0.3
        env_ids = rng.permutation(B)[:n].astype(np.int32)
        bits[env_ids[n - 1]] = True                      # the last row keeps only 3 items: a top-7 list has four fills
        bits[env_ids[n - 1], rng.permutation(n_items)[:3]] = False
        c["visited"] = np.packbits(bits.reshape(B, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(B, words)
        c["env_ids"] = env_ids
        skip = np.zeros(n, np.uint8)
        skip[1::4] = 1                                   # rows 1, 5, ... are skipped (none when n == 1) ...
        skip[n - 1] = 0                                  # ... but never the row with 3 items left
        c["skip"] = skip
    return c


def margin_of(z):
    return MARGIN * np.maximum(1.0, np.abs(z))


def check_greedy_ids(got, want, gap, runner_up, z_top, what=""):
    """The issue's rule: equal wherever the float64 top-2 gap exceeds the margin, else one of the two best items."""
    got, want = np.asarray(got), np.asarray(want)
    clear = gap > margin_of(z_top)
    assert np.array_equal(got[clear], want[clear]), (what, np.flatnonzero(clear & (got != want))[:8])
    close = ~clear
    assert ((got[close] == want[close]) | (got[close] == runner_up[close])).all(), what
    return int(close.sum())


def check_topk_ids(got, want_k1, gaps, z, what=""):
    """got [n, k]; want_k1 [n, k + 1] the float64 order of the first k + 1; gaps [n, k + 1] between neighbours.  Rank r must be the reference's
    unless one of its neighbour gaps is inside the margin; then it may be a neighbour's item."""
    n, k = got.shape
    for j in range(n):
        for r in range(k):
            w = want_k1[j, r]
            if got[j, r] == w:
                continue
            assert w >= 0 and got[j, r] >= 0, (what, j, r, got[j], want_k1[j])
            m = margin_of(z[j, w])
            near = [want_k1[j, q] for q in (r - 1, r + 1) if 0 <= q <= k and gaps[j, min(q, r)] <= m]
            assert got[j, r] in near, (what, j, r, got[j, r], w, gaps[j, max(r - 1, 0):r + 1])
