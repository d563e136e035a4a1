"""Shared inputs and plain-numpy formulas of the ranking-metric tests (cirs_rows_topk / cirs_rank_metrics): the cases the CPU tests vet are the
ones the GPU tests run.  Rows 1 / 5 / 37 / 130: one row, a partial and several workgroups of four rows (37 and 130 are no multiples of 4);
catalogues 20 (fewer items than k = 32), 130 (crosses 128, no multiple of 32 or 64), 300; k 1 / 7 / 32.  Scores and relevance are rounded
to one decimal so that ties are everywhere; about 5 % of the scores are -inf; the tables are three columns wider than the catalogue (ld = I + 3)."""
import functools

import numpy as np

from cirs_hip import rankmetrics_host as host

ROWS, CATALOGUES, KS = (1, 5, 37, 130), (20, 130, 300), (1, 7, 32)
N_USERS, N_CATS, REL_THRESHOLD = 9, 12, 2.0
SHAPES = [(n, I, masked) for n in ROWS for I in CATALOGUES for masked in (False, True)]
RTOL_PLAIN = 1e-12      # ordered sums against np.sum / np.mean: at most 496 non-negative float64 terms per sum, 2 * 496 * 2^-53 = 1.1e-13 at worst


@functools.lru_cache(maxsize=None)
def case(n, n_items, masked):
    """-> dict(scores [n, I + 3] f32, rel [U, I + 3] f64, cats [I, 4] int32 (-1 = none), packed [I] uint32, users [n] int32 (repeating),
    env_ids, visited (uint32 bitmap, about 30 % set), skip): `masked` adds the last three.  Never modified by a test."""
    from cirs_hip.synthetic import pack_item_cats
    rng = np.random.RandomState(5000 * n + 10 * n_items + (3 if masked else 0))
    I, ld = n_items, n_items + 3
    scores = np.round(rng.normal(0.0, 1.0, (n, ld)), 1).astype(np.float32)
    scores[:, :I][rng.uniform(size=(n, I)) < 0.05] = -np.inf
    scores[:, I:] = 9.0                                  # past the catalogue: would win every list if it were read
    rel = np.round(rng.normal(1.5, 1.5, (N_USERS, ld)), 1)
    rel[:, I:] = 7.0
    n_cat = rng.randint(0, 5, I)
    order = np.argsort(rng.uniform(size=(I, N_CATS)), axis=1)[:, :4]
    cats = np.where(np.arange(4)[None, :] < n_cat[:, None], order, -1).astype(np.int32)      # a fifth of the items has no category
    users = rng.randint(0, N_USERS, n).astype(np.int32)
    c = dict(n=n, n_items=I, scores=scores, rel=rel, cats=cats, packed=pack_item_cats(cats), users=users, env_ids=None, visited=None, skip=None,
             mask=None)
    if masked:
        B, words = n + 3, (I + 31) // 32
        bits = rng.uniform(size=(B, words * 32)) < 0.3
        env_ids = rng.permutation(B)[:n].astype(np.int32)
        bits[env_ids[n - 1]] = True                      # the last row keeps only 3 items: a top-7 list has four fills
        bits[env_ids[n - 1], rng.permutation(I)[:3]] = False
        if n > 1:                                        # row 0: every relevant item of its user is masked -> n_rel = 0
            bits[env_ids[0], :I] |= rel[users[0], :I] >= REL_THRESHOLD
        c["visited"] = np.packbits(bits.reshape(B, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(B, words)
        c["env_ids"] = env_ids
        skip = np.zeros(n, np.uint8)
        skip[1::4] = 1                                   # rows 1, 5, ... are skipped (none when n == 1) ...
        skip[n - 1] = 0                                  # ... but never the row with 3 items left
        c["skip"] = skip
        c["mask"] = host.mask_from_bitmap(c["visited"], env_ids, n, I)
    return c


@functools.lru_cache(maxsize=None)
def lists(n, n_items, masked, k):
    """The float64 restatement's top-k lists of the case (ids, vals): computed once, shared."""
    c = case(n, n_items, masked)
    return host.topk_rows64(c["scores"][:, :n_items], k, c["mask"], c["skip"])


@functools.lru_cache(maxsize=None)
def restated(n, n_items, masked, k):
    """(per_row, err, sums) of the restatement on its own lists."""
    c = case(n, n_items, masked)
    ids, _ = lists(n, n_items, masked, k)
    per_row, err = host.rank_metrics64(ids, c["users"], c["rel"][:, :n_items], c["packed"], k, REL_THRESHOLD, c["mask"], c["skip"])
    return per_row, err, host.reduce64(per_row, c["skip"], err)


def plain_metrics(ids, users, rel, cats, k, rel_threshold, mask=None, skip=None):
    """The textbook formulas with np.sum / np.mean, row by row: (per_row [n, 11], sums [8])."""
    n, I = len(users), rel.shape[1]
    disc = 1.0 / np.log2(np.arange(k) + 2.0)
    out = np.zeros((n, 11))
    sets = [set(int(x) for x in row if x >= 0) for row in cats]
    for j in range(n):
        if skip is not None and skip[j]:
            continue
        r = rel[users[j]]
        free = np.ones(I, bool) if mask is None else ~mask[j]
        lst = ids[j, :k]
        pos = np.flatnonzero(lst >= 0)
        items = lst[pos]
        hit = r[items] >= rel_threshold
        n_rel = int((free & (r >= rel_threshold)).sum())
        dcg = float(np.sum(np.maximum(r[items], 0.0) * disc[pos]))
        ideal = np.sort(np.maximum(r[free], 0.0))[::-1][:k]
        idcg = float(np.sum(ideal * disc[:len(ideal)]))
        sims = [(len(sets[a] & sets[b]) / len(sets[a] | sets[b])) if (sets[a] | sets[b]) else 0.0
                for q, a in enumerate(items) for b in items[q + 1:]]
        out[j] = [len(items), n_rel, hit.sum(), hit.sum() / k, hit.sum() / n_rel if n_rel else 0.0, float(hit.any()),
                  1.0 / (pos[np.argmax(hit)] + 1) if hit.any() else 0.0, dcg, idcg, dcg / idcg if idcg > 0 else 0.0,
                  1.0 - float(np.mean(sims)) if len(items) >= 2 else 0.0]
    keep = np.ones(n, bool) if skip is None else ~np.asarray(skip, bool)
    sums = np.zeros(8)
    sums[0] = keep.sum()
    if keep.any():
        sums[2:] = np.mean(out[keep][:, list(host.MEAN_COLUMNS)], axis=0)
    return out, sums


def assert_close_plain(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bar = RTOL_PLAIN * np.abs(want)
    worst = float((err[want != 0] / np.abs(want[want != 0])).max()) if (want != 0).any() else 0.0
    print(f"{what}: largest relative difference to the plain formula {worst:.3g}")
    assert (err <= bar).all(), (what, worst)
