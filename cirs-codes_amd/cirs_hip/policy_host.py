"""float64 restatement of the policy outputs -- deterministic (cirs_actor_greedy / cirs_actor_topk) and sampled (cirs_actor_sample, the
rollout's sampler; second half of the file): what the tests compare the device against.

The rule is the reference's (core/policy/ppo.py:149-151): in eval mode a discrete actor takes `logits_masked.argmax(-1)` over the unmasked
items in ascending id order, so ties go to the lowest id; the top-k list continues that order down the ranking.  logp is
Categorical(probs).log_prob of the masked soft-max with torch's probs_to_logits clamp (float32 eps)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def forward64(arrs, state):
    """(logits [n, I], value [n]) of the 2-layer ReLU trunk, the actor head and the critic head, all in float64."""
    a = {k: np.asarray(v, dtype=np.float64) for k, v in arrs.items()}
    x = np.asarray(state, dtype=np.float64)
    h1 = np.maximum(x @ a["w1"].T + a["b1"], 0.0)
    h2 = np.maximum(h1 @ a["w2"].T + a["b2"], 0.0)
    return h2 @ a["wa"].T + a["ba"], (h2 @ a["wc"].T + a["bc"]).reshape(-1)


def mask_from_bitmap(visited, env_ids, n, n_items):
    """bool [n, I]: item i of row j is masked (bit i of row env_ids[j] of the uint32 bitmap)."""
    if visited is None:
        return np.zeros((n, n_items), dtype=bool)
    bm = np.asarray(visited).view(np.uint32)
    rows = np.arange(n) if env_ids is None else np.asarray(env_ids)
    items = np.arange(n_items)
    return ((bm[rows][:, items >> 5] >> (items & 31).astype(np.uint32)) & 1).astype(bool)


def topk_from_logits(logits, k, masked=None, skip=None):
    """(ids [n, k] int64, logp [n, k] float64, gaps [n, k] float64) from float64 logits.
    Order: logit descending, ties to the lower id; -1 / -inf where fewer than k unmasked items are left or the row is skipped.
    gaps[j, r] = logit of rank r minus logit of rank r + 1 (inf where there is no rank r + 1): how far the r-th choice is from flipping."""
    z = np.asarray(logits, dtype=np.float64)
    n, I = z.shape
    masked = np.zeros((n, I), dtype=bool) if masked is None else np.asarray(masked, dtype=bool)
    ids = np.full((n, k), -1, dtype=np.int64)
    logp = np.full((n, k), -np.inf)
    gaps = np.full((n, k), np.inf)
    for j in range(n):
        if skip is not None and skip[j]:
            continue
        live = np.flatnonzero(~masked[j])
        if len(live) == 0:
            continue
        zl = z[j, live]
        order = live[np.lexsort((live, -zl))]          # primary: -logit ascending, secondary: id ascending
        m = zl.max()
        lse = m + np.log(np.exp(zl - m).sum())
        top = order[:k + 1]
        zs = z[j, top]
        r = min(k, len(order))
        ids[j, :r] = top[:r]
        logp[j, :r] = np.log(np.clip(np.exp(zs[:r] - lse), EPS32, 1.0 - EPS32))
        d = zs[:-1] - zs[1:]
        gaps[j, :len(d)] = d          # (at most k differences: `top` holds k + 1 items)
    return ids, logp, gaps


def greedy64(arrs, state, env_ids=None, visited=None, skip=None):
    """(act [n], logp [n], value [n], gap [n], runner_up [n]): the float64 arg-max, its top-2 gap and the second-best item."""
    z, value = forward64(arrs, state)
    n, I = z.shape
    masked = mask_from_bitmap(visited, env_ids, n, I)
    ids, logp, gaps = topk_from_logits(z, 2, masked, skip)
    value = np.where(np.asarray(skip, dtype=bool), 0.0, value) if skip is not None else value
    return ids[:, 0], logp[:, 0], value, gaps[:, 0], ids[:, 1]


def topk64(arrs, state, k, env_ids=None, visited=None, skip=None):
    z, _ = forward64(arrs, state)
    n, I = z.shape
    ids, logp, gaps = topk_from_logits(z, k, mask_from_bitmap(visited, env_ids, n, I), skip)
    return ids, logp, gaps, z


# ---- the sampled policy step -----------------------------------------------------------------------------------------------------
# float64 restatement of the counter-based two-level Gumbel-max sampler (csrc/rng.h): a chunk of CHUNK consecutive items by
# argmax_c (L_c + G1_c), L_c = log of the chunk's mass over its valid items, then the item inside it by argmax_i (z_i + G2_i).  The noise
# is integer-keyed (Philox4x32-10), so it is the device's bit for bit up to the float64 logs; everything else is plain float64.
CHUNK = 128
STREAM_ACTOR, STREAM_CHUNK = 0x43495253, 0x43484E4B      # 'CIRS', 'CHNK'
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on broadcastable arrays of 32-bit words held in uint64 -> the four output words (uint64 < 2^32)."""
    M0, M1, W0, W1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(32)
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0) & _M32, np.uint64(k1) & _M32
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return c0, c1, c2, c3


def gumbel_noise64(stream, count, envs, seed, rng_step):
    """[len(envs), count] float64: the noise of elements 0 .. count - 1 (items or chunks) of every env: counter (i >> 2, env, rng_step, stream),
    key = the two halves of the 64-bit seed, word i & 3; u = ((x >> 9) + 0.5) 2^-23 and g = -log(-log(u))."""
    envs = np.asarray(envs, dtype=np.int64).astype(np.uint64)
    blocks = np.arange((count + 3) // 4, dtype=np.uint64)
    seed = int(seed)
    words = philox4x32_10(blocks[None, :], envs[:, None], int(rng_step), stream, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    x = np.stack(words, axis=-1).reshape(len(envs), -1)[:, :count]
    u = ((x >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return -np.log(-np.log(u))


def _top2(score):
    """score [..., m] with -inf for absent entries -> (winner, runner_up, winning score, gap) along the last axis: ties to the lowest index,
    winner / runner_up -1 and gap +inf where there is no first / second candidate."""
    first = np.argmax(score, axis=-1)      # the first of equal maxima: the lowest id
    top = np.take_along_axis(score, first[..., None], axis=-1)[..., 0]
    rest = score.copy()
    np.put_along_axis(rest, first[..., None], -np.inf, axis=-1)
    second = np.argmax(rest, axis=-1)
    nxt = np.take_along_axis(rest, second[..., None], axis=-1)[..., 0]
    have1, have2 = np.isfinite(top), np.isfinite(nxt)
    with np.errstate(invalid="ignore"):
        gap = np.where(have2, top - nxt, np.inf)
    return np.where(have1, first, -1), np.where(have2, second, -1), top, gap


def sample64(arrs, state, seed, rng_step, env_ids=None, visited=None, skip=None):
    """The counter-based two-level draw in float64.  -> dict, n rows and C = ceil(I / 128) chunks:
      act [n] the drawn item (-1: skipped row, or no valid item left), value [n] (0 on skipped rows), chunk [n] its chunk (-1 likewise);
      chunk_score / chunk_gap / chunk_runner_up [n]: the winning L_c + G1_c, its distance to the second best chunk (inf: there is none)
      and that chunk (-1);
      item_win / item_runner_up / item_score / item_gap [n, C]: the same of z_i + G2_i inside EVERY chunk, as item ids -- a draw that went
      to the runner-up chunk is judged by that chunk's entries."""
    z, value = forward64(arrs, state)
    n, I = z.shape
    C = (I + CHUNK - 1) // CHUNK
    envs = np.arange(n) if env_ids is None else np.asarray(env_ids)
    valid = ~mask_from_bitmap(visited, env_ids, n, I)
    if skip is not None:
        valid &= ~np.asarray(skip, dtype=bool)[:, None]
        value = np.where(np.asarray(skip, dtype=bool), 0.0, value)
    zv = np.full((n, C * CHUNK), -np.inf)
    zv[:, :I] = np.where(valid, z, -np.inf)
    zc = zv.reshape(n, C, CHUNK)
    M = zc.max(axis=-1)
    some = np.isfinite(M)      # a chunk with no valid item is absent
    with np.errstate(invalid="ignore", divide="ignore"):
        L = np.where(some, M + np.log(np.exp(zc - np.where(some, M, 0.0)[..., None]).sum(axis=-1)), -np.inf)
    chunk, chunk_ru, chunk_score, chunk_gap = _top2(L + gumbel_noise64(STREAM_CHUNK, C, envs, seed, rng_step))
    g2 = gumbel_noise64(STREAM_ACTOR, C * CHUNK, envs, seed, rng_step).reshape(n, C, CHUNK)
    win, ru, item_score, item_gap = _top2(zc + g2)
    base = np.arange(C)[None, :] * CHUNK
    item_win, item_ru = np.where(win >= 0, win + base, -1), np.where(ru >= 0, ru + base, -1)
    act = np.where(chunk >= 0, np.take_along_axis(item_win, np.maximum(chunk, 0)[:, None], axis=1)[:, 0], -1)
    return dict(act=act.astype(np.int64), value=value, chunk=chunk, chunk_score=chunk_score, chunk_gap=chunk_gap, chunk_runner_up=chunk_ru,
                item_win=item_win, item_runner_up=item_ru, item_score=item_score, item_gap=item_gap)


def logp64_at(arrs, state, ids, env_ids=None, visited=None):
    """[n] float64: the masked log-soft-max at the given ids with torch's probs_to_logits clamp (float32 eps), whatever drew them; 0 where
    ids < 0 ("nothing was drawn").  A masked id has probability 0: the clamp makes it log(eps)."""
    z, _ = forward64(arrs, state)
    n, I = z.shape
    ids = np.asarray(ids, dtype=np.int64)
    zv = np.where(mask_from_bitmap(visited, env_ids, n, I), -np.inf, z)
    m = zv.max(axis=1)
    out = np.zeros(n)
    live = (ids >= 0) & np.isfinite(m)
    r = np.flatnonzero(live)
    lse = m[r] + np.log(np.exp(zv[r] - m[r, None]).sum(axis=1))
    out[r] = np.log(np.clip(np.exp(zv[r, ids[r]] - lse), EPS32, 1.0 - EPS32))
    return out


def sample_with_noise64(arrs, state, gumbel, env_ids=None, visited=None, skip=None):
    """The harness-noise path: (act [n], value [n], gap [n], runner_up [n], score [n]) of argmax_i (z_i + g_i) over the valid items, ties to
    the lowest id; act -1 on skipped rows and rows with nothing left."""
    z, value = forward64(arrs, state)
    n, I = z.shape
    valid = ~mask_from_bitmap(visited, env_ids, n, I)
    if skip is not None:
        valid &= ~np.asarray(skip, dtype=bool)[:, None]
        value = np.where(np.asarray(skip, dtype=bool), 0.0, value)
    act, ru, score, gap = _top2(np.where(valid, z + np.asarray(gumbel, dtype=np.float64), -np.inf))
    return act.astype(np.int64), value, gap, ru, score
