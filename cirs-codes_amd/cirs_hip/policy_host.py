"""float64 restatement of the deterministic policy outputs (cirs_actor_greedy / cirs_actor_topk): what the tests compare the device against.

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
