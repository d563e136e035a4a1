"""float64 numpy restatement of the ranking / list-diversity metrics (cirs_rows_topk / cirs_rank_metrics): what the tests compare the device
against, bit for bit.  It plays the role policy_host.py plays for the arg-max and the policy's top-k list.

Every float64 sum runs in the device's order (include/cirs_hip.h, csrc/rankmetrics.hip):
  dcg / idcg   position (rank) order r = 0 .. k-1
  ild          per first item a the similarities of the pairs (a, b), b = a+1 .. k-1 ascending; the partial sums then added in ascending a
  means        partial t = rows t, t + 256, ... ascending; then a halving tree over the 256 partials
The sums are written as loops over k (or the tree's 8 levels) of element-wise numpy operations over the rows: element-wise float64 `+`, `*`,
`/` are IEEE operations, the same the device executes (its build keeps -ffp-contract=off)."""
import numpy as np

from .policy_host import mask_from_bitmap  # noqa: F401  (re-exported: the bitmap has cirs_actor_topk's meaning)

TOPK_MAX = 32
COLUMNS = ("n_list", "n_rel", "hits", "precision", "recall", "hit", "mrr", "dcg", "idcg", "ndcg", "ild")
MEAN_COLUMNS = (3, 4, 5, 6, 9, 10)          # precision, recall, hit, mrr, ndcg, ild -> sums[2:8]
ERR_ID, ERR_USER = 1, 2
CAT_NONE = 0xFF


def discounts(k=TOPK_MAX):
    """1 / log2(r + 2) for r = 0 .. k-1 in float64: computed once on the host and handed to the device, which takes no logarithm."""
    return 1.0 / np.log2(np.arange(k, dtype=np.float64) + 2.0)


def cat_masks(packed):
    """uint64 category bitmask per item of the packed 4 x u8 categories (cat_mask of csrc/common.h)."""
    p = np.asarray(packed).view(np.uint32).astype(np.uint64)
    m = np.zeros(p.shape, np.uint64)
    for q in range(4):
        c = (p >> np.uint64(8 * q)) & np.uint64(0xFF)
        m |= np.where(c != CAT_NONE, np.uint64(1) << (c & np.uint64(63)), np.uint64(0))
    return m


def popcount(x):
    x = np.asarray(x, np.uint64)
    return np.unpackbits(x.reshape(-1, 1).view(np.uint8), axis=1).sum(axis=1).reshape(x.shape).astype(np.int64)


def topk_rows64(scores, k, masked=None, skip=None):
    """(ids [n, k] int64, vals [n, k] of the table's dtype): value descending, ties to the lower id (np.lexsort on (id, -value)); entries that are
    -inf, NaN or masked are never listed; -1 / -inf fills."""
    s = np.asarray(scores)
    n, I = s.shape
    ids = np.full((n, k), -1, np.int64)
    vals = np.full((n, k), -np.inf, s.dtype)
    for j in range(n):
        if skip is not None and skip[j]:
            continue
        ok = s[j] > -np.inf                         # false for NaN too
        if masked is not None:
            ok &= ~np.asarray(masked[j], bool)
        live = np.flatnonzero(ok)
        order = live[np.lexsort((live, -s[j, live].astype(np.float64)))][:k]
        ids[j, :len(order)] = order
        vals[j, :len(order)] = s[j, order]
    return ids, vals


def rank_metrics64(ids, users, rel, item_cats, k, rel_threshold, masked=None, skip=None):
    """(per_row [n, 11] float64 in COLUMNS order, err [n] int): the first k columns of ids [n, >= k] scored against rel [U, >= I]; item_cats [I]
    packed.  masked [n, I] bool: items left out of n_rel and of the ideal list.  A skipped row and a row with an id / user out of range are zero."""
    ids = np.asarray(ids, np.int64)[:, :k]
    users = np.asarray(users, np.int64)
    rel = np.asarray(rel, np.float64)
    I = len(item_cats)
    n = len(users)
    disc = discounts(TOPK_MAX)
    skipped = np.zeros(n, bool) if skip is None else np.asarray(skip, bool)
    err = np.where(((ids < -1) | (ids >= I)).any(axis=1), ERR_ID, 0) | np.where((users < 0) | (users >= rel.shape[0]), ERR_USER, 0)
    err[skipped] = 0
    live = ~skipped & (err == 0)
    out = np.zeros((n, len(COLUMNS)))
    rows = np.flatnonzero(live)
    if len(rows) == 0:
        return out, err
    L, u = ids[rows], users[rows]
    R = rel[u][:, :I]
    listed = L >= 0
    x = np.where(listed, np.take_along_axis(R, np.where(listed, L, 0), axis=1), 0.0)
    gain = np.where(x > 0.0, x, 0.0)
    hit = listed & (x >= rel_threshold)
    hits = hit.sum(axis=1)
    n_list = listed.sum(axis=1)
    free = np.ones(R.shape, bool) if masked is None else ~np.asarray(masked, bool)[rows]
    n_rel = (free & (R >= rel_threshold)).sum(axis=1)
    dcg = np.zeros(len(rows))
    for r in range(k):
        dcg = dcg + gain[:, r] * disc[r]
    ideal = -np.sort(-np.where(free & (R > 0.0), R, 0.0), axis=1)[:, :k]       # the k largest gains, descending; zeros add nothing
    idcg = np.zeros(len(rows))
    for r in range(ideal.shape[1]):
        idcg = idcg + ideal[:, r] * disc[r]
    cm = np.where(listed, cat_masks(item_cats)[np.where(listed, L, 0)], np.uint64(0))
    sim = np.zeros(len(rows))
    for a in range(k):
        sim_a = np.zeros(len(rows))
        for b in range(a + 1, k):
            uni = popcount(cm[:, a] | cm[:, b])
            pair = listed[:, a] & listed[:, b] & (uni > 0)
            sim_a = sim_a + np.where(pair, popcount(cm[:, a] & cm[:, b]) / np.maximum(uni, 1), 0.0)
        sim = sim + sim_a
    first = np.where(hits > 0, hit.argmax(axis=1) + 1, 1)
    pairs = 0.5 * n_list * (n_list - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[rows, 0], out[rows, 1], out[rows, 2] = n_list, n_rel, hits
        out[rows, 3] = hits / float(k)
        out[rows, 4] = np.where(n_rel > 0, hits / np.maximum(n_rel, 1), 0.0)
        out[rows, 5] = hits > 0
        out[rows, 6] = np.where(hits > 0, 1.0 / first, 0.0)
        out[rows, 7], out[rows, 8] = dcg, idcg
        out[rows, 9] = np.where(idcg > 0.0, dcg / np.where(idcg > 0.0, idcg, 1.0), 0.0)
        out[rows, 10] = np.where(n_list >= 2, 1.0 - sim / np.maximum(pairs, 1.0), 0.0)
    return out, err


def reduce64(per_row, skip=None, err=None):
    """sums [8] = {rows not skipped, error word, means of precision, recall, hit, mrr, ndcg, ild over the rows not skipped} in the order of
    rank_reduce_kernel."""
    per_row = np.asarray(per_row, np.float64)
    n = len(per_row)
    keep = np.ones(n, bool) if skip is None else ~np.asarray(skip, bool)
    part = np.zeros((256, len(MEAN_COLUMNS)))
    vals = np.where(keep[:, None], per_row[:, MEAN_COLUMNS], 0.0)      # a skipped row is not added (its columns are zero anyway)
    for j0 in range(0, n, 256):
        blk = vals[j0:j0 + 256]
        part[:len(blk)] = part[:len(blk)] + blk
    off = 128
    while off > 0:
        part[:off] = part[:off] + part[off:2 * off]
        off >>= 1
    cnt = int(keep.sum())
    word = 0 if err is None else int(np.bitwise_or.reduce(np.asarray(err, np.int64))) if n else 0
    sums = np.zeros(8)
    sums[0], sums[1] = cnt, word
    if cnt > 0:
        sums[2:] = part[0] / float(cnt)
    return sums
