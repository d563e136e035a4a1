"""CPU: the float64 restatement of the ranking metrics (cirs_hip/rankmetrics_host.py) on an example worked out by hand and against the plain
numpy formulas, the argument validation of cirs_rows_topk / cirs_rank_metrics (no launch), and the Python layer's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import rankcase
from cirs_hip import abi
from cirs_hip import rankmetrics_host as host


def _err():
    return abi.lib().cirs_last_error()


# ---- the restatement on hand-made cases ------------------------------------------------------------------------------------------
D1 = 1.0 / np.log2(3.0)      # the discount of rank 1 (rank 0: 1, rank 2: 1 / log2(4) = 0.5)
# five items; categories: item 0 {0, 1}, item 1 {1}, item 2 none, item 3 {2}, item 4 {0, 1, 2}
CATS = np.array([[0, 1, -1, -1], [1, -1, -1, -1], [-1, -1, -1, -1], [2, -1, -1, -1], [0, 1, 2, -1]], np.int32)
REL = np.array([[3.0, 0.0, 1.0, 2.0, -1.0],
                [0.5, 0.0, 0.0, 1.0, -2.0]])


def _packed(cats):
    from cirs_hip.synthetic import pack_item_cats
    return pack_item_cats(cats)


def test_restatement_on_a_two_row_example_worked_out_by_hand():
    ids = np.array([[3, 1, 0], [4, 2, -1]], np.int64)
    per_row, err = host.rank_metrics64(ids, np.array([0, 1]), REL, _packed(CATS), 3, 2.0)
    assert err.tolist() == [0, 0]
    # row 0: items 3, 1, 0 have relevance 2, 0, 3; the relevant items of the user are 0 and 3; pairs (3,1) 0, (3,0) 0, (1,0) 1/2
    want0 = dict(n_list=3, n_rel=2, hits=2, precision=2 / 3, recall=1.0, hit=1.0, mrr=1.0, dcg=2.0 + 0.0 * D1 + 3.0 * 0.5,
                 idcg=3.0 + 2.0 * D1 + 1.0 * 0.5, ild=1.0 - (0.0 + 0.0 + 0.5) / 3.0)
    want0["ndcg"] = want0["dcg"] / want0["idcg"]
    # row 1: items 4, 2 and a fill; relevance -2 (gain 0) and 0; nothing is relevant; the ideal list is 1, 0.5; the pair (4, 2) shares nothing
    want1 = dict(n_list=2, n_rel=0, hits=0, precision=0.0, recall=0.0, hit=0.0, mrr=0.0, dcg=0.0, idcg=1.0 + 0.5 * D1, ndcg=0.0, ild=1.0)
    for j, want in enumerate((want0, want1)):
        for q, name in enumerate(host.COLUMNS):
            np.testing.assert_allclose(per_row[j, q], want[name], rtol=1e-15, atol=0, err_msg=f"row {j} {name}")
    sums = host.reduce64(per_row)
    assert sums[0] == 2 and sums[1] == 0
    np.testing.assert_allclose(sums[2:], [(2 / 3) / 2, 0.5, 0.5, 0.5, want0["ndcg"] / 2, (want0["ild"] + 1.0) / 2], rtol=1e-15)
    # the first hit at rank 3; a list of one item; two items without a category (empty union: similarity 0)
    per_row, _ = host.rank_metrics64(np.array([[1, 2, 0], [0, -1, -1], [2, 2, -1]], np.int64), np.array([0, 0, 0]), REL, _packed(CATS), 3, 2.0)
    assert per_row[0, 6] == 1 / 3 and per_row[0, 2] == 1
    assert per_row[1, 10] == 0.0 and per_row[1, 0] == 1 and per_row[1, 9] == 3.0 / (3.0 + 2.0 * D1 + 0.5)
    assert per_row[2, 10] == 1.0
    # the mask leaves n_rel and the ideal list: without item 0 the user's best gains are 2, 1
    mask = np.zeros((1, 5), bool)
    mask[0, 0] = True
    per_row, _ = host.rank_metrics64(np.array([[3, 1, 2]], np.int64), np.array([0]), REL, _packed(CATS), 3, 2.0, masked=mask)
    assert per_row[0, 1] == 1 and per_row[0, 8] == 2.0 + 1.0 * D1 and per_row[0, 4] == 1.0


def test_restatement_skips_rows_and_flags_ids_and_users_out_of_range():
    ids = np.array([[3, 1, 0], [3, 1, 5], [3, 1, 0], [3, -2, 0], [3, 1, 0]], np.int64)
    users = np.array([0, 0, 2, 1, -1])
    per_row, err = host.rank_metrics64(ids, users, REL, _packed(CATS), 3, 2.0, skip=np.array([1, 0, 0, 0, 0]))
    assert err.tolist() == [0, host.ERR_ID, host.ERR_USER, host.ERR_ID, host.ERR_USER] and not per_row.any()
    sums = host.reduce64(per_row, np.array([1, 0, 0, 0, 0]), err)
    assert sums[0] == 4 and sums[1] == (host.ERR_ID | host.ERR_USER)
    # every row skipped: n = 0 and the means are 0
    per_row, err = host.rank_metrics64(ids[:1], users[:1], REL, _packed(CATS), 3, 2.0, skip=np.array([1]))
    assert not host.reduce64(per_row, np.array([1]), err).any()


def test_restatement_topk_order_ties_fills_and_what_is_never_listed():
    s = np.array([[1.0, 3.0, 3.0, -np.inf, np.nan, 2.0], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]], np.float32)
    ids, vals = host.topk_rows64(s, 4)
    assert ids.tolist() == [[1, 2, 5, 0], [0, 1, 2, 3]] and vals[0].tolist() == [3.0, 3.0, 2.0, 1.0] and vals.dtype == np.float32
    mask = np.zeros((2, 6), bool)
    mask[0, 1] = True
    ids, vals = host.topk_rows64(s, 4, mask, skip=np.array([0, 1]))
    assert ids.tolist() == [[2, 5, 0, -1], [-1] * 4] and np.isneginf(vals[0, 3]) and np.isneginf(vals[1]).all()
    assert host.discounts(3).tolist() == [1.0, D1, 0.5]
    assert host.cat_masks(_packed(CATS)).tolist() == [3, 2, 0, 4, 7]
    assert host.popcount(np.array([0, 7, 1 << 63], np.uint64)).tolist() == [0, 3, 1]


@pytest.mark.parametrize("k", rankcase.KS)
@pytest.mark.parametrize("n,I,masked", rankcase.SHAPES)
def test_restatement_ordered_sums_against_plain_numpy(n, I, masked, k):
    c = rankcase.case(n, I, masked)
    ids, vals = rankcase.lists(n, I, masked, k)
    # the lists themselves: no id masked, -inf or twice; values descending; as many as there are candidates
    for j in range(n):
        got = ids[j][ids[j] >= 0]
        ok = c["scores"][j, :I] > -np.inf
        if masked:
            ok &= ~c["mask"][j]
        want_len = 0 if (masked and c["skip"][j]) else min(k, int(ok.sum()))
        assert len(got) == want_len and len(set(got.tolist())) == len(got) and ok[got].all() and (ids[j, len(got):] == -1).all()
        assert (np.diff(vals[j, :len(got)]) <= 0).all()
    per_row, err, sums = rankcase.restated(n, I, masked, k)
    assert not err.any()
    plain, plain_sums = rankcase.plain_metrics(ids, c["users"], c["rel"][:, :I], c["cats"], k, rankcase.REL_THRESHOLD, c["mask"], c["skip"])
    assert np.array_equal(per_row[:, :3], plain[:, :3])            # the integer columns
    rankcase.assert_close_plain(per_row[:, 3:], plain[:, 3:], f"per_row {n}x{I} k={k}")
    rankcase.assert_close_plain(sums, plain_sums, f"means {n}x{I} k={k}")
    assert ((per_row[:, 9] >= 0) & (per_row[:, 9] <= 1)).all()
    if masked:
        assert (~c["mask"][n - 1]).sum() == 3 and not per_row[c["skip"].astype(bool)].any()
        if n > 1:
            assert per_row[0, 1] == 0 and per_row[0, 4] == 0 and per_row[0, 6] == 0         # the row without relevant items


# ---- host-side validation: every refusal happens before any launch ------------------------------------------------------------------
def test_rows_topk_validates_before_any_launch():
    lib = abi.lib()
    call = lambda k=7, n=5, I=130, ld=133, scores=8, ids=8: lib.cirs_rows_topk(scores, n, I, ld, k, None, None, None, ids, None, None)   # noqa: E731
    for k in (0, 33, -1):
        assert call(k=k) == -1 and b"k must lie in 1..32" in _err(), k
    assert call(ld=129) == -1 and b"ld < n_items" in _err()
    assert call(I=0, ld=0) == -1 and b"n_items" in _err()
    assert call(scores=None) == -1 and b"null" in _err()
    assert call(ids=None) == -1 and b"null" in _err()
    assert call(n=0, scores=None, ids=None) == 0                 # empty batch


def _rank_cfg(**kw):
    cfg = abi.RankCfg(n_users=9, n_items=130, k=7, rel_threshold=2.0)
    for name, v in kw.items():
        setattr(cfg, name, v)
    return cfg


def test_rank_metrics_validates_before_any_launch():
    lib = abi.lib()
    need = lib.cirs_rank_metrics_workspace_bytes(5)
    assert need >= 5 * 4 and lib.cirs_rank_metrics_workspace_bytes(0) == 0 and lib.cirs_rank_metrics_workspace_bytes(-3) == 0

    def call(cfg=None, n=5, ld_ids=7, ld_rel=133, ws_bytes=need, **ptrs):
        p = dict(ids=8, users=8, rel=8, item_cats=8, per_row=8, sums=8, ws=8)
        p.update(ptrs)
        cfg = _rank_cfg() if cfg is None else cfg
        return lib.cirs_rank_metrics(C.byref(cfg), p["ids"], ld_ids, p["users"], n, p["rel"], ld_rel, p["item_cats"], None, None, None,
                                     p["per_row"], p["sums"], p["ws"], ws_bytes, None)
    assert lib.cirs_rank_metrics(None, 8, 7, 8, 5, 8, 133, 8, None, None, None, 8, 8, 8, need, None) == -1 and b"null cfg" in _err()
    for k in (0, 33, -1):
        assert call(_rank_cfg(k=k), ld_ids=40) == -1 and b"k must lie in 1..32" in _err(), k
    assert call(ld_ids=6) == -1 and b"ld_ids < k" in _err()
    assert call(ld_rel=129) == -1 and b"ld_rel < n_items" in _err()
    assert call(_rank_cfg(n_users=0)) == -1 and b"n_users" in _err()
    assert call(_rank_cfg(n_items=0), ld_rel=0) == -1 and b"n_items" in _err()
    for name in ("ids", "users", "rel", "item_cats", "per_row", "sums", "ws"):
        assert call(**{name: None}) == -1 and b"null" in _err(), name
    assert call(ws_bytes=need - 1) == -1 and b"workspace too small" in _err()
    assert call(n=0, ws_bytes=0, ws=None) == 0                   # empty batch
    assert C.sizeof(abi.RankCfg) == 4 * 4 + 8 + 8 * abi.TOPK_MAX


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_bad_arguments():
    from cirs_hip.rankmetrics import RankMetrics
    c = rankcase.case(5, 20, False)
    rel, cats = torch.as_tensor(c["rel"][:, :20].copy()), c["cats"]
    with pytest.raises(ValueError, match="rel_threshold"):
        RankMetrics(rel, cats, device="cpu")
    with pytest.raises(ValueError, match="rel_threshold"):
        RankMetrics.for_env(None)
    with pytest.raises(ValueError, match="item_cats"):
        RankMetrics(rel, cats[:19], rel_threshold=2.0, device="cpu")
    rm = RankMetrics(rel, cats, rel_threshold=2.0, device="cpu")      # host tensors: enough for every check in front of a launch
    assert rm.rel.data_ptr() == rel.data_ptr(), "a float64 table on the engine's device is used as it is"
    scores, ids = torch.zeros(5, 20), torch.zeros((5, 7), dtype=torch.int64)
    for k in (0, 33, 2.5):
        with pytest.raises(ValueError, match="1..32"):
            rm.topk_rows(scores, k)
        with pytest.raises(ValueError, match="1..32"):
            rm.evaluate(ids, np.zeros(5), k=k)
    with pytest.raises(ValueError, match="1..32"):
        rm.evaluate(torch.zeros((5, 33), dtype=torch.int64), np.zeros(5))
    with pytest.raises(ValueError, match="exceeds"):
        rm.evaluate(ids, np.zeros(5), k=8)
    with pytest.raises(ValueError, match="users has 4 rows"):
        rm.evaluate(ids, np.zeros(4))
    with pytest.raises(ValueError, match="skip has 6 rows"):
        rm.evaluate(ids, np.zeros(5), skip=np.zeros(6, np.uint8))
    with pytest.raises(ValueError, match="skip has 3 rows"):
        rm.topk_rows(scores, 7, skip=np.zeros(3, np.uint8))
    with pytest.raises(ValueError, match="bitmap"):
        rm.topk_rows(scores, 7, visited=torch.zeros((5, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="visited has 4 rows"):
        rm.topk_rows(scores, 7, visited=torch.zeros((4, 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="float32"):
        rm.topk_rows(scores[:, :19], 7)
    with pytest.raises(ValueError, match="int64"):
        rm.evaluate(ids.int(), np.zeros(5))
    # the public entry points check k and the threshold before they touch a device
    from core.policy.ppo import PPOPolicy
    from core.user_model import UserModel
    import evaluation
    for k in (0, 33):
        with pytest.raises(ValueError, match="1..32"):
            PPOPolicy.rank_metrics(object.__new__(PPOPolicy), None, None, None, k, rel_threshold=2.0)
        with pytest.raises(ValueError, match="1..32"):
            UserModel.evaluate_ranking(object.__new__(UserModel), None, None, k, rel_threshold=2.0)
        with pytest.raises(ValueError, match="1..32"):
            evaluation.test_ranking_kuaishou(object.__new__(UserModel), None, None, k, rel_threshold=2.0)
