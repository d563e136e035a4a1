"""GPU: cirs_rows_topk and cirs_rank_metrics (cirs_hip.rankmetrics.RankMetrics) against the float64 restatement (cirs_hip/rankmetrics_host.py) bit
for bit and against the plain numpy formulas within 1e-12 relative, on the cases of tests/rankcase.py (vetted on the CPU by
tests/test_rankmetrics_cpu.py); then the public entry points PPOPolicy.rank_metrics and UserModel.evaluate_ranking on the synthetic stacks."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import rankcase
from cirs_hip import rankmetrics_host as host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_COLS = slice(3, 11)


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _engine(n, I, masked):
    """The case on the device: computed once, shared by the tests (never modified).  The tables keep their three extra columns (ld = I + 3)."""
    from cirs_hip.rankmetrics import RankMetrics
    c = rankcase.case(n, I, masked)
    rel_wide = _dev(c["rel"])
    rm = RankMetrics(rel_wide[:, :I], c["cats"], rel_threshold=rankcase.REL_THRESHOLD)
    assert rm.rel.data_ptr() == rel_wide.data_ptr() and rm.rel.stride(0) == I + 3, "the relevance table is used in place"
    dev = dict(scores=_dev(c["scores"])[:, :I], users=_dev(c["users"]), env_ids=_dev(c["env_ids"]),
               visited=_dev(None if c["visited"] is None else c["visited"].view(np.int32)), skip=_dev(c["skip"]))
    return c, rm, dev


def _masks(dev):
    return dict(visited=dev["visited"], env_ids=dev["env_ids"], skip=dev["skip"])


@functools.lru_cache(maxsize=None)
def _topk(n, I, masked, k):
    c, rm, dev = _engine(n, I, masked)
    return rm.topk_rows(dev["scores"], k, **_masks(dev))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _sums_of(res, k):
    return np.array([res["n"], 0.0] + [res[f"{m}@{k}"] for m in ("Precision", "Recall", "HR", "MRR", "NDCG", "ILD")])


@pytest.mark.parametrize("k", rankcase.KS)
@pytest.mark.parametrize("n,I,masked", rankcase.SHAPES)
def test_topk_rows_equals_the_restatement(n, I, masked, k):
    c, rm, dev = _engine(n, I, masked)
    ids, vals = _topk(n, I, masked, k)
    assert ids.shape == (n, k) and ids.dtype == torch.int64 and vals.shape == (n, k) and vals.dtype == torch.float32
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    w_ids, w_vals = rankcase.lists(n, I, masked, k)
    assert np.array_equal(ids, w_ids), np.argwhere(ids != w_ids)[:5]
    assert np.array_equal(vals.view(np.uint32), w_vals.view(np.uint32)), "values are the table's bits, fills -inf"
    for j in range(n):                   # no id masked, -inf or twice
        got = ids[j][ids[j] >= 0]
        assert len(set(got.tolist())) == len(got) and (c["scores"][j, got] > -np.inf).all()
        assert not masked or not c["mask"][j, got].any()


@pytest.mark.parametrize("k", rankcase.KS)
@pytest.mark.parametrize("n,I,masked", rankcase.SHAPES)
def test_evaluate_equals_the_restatement_bit_for_bit(n, I, masked, k):
    c, rm, dev = _engine(n, I, masked)
    ids, _ = _topk(n, I, masked, k)
    res = rm.evaluate(ids, dev["users"], **_masks(dev))
    assert set(res) == {f"{m}@{k}" for m in ("Precision", "Recall", "HR", "MRR", "NDCG", "ILD", "CV")} | {"n", "per_row"}
    per_row = res["per_row"].cpu().numpy()
    ids_h = ids.cpu().numpy()
    w_row, w_err = host.rank_metrics64(ids_h, c["users"], c["rel"][:, :I], c["packed"], k, rankcase.REL_THRESHOLD, c["mask"], c["skip"])
    w_sums = host.reduce64(w_row, c["skip"], w_err)
    assert not w_err.any()
    assert np.array_equal(per_row[:, :3], w_row[:, :3]), "the integer columns"
    _same_bits(per_row[:, FLOAT_COLS], w_row[:, FLOAT_COLS], f"per_row {n}x{I} k={k}")
    _same_bits(_sums_of(res, k), w_sums, f"means {n}x{I} k={k}")
    plain, plain_sums = rankcase.plain_metrics(ids_h, c["users"], c["rel"][:, :I], c["cats"], k, rankcase.REL_THRESHOLD, c["mask"], c["skip"])
    assert np.array_equal(per_row[:, :3], plain[:, :3])
    rankcase.assert_close_plain(per_row[:, FLOAT_COLS], plain[:, FLOAT_COLS], f"per_row {n}x{I} k={k}")
    rankcase.assert_close_plain(_sums_of(res, k), plain_sums, f"means {n}x{I} k={k}")
    listed = ids_h[ids_h >= 0]
    assert res[f"CV@{k}"] == len(set(listed.tolist())) / I
    # properties
    ndcg = per_row[:, 9]
    assert ((ndcg >= 0) & (ndcg <= 1)).all()
    none = per_row[:, 1] == 0
    assert not per_row[none][:, [4, 5, 6]].any(), "a row without relevant items has recall, hit and mrr 0"
    if k == 1:
        assert not per_row[:, 10].any(), "a list of one item has no diversity"
    if masked:
        sk = c["skip"].astype(bool)
        assert not per_row[sk].any() and res["n"] == n - sk.sum()
        if n > 1:
            assert per_row[0, 1] == 0 and per_row[n - 1, 0] <= 3      # every relevant item masked; three items left


@pytest.mark.parametrize("n,I,masked", [(37, 130, False), (37, 130, True), (5, 20, True)])
def test_the_ideal_list_scores_one(n, I, masked):
    """A list in the row's ideal order (relevance as the score) has dcg == idcg bit for bit and ndcg == 1.0."""
    c, rm, dev = _engine(n, I, masked)
    k = 7
    # relevance as the score: rounding one-decimal values to float32 keeps their order and their ties, so the lists are in the float64 order
    gains = rm.rel[dev["users"].long()].float()
    ids, _ = rm.topk_rows(gains.contiguous(), k, **_masks(dev))
    per_row = rm.evaluate(ids, dev["users"], **_masks(dev))["per_row"].cpu().numpy()
    live = per_row[:, 8] > 0
    assert live.sum() >= 1
    assert np.array_equal(_bits(per_row[live, 7]), _bits(per_row[live, 8])) and (per_row[live, 9] == 1.0).all()


def test_all_rows_skipped_and_nan_scores():
    c, rm, dev = _engine(5, 20, True)
    ids, _ = _topk(5, 20, True, 7)
    every = torch.ones(5, dtype=torch.uint8, device="cuda")
    res = rm.evaluate(ids, dev["users"], visited=dev["visited"], env_ids=dev["env_ids"], skip=every)
    assert res["n"] == 0 and not res["per_row"].any() and res["CV@7"] == 0.0
    assert all(res[f"{m}@7"] == 0.0 for m in ("Precision", "Recall", "HR", "MRR", "NDCG", "ILD"))
    s = torch.tensor([[1.0, float("nan"), 3.0, 3.0, float("-inf")] + [float("nan")] * 15], device="cuda")
    ids, vals = rm.topk_rows(s, 4)
    assert ids.tolist() == [[2, 3, 0, -1]] and vals[0, :3].tolist() == [3.0, 3.0, 1.0] and bool(torch.isneginf(vals[0, 3]))


@pytest.mark.parametrize("n,I,masked", [(130, 300, True), (37, 130, False)])
def test_a_prefix_is_scored_in_place(n, I, masked):
    c, rm, dev = _engine(n, I, masked)
    ids32, _ = _topk(n, I, masked, 32)
    ids7, _ = _topk(n, I, masked, 7)
    assert torch.equal(ids32[:, :7], ids7)
    a = rm.evaluate(ids32, dev["users"], k=7, **_masks(dev))
    b = rm.evaluate(ids7, dev["users"], **_masks(dev))
    assert torch.equal(a["per_row"].view(torch.int64), b["per_row"].view(torch.int64))
    assert {k: v for k, v in a.items() if k != "per_row"} == {k: v for k, v in b.items() if k != "per_row"}


def test_an_id_out_of_range_is_reported_not_used():
    n, I, k = 37, 130, 7
    c, rm, dev = _engine(n, I, False)
    ids, _ = _topk(n, I, False, k)
    good = rm.evaluate(ids, dev["users"])["per_row"]
    bad = ids.clone()
    bad[11, 3] = I                                       # one past the catalogue
    with pytest.raises(ValueError, match="outside") as info:
        rm.evaluate(bad, dev["users"])
    per_row = info.value.per_row
    rows = torch.arange(n, device="cuda") != 11
    assert torch.equal(per_row[rows].view(torch.int64), good[rows].view(torch.int64)) and not per_row[11].any()
    users = dev["users"].clone()
    users[2] = rankcase.N_USERS
    with pytest.raises(ValueError, match="user outside"):
        rm.evaluate(ids, users)
    again = rm.evaluate(ids, dev["users"])["per_row"]    # the engine goes on working
    assert torch.equal(again.view(torch.int64), good.view(torch.int64))


# ---- the public entry points on the synthetic stacks ------------------------------------------------------------------------------
@pytest.fixture()
def _global_generators_left_as_found():
    """Module constructors draw initial weights from torch's global CPU generator and fit_data its permutations from the CUDA one: put both
    back, so the tests that run after this file see the streams they saw before it existed."""
    cpu, gpu, npy = torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu)
    np.random.set_state(npy)


PPO_ARGS = ["--n-users", "100", "--n-items", "300", "--training-num", "16", "--episode-per-collect", "16", "--test-num", "8", "--batch-size", "64",
            "--max_turn", "12", "--tau", "10", "--dropout", "0", "--force_length", "5", "--leave_threshold", "0", "--num_leave_compute", "1",
            "--epoch", "1", "--step-per-epoch", "60"]


def test_ppo_policy_rank_metrics(_global_generators_left_as_found):
    from cirs_hip.rankmetrics import RankMetrics
    from tianshou.data import Batch
    spec = importlib.util.spec_from_file_location("cirs_rl_kuaishou_synth", os.path.join(ROOT, "examples", "cirs_rl_kuaishou_synth.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    args = ex.get_args(PPO_ARGS)
    tab, envs, st, policy, coll = ex.build(args)
    env = ex.gym.make(args.env)
    k, thr = 10, 3.0
    users = np.random.RandomState(5).randint(0, 100, 16)
    rm = RankMetrics.for_env(env, rel_threshold=thr)
    assert rm.rel.data_ptr() == env.device_tables().mat.data_ptr()
    obs = torch.randn(16, 20, generator=torch.Generator().manual_seed(1))
    got = policy.rank_metrics(Batch(obs=obs), users, env, k, rel_threshold=thr)
    top = policy.topk(Batch(obs=obs), k)
    want = rm.evaluate(top.act, users)
    assert torch.equal(got["per_row"].view(torch.int64), want["per_row"].view(torch.int64))
    assert {n: v for n, v in got.items() if n != "per_row"} == {n: v for n, v in want.items() if n != "per_row"} and got["n"] == 16
    w_row, w_err = host.rank_metrics64(top.act.cpu().numpy(), users, tab.mat, rm.item_cats.cpu().numpy(), k, thr)
    _same_bits(got["per_row"].cpu().numpy(), w_row, "PPOPolicy.rank_metrics")
    _same_bits(_sums_of(got, k), host.reduce64(w_row, None, w_err), "PPOPolicy.rank_metrics means")
    assert 0 < got[f"CV@{k}"] <= 16 * k / 300 and 0 <= got[f"NDCG@{k}"] <= 1
    # remove_recommended_ids: the bitmap of the running episodes masks the list, n_rel and the ideal list alike
    buf = _RunningEpisodes(np.random.RandomState(6).randint(0, 300, (16, 3)))
    got = policy.rank_metrics(Batch(obs=obs), users, env, k, rel_threshold=thr, buffer=buf, remove_recommended_ids=True)
    _, env_ids, visited = policy._rows(Batch(obs=obs), buf, True)
    assert visited is not None and bool(visited.any())
    top = policy.topk(Batch(obs=obs), k, buffer=buf, remove_recommended_ids=True)
    want = rm.evaluate(top.act, users, visited=visited, env_ids=env_ids)
    assert torch.equal(got["per_row"].view(torch.int64), want["per_row"].view(torch.int64))
    assert {n: v for n, v in got.items() if n != "per_row"} == {n: v for n, v in want.items() if n != "per_row"}
    mask = host.mask_from_bitmap(visited.cpu().numpy(), env_ids.cpu().numpy(), 16, 300)
    assert mask[np.arange(16)[:, None], buf.act.reshape(16, 3)].all() and mask.sum() <= 16 * 3
    w_row, _ = host.rank_metrics64(top.act.cpu().numpy(), users, tab.mat, rm.item_cats.cpu().numpy(), k, thr, masked=mask)
    _same_bits(got["per_row"].cpu().numpy(), w_row, "PPOPolicy.rank_metrics, masked")
    assert not mask[np.arange(16)[:, None], top.act.cpu().numpy()].any()
    with pytest.raises(ValueError, match="rel_threshold"):
        policy.rank_metrics(Batch(obs=obs), users, env, k)


class _RunningEpisodes:
    """What PPOPolicy reads of a replay buffer to find the items of the running episodes (core/policy/utils.py:7-27): n unfinished episodes of
    T recommendations each, stored one after the other."""

    def __init__(self, acts):
        n, self._T = acts.shape
        self.act = acts.reshape(-1).astype(np.int64)
        self.done = np.zeros(n * self._T, bool)
        self._lengths = np.full(n, self._T)
        self.last_index = np.arange(n) * self._T + self._T - 1

    def __len__(self):
        return len(self.act)

    def prev(self, idx):
        return np.where(idx % self._T == 0, idx, idx - 1)


@pytest.fixture(scope="module")
def workspace(tmp_path_factory):
    from cirs_hip.synthetic import write_kuairec_workspace
    from environments.KuaishouRec.env.kuaishouEnv import KuaishouEnv
    root = str(tmp_path_factory.mktemp("rank") / "data")
    write_kuairec_workspace(root, n_users=30, n_items=1400, n_env_users=16, n_env_items=60, log_len=(20, 40), seed=3)
    env = KuaishouEnv(*KuaishouEnv.load_mat(root), num_leave_compute=1, leave_threshold=0, max_turn=10)
    return root, env


def _check_model(model, env, val_set, k=10, thr=1.0):
    import evaluation
    from functools import partial
    U, I = env.mat.shape
    res = model.evaluate_ranking(env, val_set, k, rel_threshold=thr)
    assert res["n"] == U and res["ids"].shape == (U, k) and res["per_row"].shape == (U, 11)
    # the restatement on the read-back sweep scores
    df = val_set.df_photo_env
    scores, _ = model.device_model().sweep(np.asarray(env.lbe_user.classes_), df.index.to_numpy(), df[["feat0", "feat1", "feat2", "feat3"]].to_numpy(),
                                           df["photo_duration"].to_numpy())
    w_ids, _ = host.topk_rows64(scores.cpu().numpy(), k)
    assert np.array_equal(res["ids"].cpu().numpy(), w_ids)
    from cirs_hip.synthetic import pack_item_cats
    w_row, w_err = host.rank_metrics64(w_ids, np.arange(U), env.mat, pack_item_cats(env.item_cats()), k, thr)
    _same_bits(res["per_row"].cpu().numpy(), w_row, "evaluate_ranking")
    _same_bits(_sums_of(res, k), host.reduce64(w_row, None, w_err), "evaluate_ranking means")
    # two calls, blocks of 7 users and one block, and the evaluation function give the same bits
    for other in (model.evaluate_ranking(env, val_set, k, rel_threshold=thr), model.evaluate_ranking(env, val_set, k, rel_threshold=thr, batch_users=7),
                  model.evaluate_ranking(env, val_set, k, rel_threshold=thr, batch_users=U),
                  partial(evaluation.test_ranking_kuaishou, env=env, dataset_val=val_set, k=k, rel_threshold=thr)(model)):
        assert torch.equal(other["per_row"].view(torch.int64), res["per_row"].view(torch.int64)) and torch.equal(other["ids"], res["ids"])
        assert {n: v for n, v in other.items() if n not in ("per_row", "ids")} == {n: v for n, v in res.items() if n not in ("per_row", "ids")}
    some = np.array([5, 0, 5, 11])
    part = model.evaluate_ranking(env, val_set, k, rel_threshold=thr, users=some)
    assert torch.equal(part["per_row"].view(torch.int64), res["per_row"][torch.as_tensor(some).cuda()].view(torch.int64))
    with pytest.raises(ValueError, match="rel_threshold"):
        model.evaluate_ranking(env, val_set, k)


def test_pairwise_evaluate_ranking(workspace, tmp_path, _global_generators_left_as_found):
    from core.user_model_train import train_user_model
    root, env = workspace
    run = train_user_model(root, save_root=str(tmp_path), tau=800.0, feature_dim=8, batch_size=64, epoch=1, lr=5e-3)
    _check_model(run.model, env, run.val_set)


def test_dice_evaluate_ranking(workspace, tmp_path, _global_generators_left_as_found):
    from core.user_model_train import train_dice_kuaishou
    root, env = workspace
    run = train_dice_kuaishou(root, save_root=str(tmp_path), feature_dim=8, batch_size=64, epoch=1, lr=5e-3)
    _check_model(run.model, env, run.val_set)
