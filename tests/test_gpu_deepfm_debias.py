"""GPU: the two Kuaishou debiasing baselines on the device -- the IPS / PD loss kinds of the DeepFM training step and the whole-pass
entry cirs_deepfm_train_epoch against the reference recordings (tests/golden/usertrain_debias.npz), the step entry and the host
restatement; the score kernels cirs_item_bin_counts / cirs_item_bin_gather against the recorded score columns; the training run."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import debiascase
import traincase

pytestmark = pytest.mark.gpu


def _np(sd):
    return {k: v.cpu().numpy() for k, v in sd.items()}


def _run_steps(c, kind, x, y, score, n, steps, **kw):
    """`steps` step() calls on consecutive batches of n rows -> ([steps, 5] losses, parameters after the first step, final, trainer)."""
    from cirs_hip.deepfm_train import DeepFMTrainer
    tr = DeepFMTrainer(c["init"], use_ab=c.get("use_ab", False), lambda_ab=c.get("lambda_ab", 0.0), loss_kind=kind, **kw)
    losses, first = [], None
    for st in range(steps):
        lo = tr.step(torch.as_tensor(x[st * n:(st + 1) * n]), torch.as_tensor(y[st * n:(st + 1) * n]), torch.as_tensor(score[st * n:(st + 1) * n]))
        losses.append(lo.cpu().numpy().copy())
        if st == 0:
            first = _np(tr.state_dict())
    return np.array(losses), first, _np(tr.state_dict()), tr


def test_debias_losses_match_reference_fit_data(golden_dir):
    for ci, c in enumerate(debiascase.load_train(golden_dir)):
        losses, first, final, _ = _run_steps(c, c["kind"], c["x"], c["y"], c["score"], c["n"], c["steps"])
        print(f"case {ci} {c['kind']}: losses {losses[:, [0, 4]].tolist()} recorded {c['losses'].tolist()}")
        np.testing.assert_allclose(losses[:, [0, 4]], c["losses"], rtol=3e-5, err_msg=f"case {ci}")
        traincase.compare_params(first, c["first"], c["init"], f"case {ci} first step")
        traincase.compare_params(final, c["final"], c["init"], f"case {ci} final")
        assert np.all(final["embedding_dict.feat.weight"][0] == 0)
        assert set(final) == set(c["final"])
        assert np.all(losses[:, 3] == 0)


def test_mirror_fit_data_with_the_debias_losses(golden_dir):
    from core.inputs import SparseFeatP
    from core.static_dataset import StaticDataset
    from core.user_model_pairwise import UserModel_Pairwise, loss_kuaishou_IPS_pairwise, loss_kuaishou_PD_pairwise
    from deepctr_torch.inputs import DenseFeat
    loss_of = {"ips": loss_kuaishou_IPS_pairwise, "pd": loss_kuaishou_PD_pairwise}
    for ci, c in enumerate(debiascase.load_train(golden_dir)):
        U, I, F, E = c["U"], c["I"], c["F"], c["E"]
        x_columns = [SparseFeatP("user_id", U, embedding_dim=E), SparseFeatP("photo_id", I, embedding_dim=E)] + \
                    [SparseFeatP(f"feat{i}", F, embedding_dim=E, embedding_name="feat", padding_idx=0) for i in range(4)] + [DenseFeat("photo_duration", 1)]
        model = UserModel_Pairwise(x_columns, [DenseFeat("y", 1)], "regression", 1, dnn_hidden_units=(64, 64), seed=2021, l2_reg_dnn=0.1, device="cpu")
        model.load_state_dict({k: torch.as_tensor(v) for k, v in c["init"].items()})
        model.compile(optimizer="adam", loss_func=loss_of[c["kind"]], metric_fun={}, metrics=None)
        ds = StaticDataset(x_columns, [DenseFeat("y", 1)], num_workers=0)
        ds.compile_dataset(c["x"], c["y"], c["score"])
        hist = model.fit_data(ds, dataset_val=None, batch_size=c["n"], epochs=1, shuffle=False, callbacks=[])
        np.testing.assert_allclose(hist[0]["loss"], c["losses"].sum() / c["N"], rtol=3e-5)
        got = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        traincase.compare_params({k: got[k] for k in c["final"]}, c["final"], c["init"], f"mirror case {ci}")


def _extended_case0(golden_dir):
    """usertrain.npz case 0 (alpha/beta on) extended to N = 100 rows by repeating rows with other labels."""
    c = traincase.load(golden_dir)[0]
    rng = np.random.RandomState(5)
    N = 100
    pick = np.r_[np.arange(len(c["x"])), rng.randint(0, len(c["x"]), N - len(c["x"]))]
    x = c["x"][pick].copy()
    x[len(c["x"]):, 6] = rng.uniform(2, 60, N - len(c["x"]))
    return c, x, rng.uniform(0, 5, (N, 1)), rng.gamma(1.0, 0.5, (N, 1)) + 0.05


# a fixed non-identity order over the 100 rows: 87 entries, rows 0 and 41 three times, thirteen-odd rows left out
def _order():
    rng = np.random.RandomState(9)
    order = rng.permutation(100)[:81]
    return np.r_[order[:40], [0, 41, 0], order[40:], [41, 0, 41]].astype(np.int64)


@pytest.mark.parametrize("kind", ["pairwise", "ips", "pd"])
def test_epoch_call_equals_step_calls_bit_for_bit(golden_dir, kind):
    from cirs_hip.deepfm_train import DeepFMTrainer
    c, x, y, score = _extended_case0(golden_dir)
    order, batch = _order(), 37
    assert len(order) != len(x) and len(np.unique(order)) < len(order) and len(order) % batch
    use_ab = kind == "pairwise"
    init = c["init"] if use_ab else {k: v for k, v in c["init"].items() if not k.startswith("ab_")}
    kw = dict(use_ab=use_ab, lambda_ab=c["lambda_ab"], loss_kind=kind)

    def by_epoch():
        tr = DeepFMTrainer(init, **kw)
        assert tr.load(x, y, score) == len(x)
        lo = tr.epoch(order, batch)
        assert tr.step_count == 3
        return lo.cpu().numpy(), _np(tr.state_dict())

    def by_batches():
        tr = DeepFMTrainer(init, **kw)
        out = []
        for s0 in range(0, len(order), batch):
            idx = order[s0:s0 + batch]
            if kind == "pairwise":         # the step entry on the gathered rows
                out.append(tr.step(x[idx], y[idx], score[idx]).cpu().numpy().copy())
            else:                          # kinds 1 and 2 have no step entry of their own: one epoch call per batch
                tr.load(x, y, score)
                out.append(tr.epoch(idx, batch).cpu().numpy()[0])
        return np.array(out), _np(tr.state_dict())

    l_e, p_e = by_epoch()
    l_b, p_b = by_batches()
    assert l_e.shape == (3, 5) and np.isfinite(l_e).all()
    assert np.array_equal(l_e, l_b)
    for k in p_b:
        assert np.array_equal(p_e[k], p_b[k]), k
    l_2, p_2 = by_epoch()
    assert np.array_equal(l_e, l_2) and all(np.array_equal(p_e[k], p_2[k]) for k in p_e)
    # order=None is the identity
    tr_a, tr_b = DeepFMTrainer(init, **kw), DeepFMTrainer(init, **kw)
    tr_a.load(x, y, score); tr_b.load(x, y, score)
    assert np.array_equal(tr_a.epoch(None, batch).cpu().numpy(), tr_b.epoch(np.arange(len(x)), batch).cpu().numpy())
    assert all(torch.equal(a, b) for a, b in zip(tr_a.state_dict().values(), tr_b.state_dict().values()))


@pytest.mark.parametrize("kind", ["ips", "pd"])
@pytest.mark.parametrize("E,batch", [(8, 1), (8, 5), (16, 5)])
def test_small_shapes_against_the_host_restatement(golden_dir, kind, E, batch):
    from cirs_hip import deepfm_host
    c = next(c for c in debiascase.load_train(golden_dir) if c["kind"] == kind and c["E"] == E)
    N = 3 * batch - (1 if batch > 1 else 0)          # the last batch short where there is room
    x, y, score = c["x"][:N], c["y"][:N], c["score"][:N]
    want_l, kept, want_final = deepfm_host.torch_train(c["init"], x, y, score, batch, kind=kind, keep=(0,))
    losses, first, final, _ = _run_steps(c, kind, x, y, score, batch, 3)
    np.testing.assert_allclose(losses[:, [0, 4]], want_l[:, [0, 4]], rtol=3e-5)      # {loss, reg}: the columns the recordings hold
    traincase.compare_params(first, kept[0], c["init"], f"{kind} E={E} batch={batch} first step")
    traincase.compare_params(final, want_final, c["init"], f"{kind} E={E} batch={batch} final")


def test_refusals(golden_dir):
    from cirs_hip import abi
    from cirs_hip.deepfm_train import DeepFMTrainer
    c = debiascase.load_train(golden_dir)[0]
    for kind in ("ips", "pd"):
        with pytest.raises(ValueError):
            DeepFMTrainer(c["init"], use_ab=True, loss_kind=kind)
    with pytest.raises(ValueError):
        DeepFMTrainer(c["init"], use_ab=False, loss_kind="dice")
    tr = DeepFMTrainer(c["init"], use_ab=False, loss_kind="ips")
    tr.load(c["x"], c["y"], c["score"])
    before = tr.flat.clone()
    with pytest.raises(ValueError):
        tr.epoch(None, 0)
    with pytest.raises(IndexError):
        tr.epoch(np.array([0, c["N"]]), 2)
    # the entry point itself: refused on the host, nothing launched
    lib = abi.lib()
    ws = tr._workspace(8)
    losses = torch.zeros(4, 5, device="cuda")

    def call(loss_kind, use_ab, batch_size):
        return lib.cirs_deepfm_train_epoch(C.byref(tr.cfg), tr.flat.data_ptr(), tr.grads.data_ptr(), tr.adam_m.data_ptr(), tr.adam_v.data_ptr(), 0,
                                           *[t.data_ptr() for t in tr._data], c["N"], None, 8, batch_size, loss_kind, use_ab, 0.0, 1e-5, 1e-5, 0.1,
                                           1e-3, 0.9, 0.999, 1e-8, losses.data_ptr(), ws.data_ptr(), ws.numel(), None)
    for args, word in [((1, 1, 8), b"alpha/beta"), ((2, 1, 8), b"alpha/beta"), ((3, 0, 8), b"unknown loss kind"), ((-1, 0, 8), b"unknown loss kind"),
                       ((1, 0, 0), b"batch"), ((0, 0, -2), b"batch")]:
        assert call(*args) == -1 and word in lib.cirs_last_error(), args
    torch.cuda.synchronize()
    assert torch.equal(tr.flat, before) and tr.step_count == 0 and float(losses.abs().max()) == 0.0


def test_score_kernels_match_the_recorded_columns(golden_dir):
    from cirs_hip.dataprep import ips_scores, item_bin_counts, popularity_scores, time_bin_bounds
    cases = debiascase.load_scores(golden_dir)
    assert [len(s["photo"]) for s in cases][:2] == [300, 257]
    for si, s in enumerate(cases):
        photo, ts = s["photo"], s["timestamp"]
        n_items = int(photo.max()) + 1
        bounds = time_bin_bounds(ts.min(), ts.max(), s["num_bin"])
        _, bins, counts = item_bin_counts(photo, ts, bounds)
        want_bins = debiascase.host_bins(ts, bounds)
        assert np.array_equal(bins.cpu().numpy(), want_bins), f"score case {si}: bins"
        assert np.array_equal(counts.cpu().numpy(), debiascase.host_counts(photo, want_bins, s["num_bin"], n_items)), f"score case {si}: counts"
        _, bins1, counts1 = item_bin_counts(photo)
        assert np.all(bins1.cpu().numpy() == 0) and np.array_equal(counts1.cpu().numpy()[0], np.bincount(photo, minlength=n_items))
        assert np.array_equal(ips_scores(photo), s["ips"]), f"score case {si}: ips"
        for gamma, want in s["pd"].items():
            assert np.array_equal(popularity_scores(photo, ts, gamma, num_bin=s["num_bin"]), want), f"score case {si}: pd gamma {gamma}"
    assert cases[1]["photo"].max() + 1 == 45 and len(np.unique(cases[2]["timestamp"])) == 1
    # rows exactly on the interior bounds belong to the bin that starts there
    ts = cases[0]["timestamp"]
    bounds = time_bin_bounds(ts.min(), ts.max(), 5)
    on = np.isin(ts, bounds[1:-1])
    assert on.sum() >= 8
    _, bins, _ = item_bin_counts(cases[0]["photo"], ts, bounds)
    assert np.array_equal(bins.cpu().numpy()[on], np.searchsorted(bounds, ts[on]))
    assert bins.cpu().numpy()[ts == ts.max()].tolist() == [4]
    # a row no bin takes keeps 0; an item id outside the table is not counted
    _, bins, counts = item_bin_counts(np.array([1, 2, 7, 1]), np.array([0.0, 5.0, 1.0, 2.5]), np.array([0.0, 1.0, 2.0]), n_items=4)
    assert bins.cpu().numpy().tolist() == [0, -1, -1, -1] and counts.cpu().numpy().tolist() == [[0, 1, 0, 0], [0, 0, 0, 0]]


@pytest.mark.parametrize("method", ["ips", "pd"])
def test_debias_training_run(tmp_path, method):
    from cirs_hip.synthetic import write_kuairec_workspace
    from core.user_model_pairwise import UserModel_Pairwise
    from core.user_model_train import train_debias_kuaishou
    from environments.KuaishouRec.env.kuaishouEnv import KuaishouEnv
    root = str(tmp_path / "data")
    write_kuairec_workspace(root, n_users=30, n_items=1400, n_env_users=16, n_env_items=60, log_len=(20, 40), seed=3)
    calls = []
    run = train_debias_kuaishou(root, method=method, save_root=str(tmp_path), feature_dim=8, batch_size=64, epoch=3, lr=5e-3,
                                rl_test=lambda model, epoch: calls.append(epoch) or float(epoch))
    losses = [h["loss"] for h in run.history]
    print(method, "loss per epoch", losses)
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert calls == [0, 1, 2] and run.history[-1]["RL_val"] == 2.0
    assert run.model.ab_columns is None
    model_dir = os.path.join(str(tmp_path), "saved_models", "KuaishouEnv-v0", {"ips": "DeepFM-IPS-pairwise", "pd": "PD-pairwise"}[method])
    if method == "pd":               # PD-pairwise.py saves nothing
        assert run.paths is None and os.listdir(model_dir) == ["logs"]
        return
    with open(run.paths.params, "rb") as fh:
        params = pickle.load(fh)
    clone = UserModel_Pairwise(**params)
    clone.load_state_dict(torch.load(run.paths.state_dict))
    again = KuaishouEnv.compute_normed_reward(clone, run.lbe_user, run.lbe_photo, run.val_set.df_photo_env)
    with open(run.paths.normed_mat, "rb") as fh:
        saved = pickle.load(fh)
    assert saved.shape == (len(run.lbe_user.classes_), len(run.lbe_photo.classes_))
    np.testing.assert_allclose(again, saved, rtol=1e-6, atol=1e-9)
    assert saved.min() == 0.0 and saved.max() == 1.0
