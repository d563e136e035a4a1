"""GPU: the DICE debiasing baseline on the device -- cirs_dice_train_epoch against the recording of the reference's fit_data
(tests/golden/usertrain_dice.npz) and the host restatement, cirs_dice_forward / DeviceDice against the recorded forward values,
UserModel_DICE.fit_data, the refusals and the training run."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import dicecase
import traincase

pytestmark = pytest.mark.gpu

REC = dicecase.load()


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    """Module constructors draw initial weights from torch's global CPU generator and fit_data its permutations from the CUDA one: put both
    back, so the tests that run after this file see the streams they saw before it existed."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu)


def _np(sd):
    return {k: v.cpu().numpy() for k, v in sd.items()}


def _run_steps(init, x, y, score, n, steps):
    """`steps` step() calls on consecutive batches of n rows -> ([steps, 6] losses, parameters after the first step, final)."""
    from cirs_hip.dice_train import DiceTrainer
    tr = DiceTrainer(init, **dicecase.L2)
    losses, first = [], None
    for st in range(steps):
        lo = tr.step(x[st * n:(st + 1) * n], y[st * n:(st + 1) * n], score[st * n:(st + 1) * n])
        losses.append(lo.cpu().numpy().copy())
        if st == 0:
            first = _np(tr.state_dict())
    assert tr.step_count == steps
    return np.array(losses), first, _np(tr.state_dict())


@pytest.mark.parametrize("ci", range(len(REC["cases"])))
def test_recorded_cases(ci):
    c = REC["cases"][ci]
    losses, first, final = _run_steps(c["init"], c["x"], c["y"], c["score"], c["n"], c["steps"])
    print(f"case {ci}: {{loss, reg}} {losses[:, [0, 5]].tolist()} recorded {c['losses'].tolist()}")
    np.testing.assert_allclose(losses[:, [0, 5]], c["losses"], rtol=dicecase.LOSS_RTOL, err_msg=f"case {ci}")
    np.testing.assert_allclose(losses[:, 1:5].sum(1), losses[:, 0], rtol=1e-6)
    traincase.compare_params(first, c["first"], c["init"], f"case {ci} first step")
    traincase.compare_params(final, c["final"], c["init"], f"case {ci} final")
    assert np.all(final["embedding_dict.feat.weight"][0] == 0)
    assert set(final) == set(c["final"])
    # linear_model.*: no data gradient, moved by the regulariser alone
    names = dicecase.unused_names(c["final"])
    assert len(names) == 6
    traincase.compare_params({k: final[k] for k in names}, {k: c["final"][k] for k in names}, c["init"], f"case {ci} linear_model")
    if ci == 0:          # the second batch is all +1
        assert losses[1, 4] == 0.0 and losses[0, 4] > 0.0 and losses[1, 3] != 0.0


@pytest.mark.parametrize("E,batch", [(8, 1), (8, 5), (16, 5)])
def test_small_shapes_against_the_host_restatement(E, batch):
    from cirs_hip import dice_host
    c = next(c for c in REC["cases"] if c["E"] == E)
    N = 3 * batch - (1 if batch > 1 else 0)          # the last batch short where there is room
    x, y, score = c["x"][:N], c["y"][:N], c["score"][:N]
    want_l, kept, want_final = dice_host.torch_train(c["init"], x, y, score, batch, keep=(0,), **dicecase.L2)
    losses, first, final = _run_steps(c["init"], x, y, score, batch, 3)
    print(f"E={E} batch={batch}: device {losses.tolist()} host {want_l.tolist()}")
    np.testing.assert_allclose(losses[:, [0, 5]], want_l[:, [0, 5]], rtol=dicecase.LOSS_RTOL)
    traincase.compare_params(first, kept[0], c["init"], f"E={E} batch={batch} first step")
    traincase.compare_params(final, want_final, c["init"], f"E={E} batch={batch} final")


def test_emb_dim_32_against_the_host_restatement():
    """The widest embedding the entry accepts: a model built here (embedding tables scaled up like the recorded cases), batch 5, three steps,
    the last batch short; same bars as the recorded shapes."""
    from cirs_hip import dice_host
    from core.user_model_DICE import UserModel_DICE
    from deepctr_torch.inputs import DenseFeat
    c = REC["cases"][0]
    U, I, F, E, batch = 20, 30, c["F"], 32, 5
    model = UserModel_DICE(dicecase.feature_columns(U, I, F, E), [DenseFeat("y", 1)], "regression", 1, dnn_hidden_units=(64, 64), seed=7)
    rng = np.random.RandomState(32)
    init = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    for k in init:
        if "embedding_dict" in k:
            init[k] = rng.normal(0, 0.3, init[k].shape).astype(np.float32)
    init["embedding_dict.feat.weight"][0] = 0
    N = 3 * batch - 1
    x = c["x"][:N].copy()
    x[:, [0, 1]] %= U; x[:, [2, 3, 9, 10]] %= I
    y, score = c["y"][:N], c["score"][:N]
    assert (score > 0).any() and (score < 0).any()
    want_l, kept, want_final = dice_host.torch_train(init, x, y, score, batch, keep=(0,), **dicecase.L2)
    losses, first, final = _run_steps(init, x, y, score, batch, 3)
    print(f"E=32: device {losses[:, [0, 5]].tolist()} host {want_l[:, [0, 5]].tolist()}")
    np.testing.assert_allclose(losses[:, [0, 5]], want_l[:, [0, 5]], rtol=dicecase.LOSS_RTOL)
    traincase.compare_params(first, kept[0], init, "E=32 first step")
    traincase.compare_params(final, want_final, init, "E=32 final")
    from cirs_hip.dice_train import DeviceDice
    x7 = np.concatenate([x[:, [0, 2]], x[:, 4:9]], axis=1)
    got = DeviceDice(init).forward(x7[:, 0], x7[:, 1], x7[:, 2:6], x7[:, 6]).cpu().numpy()
    host = dice_host.forward({k: torch.as_tensor(v) for k, v in init.items()}, torch.as_tensor(x7, dtype=torch.float32)).numpy()
    np.testing.assert_allclose(got, host, rtol=1e-5, atol=2e-6)


# a fixed non-identity order over the 100 rows: 87 entries, rows 0 and 41 three times, thirteen-odd rows left out
def _order():
    rng = np.random.RandomState(9)
    order = rng.permutation(100)[:81]
    return np.r_[order[:40], [0, 41, 0], order[40:], [41, 0, 41]].astype(np.int64)


def test_epoch_call_equals_step_calls_bit_for_bit():
    from cirs_hip.dice_train import DiceTrainer
    c = REC["cases"][0]
    x, y, score = c["x"], c["y"], c["score"]
    order, batch = _order(), 37
    assert len(order) != len(x) and len(np.unique(order)) < len(order) and len(order) % batch

    def by_epoch():
        tr = DiceTrainer(c["init"], **dicecase.L2)
        assert tr.load(x, y, score) == len(x)
        lo = tr.epoch(order, batch)
        assert tr.step_count == 3
        return lo.cpu().numpy(), _np(tr.state_dict())

    def by_batches():
        tr = DiceTrainer(c["init"], **dicecase.L2)
        out = []
        for s0 in range(0, len(order), batch):
            idx = order[s0:s0 + batch]
            out.append(tr.step(x[idx], y[idx], score[idx]).cpu().numpy().copy())
        return np.array(out), _np(tr.state_dict())

    l_e, p_e = by_epoch()
    l_b, p_b = by_batches()
    assert l_e.shape == (3, 6) and np.isfinite(l_e).all()
    assert np.array_equal(l_e, l_b)
    for k in p_b:
        assert np.array_equal(p_e[k], p_b[k]), k
    l_2, p_2 = by_epoch()
    assert np.array_equal(l_e, l_2) and all(np.array_equal(p_e[k], p_2[k]) for k in p_e)
    # order=None is the identity
    tr_a, tr_b = DiceTrainer(c["init"], **dicecase.L2), DiceTrainer(c["init"], **dicecase.L2)
    tr_a.load(x, y, score); tr_b.load(x, y, score)
    assert np.array_equal(tr_a.epoch(None, batch).cpu().numpy(), tr_b.epoch(np.arange(len(x)), batch).cpu().numpy())
    assert all(torch.equal(a, b) for a, b in zip(tr_a.state_dict().values(), tr_b.state_dict().values()))


def test_out_of_range_order_entry_gives_a_nan_loss():
    """The documented behaviour of the entry: the index is not read, that step's loss is NaN, the other steps are not."""
    from cirs_hip.dice_train import DiceTrainer
    c = REC["cases"][0]
    tr = DiceTrainer(c["init"], **dicecase.L2)
    tr.load(c["x"], c["y"], c["score"])
    order = np.arange(20, dtype=np.int64)
    order[13] = c["N"] + 5
    with pytest.raises(IndexError):
        tr.epoch(order, 10)
    lo = tr.epoch(order, 10, check=False).cpu().numpy()
    assert np.isfinite(lo[0]).all() and np.isnan(lo[1, 0]) and np.isnan(lo[1, 1]) and np.isfinite(lo[1, 2:5]).all()


def test_forward_and_sweep_match_the_recording():
    from cirs_hip.dice_train import DeviceDice
    f = REC["forward"]
    dm = DeviceDice(REC["cases"][0]["init"])
    x = f["x"]
    y = dm.forward(x[:, 0], x[:, 1], x[:, 2:6], x[:, 6]).cpu().numpy()
    print("forward max |diff|", np.abs(y - f["y"][:, 0]).max(), "max |y|", np.abs(f["y"]).max())
    np.testing.assert_allclose(y, f["y"][:, 0], rtol=1e-5, atol=2e-6)          # the bar of tests/test_gpu_deepfm.py's forward checks
    # the rows as a sweep: user r against the item of row r sits on the diagonal
    pred, mm = dm.sweep(x[:, 0], x[:, 1], x[:, 2:6], x[:, 6])
    assert pred.shape == (50, 50)
    np.testing.assert_allclose(pred.diagonal().cpu().numpy(), f["y"][:, 0], rtol=1e-5, atol=2e-6)
    assert float(mm[0]) == float(pred.min()) and float(mm[1]) == float(pred.max())


def test_sweep_equals_forward_on_the_pairs_bit_for_bit():
    from cirs_hip.dice_train import DeviceDice
    c = REC["cases"][0]
    dm = DeviceDice(c["init"])
    rng = np.random.RandomState(3)
    users, items = np.array([7, 31]), rng.permutation(c["I"])[:33]
    feats = np.where(np.arange(4)[None, :] < rng.randint(1, 5, 33)[:, None], rng.randint(1, c["F"], (33, 4)), 0)
    dur = rng.uniform(2, 60, 33)
    pred, mm = dm.sweep(users, items, feats, dur)
    pairs = dm.forward(np.repeat(users, 33), np.tile(items, 2), np.tile(feats, (2, 1)), np.tile(dur, 2))
    assert pred.shape == (2, 33) and torch.equal(pred.reshape(-1), pairs)
    dm.PAIRS_PER_CALL = 33                  # one user per call
    pred1, mm1 = dm.sweep(users, items, feats, dur)
    assert torch.equal(pred1, pred) and torch.equal(mm1, mm)
    # a row with an id outside its table is not read
    bad = dm.forward([0, c["U"]], [0, 0], np.zeros((2, 4)), [1.0, 1.0]).cpu().numpy()
    assert np.isfinite(bad[0]) and np.isnan(bad[1])


def test_mirror_fit_data():
    from core.static_dataset import StaticDataset
    from core.user_model_DICE import UserModel_DICE, loss_kuaishou_DICE
    from deepctr_torch.inputs import DenseFeat
    for ci, c in enumerate(REC["cases"]):
        x_columns = dicecase.feature_columns(c["U"], c["I"], c["F"], c["E"])
        model = UserModel_DICE(x_columns, [DenseFeat("y", 1)], "regression", 1, dnn_hidden_units=(64, 64), seed=2021, l2_reg_dnn=0.1, device="cpu")
        model.load_state_dict({k: torch.as_tensor(v) for k, v in c["init"].items()})
        back = model.state_dict()
        assert set(back) == set(c["init"]) and all(np.array_equal(back[k].numpy(), c["init"][k]) for k in back)
        model.compile(optimizer="adam", loss_func=loss_kuaishou_DICE, metric_fun={}, metrics=None)
        ds = StaticDataset(x_columns, [DenseFeat("y", 1)], num_workers=0)
        ds.compile_dataset(c["x"], c["y"], c["score"])
        hist = model.fit_data(ds, dataset_val=None, batch_size=c["n"], epochs=1, shuffle=False, callbacks=[])
        np.testing.assert_allclose(hist[0]["loss"], c["losses"].sum() / c["N"], rtol=dicecase.LOSS_RTOL)
        got = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        traincase.compare_params({k: got[k] for k in c["final"]}, c["final"], c["init"], f"mirror case {ci}")
        # the module's forward runs over the fitted weights
        f = REC["forward"]["x"][:5].copy()
        f[:, 0] %= c["U"]; f[:, 1] %= c["I"]
        y = model.forward(torch.as_tensor(f)).cpu().numpy()
        assert y.shape == (5, 1) and np.isfinite(y).all()


def test_refusals():
    from cirs_hip import abi
    from cirs_hip.dice_train import DeviceDice, DiceTrainer
    from core.user_model_DICE import UserModel_DICE
    from core.user_model_pairwise import loss_kuaishou_IPS_pairwise
    from deepctr_torch.inputs import DenseFeat
    c = REC["cases"][0]
    model = UserModel_DICE(dicecase.feature_columns(c["U"], c["I"], c["F"], c["E"]), [DenseFeat("y", 1)], "regression", 1, dnn_hidden_units=(64, 64))
    with pytest.raises(AssertionError):
        model.compile(optimizer="adam", loss_func=loss_kuaishou_IPS_pairwise)
    with pytest.raises(AssertionError):
        model.compile(optimizer="adam", loss_func=lambda *a: 0)
    bad = dict(c["init"])
    bad["embedding_dict.user_int.weight"] = np.zeros((c["U"], 12), np.float32)
    with pytest.raises(ValueError):
        DiceTrainer(bad)
    tr = DiceTrainer(c["init"], **dicecase.L2)
    with pytest.raises(IndexError):           # an id outside its table is refused when the data set is loaded
        x = c["x"].copy(); x[3, 10] = c["I"]
        tr.load(x, c["y"], c["score"])
    tr.load(c["x"], c["y"], c["score"])
    before = tr.flat.clone()
    with pytest.raises(ValueError):
        tr.epoch(None, 0)
    # the entry points themselves: refused on the host, nothing launched
    lib = abi.lib()
    ws = tr._workspace(8)
    losses = torch.zeros(4, 6, device="cuda")

    def call(cfg=tr.cfg, params=tr.flat.data_ptr(), ws_bytes=ws.numel(), step_before=0, col0=tr._data[0].data_ptr(), batch=8):
        cols = [col0] + [t.data_ptr() for t in tr._data[1:]]
        return lib.cirs_dice_train_epoch(C.byref(cfg), params, tr.grads.data_ptr(), tr.adam_m.data_ptr(), tr.adam_v.data_ptr(), step_before,
                                         *cols, c["N"], None, 8, batch, 1e-5, 1e-5, 0.1, 1e-3, 0.9, 0.999, 1e-8, losses.data_ptr(),
                                         ws.data_ptr(), ws_bytes, None)
    cfg12 = abi.DiceCfg(n_user_vocab=c["U"], n_item_vocab=c["I"], n_feat_vocab=c["F"], emb_dim=12, hidden=64)
    cfg_h = abi.DiceCfg(n_user_vocab=c["U"], n_item_vocab=c["I"], n_feat_vocab=c["F"], emb_dim=8, hidden=128)
    for kw, word in [(dict(cfg=cfg12), b"emb_dim"), (dict(cfg=cfg_h), b"hidden"), (dict(params=None), b"null argument"),
                     (dict(col0=None), b"null data column"), (dict(ws_bytes=1024), b"workspace too small"),
                     (dict(step_before=-1), b"negative step count"), (dict(batch=0), b"batch")]:
        assert call(**kw) != 0 and word in lib.cirs_last_error(), kw
    out = torch.zeros(2, device="cuda")
    ids = torch.zeros(2, dtype=torch.int64, device="cuda")
    f4 = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    assert lib.cirs_dice_forward(C.byref(cfg12), tr.flat.data_ptr(), ids.data_ptr(), ids.data_ptr(), f4.data_ptr(), out.data_ptr(), 2,
                                 out.data_ptr(), None) != 0 and b"emb_dim" in lib.cirs_last_error()
    assert lib.cirs_dice_forward(C.byref(tr.cfg), None, ids.data_ptr(), ids.data_ptr(), f4.data_ptr(), out.data_ptr(), 2, out.data_ptr(),
                                 None) != 0 and b"null argument" in lib.cirs_last_error()
    assert lib.cirs_dice_train_workspace_bytes(None, 8) == 0 and lib.cirs_dice_train_param_count(None) == 0
    torch.cuda.synchronize()
    assert torch.equal(tr.flat, before) and tr.step_count == 0 and float(losses.abs().max()) == 0.0
    assert DeviceDice(c["init"]).flat.numel() == tr.flat.numel()


class _Epochs:
    def __init__(self):
        self.seen = []

    def on_train_begin(self): pass
    def on_train_end(self): pass
    def on_epoch_begin(self, epoch): pass

    def on_epoch_end(self, epoch, logs):
        self.seen.append((epoch, dict(logs)))


def test_dice_training_run(tmp_path):
    from cirs_hip.synthetic import write_kuairec_workspace
    from core.user_model_DICE import UserModel_DICE
    from core.user_model_train import train_dice_kuaishou
    root = str(tmp_path / "data")
    write_kuairec_workspace(root, n_users=30, n_items=1400, n_env_users=16, n_env_items=60, log_len=(20, 40), seed=3)
    calls, cb = [], _Epochs()

    def rl_test(model):
        calls.append(len(calls))
        return {"RL_val": float(len(calls))}
    run = train_dice_kuaishou(root, save_root=str(tmp_path), feature_dim=8, batch_size=64, epoch=3, lr=5e-3, rl_test=rl_test, callbacks=[cb])
    losses = [h["loss"] for h in run.history]
    print("loss per epoch", losses)
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert len(calls) == 4 and [e for e, _ in cb.seen] == [-1, 0, 1, 2]
    assert cb.seen[0][1] == {"RL_val": 1.0} and run.history[-1]["RL_val"] == 4.0
    model_dir = os.path.join(str(tmp_path), "saved_models", "KuaishouEnv-v0", "DICE")
    assert sorted(os.listdir(model_dir)) == ["DICE_params_DICE.pickle", "logs"]        # DICE.py writes the params pickle only
    with open(run.paths.params, "rb") as fh:
        params = pickle.load(fh)
    clone = UserModel_DICE(**params)
    clone.load_state_dict(run.model.state_dict())
    # the score column is the sign rule over the log's own counts
    from core.user_data import load_dataset_kuaishou_DICE
    ds, x_columns, _ = load_dataset_kuaishou_DICE(8, 8, datapath=root)
    assert ds.x_numpy.shape[1] == 16 and len(x_columns) == 16 and set(np.unique(ds.score)) == {-1, 1}
    assert np.array_equal(ds.x_numpy[:, 0], ds.x_numpy[:, 1]) and np.array_equal(ds.x_numpy[:, 2], ds.x_numpy[:, 3])
    assert np.array_equal(ds.x_numpy[:, 9], ds.x_numpy[:, 10])
    count = np.bincount(ds.x_numpy[:, 2].astype(np.int64), minlength=int(ds.x_numpy[:, 9].max()) + 1)
    want = np.where(np.maximum(count[ds.x_numpy[:, 2].astype(np.int64)], 1) > np.maximum(count[ds.x_numpy[:, 9].astype(np.int64)], 1), 1, -1)
    assert np.array_equal(ds.score[:, 0], want)
    # the static-policy evaluation's recommendation runs over the DICE device model
    user = int(run.lbe_user.classes_[0])
    idx, raw, val = clone.recommend_k_item(user, run.val_set, k=3, is_softmax=False)
    items = run.val_set.df_photo_env.index.to_numpy()
    assert len(set(idx.tolist())) == 3 and np.array_equal(items[idx], raw) and np.isfinite(val).all()
    pred, _ = clone.device_model().sweep([user], items, run.val_set.df_photo_env[["feat0", "feat1", "feat2", "feat3"]].to_numpy(),
                                         run.val_set.df_photo_env["photo_duration"].to_numpy())
    assert idx[0] == int(pred[0].argmax())
