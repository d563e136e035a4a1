"""GPU: the validation pass (csrc/userval.hip: cirs_deepfm_validate / cirs_dice_validate; core.user_model predict_data, evaluate_data,
fit_data with a validation set) against the reference's recordings (tests/golden/userval_metrics.npz), float64 numpy, the per-row
forward kernels, itself (bit stability), and the reference's recorded fit_data logs."""
import ctypes as C

import numpy as np
import pytest
import torch

import valcase

pytestmark = pytest.mark.gpu

GROUP_ROWS = 128          # one workgroup's share: 4 wavefronts x one tile of 32 rows
MAX_GROUPS = 1536         # past this many workgroups the wavefronts walk several tiles
FINAL_LANES = 256         # validate_final_kernel: one lane per partial pair up to here


@pytest.fixture(scope="module")
def cases(golden_dir):
    return valcase.load(golden_dir)


def _device_model(kind, sd):
    from cirs_hip.deepfm import DeviceDeepFM
    from cirs_hip.dice_train import DeviceDice
    return DeviceDeepFM(sd) if kind == "pairwise" else DeviceDice(sd)


def _valset(dm, x, y):
    from cirs_hip.userval import ValSet
    return ValSet(x, y, dm.cfg, dm.device)


def _np_sums(pred, y):
    e = pred.astype(np.float64) - np.asarray(y, np.float64).reshape(-1)
    return np.array([np.abs(e).sum(), (e * e).sum()])


def _metrics():
    from core.user_model import metric_mae, metric_mse
    return {"mae": metric_mae, "mse": metric_mse}


# 1. predictions against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(4))
def test_predict_data_matches_the_reference(cases, ci):
    c = cases[ci]
    model, xc, yc = valcase.build_model(c)
    val = valcase.dataset(xc[:7] if c["kind"] == "pairwise" else xc[:9], yc, c["x"], c["y"])
    got = model.predict_data(val, batch_size=32)
    assert got.shape == (77, 1) and got.dtype == np.float64
    print(f"case {ci}: max |diff| {np.abs(got - c['pred']).max():.3e}")
    np.testing.assert_allclose(got, c["pred"], rtol=1e-5, atol=3e-6)
    assert np.array_equal(got, model.predict_data(val))          # batch_size has no effect


# 2. the reduction against float64 numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(4))
def test_device_sums_match_float64_numpy_over_the_device_predictions(cases, ci):
    c = cases[ci]
    dm = _device_model(c["kind"], c["sd"])
    pred, sums = dm.validate(_valset(dm, c["x"], c["y"]), want_pred=True)
    assert sums.dtype == torch.float64 and sums.is_cuda and pred.dtype == torch.float32
    np.testing.assert_allclose(sums.cpu().numpy(), _np_sums(pred.cpu().numpy(), c["y"]), rtol=1e-11)


# 3. metrics against the recorded values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(4))
def test_evaluate_data_matches_the_recorded_metrics(cases, ci):
    c = cases[ci]
    model, xc, yc = valcase.build_model(c, metric_fun=_metrics())
    val = valcase.dataset(xc[:7] if c["kind"] == "pairwise" else xc[:9], yc, c["x"], c["y"])
    got = model.evaluate_data(val)
    assert list(got) == ["mae", "mse"] and all(type(v) is float for v in got.values())
    delta = 3e-6 + 1e-5 * np.abs(c["pred"]).max()
    emax = np.abs(c["pred"] - c["y"]).max()
    print(f"case {ci}: mae diff {abs(got['mae'] - c['eval']['mae']):.3e} (bound {delta:.3e}), mse diff {abs(got['mse'] - c['eval']['mse']):.3e}")
    assert abs(got["mae"] - c["eval"]["mae"]) <= delta
    assert abs(got["mse"] - c["eval"]["mse"]) <= 2 * emax * delta + delta * delta
    # an untagged callable takes the reference's route: (y, float64 predictions)
    seen = {}

    def plain(y, y_predict):
        seen["shapes"] = (y.shape, y_predict.shape, y_predict.dtype)
        return np.abs(y - y_predict).mean()
    model.metric_fun = {"mae": _metrics()["mae"], "plain": plain}
    mixed = model.evaluate_data(val)
    assert seen["shapes"] == ((77, 1), (77, 1), np.float64) and mixed["mae"] == got["mae"]
    np.testing.assert_allclose(mixed["plain"], got["mae"], rtol=1e-12)


# 4. the tile kernel against the per-row kernels ------------------------------------------------------------------------------------
SHAPES = [("pairwise", 8), ("pairwise", 16), ("pairwise", 32), ("pairwise", 64), ("dice", 8), ("dice", 16), ("dice", 32)]
ONE_MORE = GROUP_ROWS * (FINAL_LANES // 4 + 1) + 1        # 65 full workgroups and one row: 264 partial pairs for 256 lanes


def _against_per_row(dm, x, y):
    pred, sums = dm.validate(_valset(dm, x, y), want_pred=True)
    want = dm.forward(x[:, 0], x[:, 1], x[:, 2:6], x[:, 6])
    pred, want = pred.cpu().numpy(), want.cpu().numpy()
    assert pred.shape == (len(x),)
    np.testing.assert_allclose(pred, want, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(sums.cpu().numpy(), _np_sums(pred, y), rtol=1e-11)
    return pred


@pytest.mark.parametrize("kind,E", SHAPES)
def test_tile_kernel_matches_the_per_row_kernel(kind, E):
    U, I = 37, 53
    dm = _device_model(kind, valcase.random_state_dict(kind, U, I, E, seed=E + len(kind)))
    assert ONE_MORE == 8321
    for n in (1, 31, 32, 33, GROUP_ROWS + 1, ONE_MORE):
        x, y = valcase.random_rows(U, I, n, seed=n)
        pred = _against_per_row(dm, x, y)
        assert np.unique(pred).size > min(n, 8) // 2 and np.abs(pred).max() > 0.1
    for n in (33, ONE_MORE):                                   # every row the same
        x, y = valcase.random_rows(U, I, n, seed=3, same=True)
        pred = _against_per_row(dm, x, y)
        assert np.all(pred == pred[0])


@pytest.mark.parametrize("kind,E", [("pairwise", 8), ("dice", 16)])
def test_more_rows_than_one_tile_per_wavefront(kind, E):
    U, I = 37, 53
    dm = _device_model(kind, valcase.random_state_dict(kind, U, I, E, seed=1))
    x, y = valcase.random_rows(U, I, MAX_GROUPS * GROUP_ROWS + 33, seed=2)
    _against_per_row(dm, x, y)


# 5. bit stability ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,E", [("pairwise", 16), ("dice", 8)])
def test_two_runs_and_the_optional_outputs_give_the_same_bits(kind, E):
    U, I = 37, 53
    dm = _device_model(kind, valcase.random_state_dict(kind, U, I, E, seed=5))
    x, y = valcase.random_rows(U, I, ONE_MORE, seed=6)
    vs = _valset(dm, x, y)
    p1, s1 = dm.validate(vs, want_pred=True)
    p2, s2 = dm.validate(vs, want_pred=True)
    assert torch.equal(p1, p2) and torch.equal(s1, s2)
    none, s3 = dm.validate(vs, want_pred=False)
    p4, none4 = dm.validate(vs, want_pred=True, want_sums=False)
    assert none is None and none4 is None and torch.equal(s3, s1) and torch.equal(p4, p1)
    # without y only the predictions can be asked for
    nolabel = _valset(dm, x, None)
    assert torch.equal(dm.validate(nolabel, want_pred=True, want_sums=False)[0], p1)
    with pytest.raises(ValueError):
        dm.validate(nolabel)


def test_entry_refusals(cases):
    from cirs_hip import abi
    c = cases[0]
    dm = _device_model("pairwise", c["sd"])
    vs = _valset(dm, c["x"], c["y"])
    lib = abi.lib()
    sums = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.cirs_deepfm_validate_workspace_bytes(C.byref(dm.cfg), vs.n), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 16 * 4 and lib.cirs_deepfm_validate_workspace_bytes(C.byref(dm.cfg), 0) == 0

    def call(n, y, pred, s, ws_bytes):
        return lib.cirs_deepfm_validate(C.byref(dm.cfg), C.byref(dm.w), vs.uid.data_ptr(), vs.pid.data_ptr(), vs.feats.data_ptr(), vs.dur.data_ptr(), y,
                                        n, pred, s, ws.data_ptr(), ws_bytes, None)
    for args, word in [((0, vs.y.data_ptr(), None, sums.data_ptr(), ws.numel()), b"empty"), ((-3, vs.y.data_ptr(), None, sums.data_ptr(), ws.numel()), b"empty"),
                       ((77, None, None, sums.data_ptr(), ws.numel()), b"need y"), ((77, vs.y.data_ptr(), None, None, ws.numel()), b"neither"),
                       ((77, vs.y.data_ptr(), None, sums.data_ptr(), 8), b"workspace")]:
        assert call(*args) == -1 and word in lib.cirs_last_error(), args
    torch.cuda.synchronize()
    assert sums.tolist() == [-1.0, -1.0]
    other = valcase.random_state_dict("pairwise", c["U"] + 1, c["I"], c["E"], seed=0)
    with pytest.raises(ValueError):
        _device_model("pairwise", other).validate(vs)


# 6. trainer against model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 2])
def test_trainer_validate_equals_the_model_loaded_from_its_state_dict(cases, ci):
    c = cases[ci]
    f = c["fit"]
    model, xc, yc = valcase.build_model(c, metric_fun=_metrics(), lr=f["lr"])
    tr = model._new_trainer()
    tr.load(f["x"], f["y"], f["score"])
    tr.epoch(None, f["batch"])
    dm0 = model.device_model()
    vs = _valset(dm0, c["x"], c["y"])
    _, live = tr.validate(vs)
    clone, xc, yc = valcase.build_model(c, sd=tr.state_dict(), metric_fun=_metrics())
    val = valcase.dataset(xc[:7] if c["kind"] == "pairwise" else xc[:9], yc, c["x"], c["y"])
    got = clone.evaluate_data(val)
    live = live.cpu().numpy()
    assert got == {"mae": float(live[0] / 77), "mse": float(live[1] / 77)}
    assert got != model.evaluate_data(val)                      # the step moved the numbers


# 7. fit_data against the reference's recorded run -----------------------------------------------------------------------------------
class _Record:
    def __init__(self, model, val):
        self.model, self.val, self.seen = model, val, []

    def on_train_begin(self): pass
    def on_train_end(self): pass
    def on_epoch_begin(self, epoch): pass

    def on_epoch_end(self, epoch, logs):
        self.seen.append((epoch, dict(logs), self.model.evaluate_data(self.val)))


# Largest relative deviation of mae / mse from the reference's recorded logs, measured on an MI355X against this fixture:
#   pairwise E = 8 (IPS loss): 2.4e-7 (mse, epoch 1);  DICE E = 8: 9.1e-8 (mse, epoch 1)
# asserted at 4 x that, rounded up to one digit, and never looser than 1e-3 (the fixture's records differ by >= 1 % per epoch, so
# metrics of stale weights cannot pass).
FIT_RTOL = {0: 1e-6, 2: 4e-7}


@pytest.mark.parametrize("ci", [0, 2])
def test_fit_data_reports_validation_metrics_like_the_reference(cases, ci):
    c = cases[ci]
    f = c["fit"]
    model, xc, yc = valcase.build_model(c, metric_fun=_metrics(), lr=f["lr"])
    val = valcase.dataset(xc[:7] if c["kind"] == "pairwise" else xc[:9], yc, c["x"], c["y"])
    train = valcase.dataset(xc, yc, f["x"], f["y"], f["score"])
    hook_saw = []

    def hook(m):
        hook_saw.append(m.evaluate_data(val))
        return {"RL_a": float(len(hook_saw)), "RL_b": 0.5}
    model.compile_RL_test(hook)
    rec = _Record(model, val)
    history = model.fit_data(train, val, batch_size=f["batch"], epochs=f["epochs"], shuffle=False, callbacks=[rec])
    assert [e for e, _, _ in rec.seen] == [-1, 0, 1]
    assert list(rec.seen[0][1]) == ["mae", "mse", "RL_a", "RL_b"]
    assert all(list(lg) == ["loss", "mae", "mse", "RL_a", "RL_b"] for _, lg, _ in rec.seen[1:])
    assert history == [lg for _, lg, _ in rec.seen[1:]]
    for k, (epoch, logs, at_callback) in enumerate(rec.seen):
        # the hook and the callback score the weights of their epoch: the published module equals the trainer's live parameters
        assert hook_saw[k] == {"mae": logs["mae"], "mse": logs["mse"]} == at_callback, epoch
        assert logs["RL_a"] == float(k + 1)
    got = np.array([[lg["mae"], lg["mse"]] for _, lg, _ in rec.seen])
    dev = np.abs(got - f["logs"][:, 1:]) / f["logs"][:, 1:]
    print(f"case {ci}: relative deviation of mae / mse from the recorded logs per record {dev.tolist()}; loss {[h['loss'] for h in history]} "
          f"recorded {f['logs'][1:, 0].tolist()}")
    assert FIT_RTOL[ci] is not None and FIT_RTOL[ci] <= 1e-3
    assert dev.max() <= FIT_RTOL[ci]
    np.testing.assert_allclose([h["loss"] for h in history], f["logs"][1:, 0], rtol=1e-3)
    assert model.evaluate_data(val) == rec.seen[-1][2]          # the state after fit_data: the last epoch's weights


# 8. no behaviour change without metrics ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 2])
def test_fit_data_without_metrics_is_as_before(cases, ci):
    c = cases[ci]
    f = c["fit"]
    runs = []
    for with_val in (False, True):
        model, xc, yc = valcase.build_model(c, metric_fun=None, lr=f["lr"])
        val = valcase.dataset(xc[:7] if c["kind"] == "pairwise" else xc[:9], yc, c["x"], c["y"])
        train = valcase.dataset(xc, yc, f["x"], f["y"], f["score"])
        rec = _Record(model, val)
        rec.on_epoch_end = lambda epoch, logs, rec=rec: rec.seen.append((epoch, dict(logs)))
        history = model.fit_data(train, val if with_val else None, batch_size=f["batch"], epochs=f["epochs"], shuffle=False, callbacks=[rec])
        assert [e for e, _ in rec.seen] == [0, 1] and all(list(h) == ["loss"] for h in history)
        runs.append((history, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
