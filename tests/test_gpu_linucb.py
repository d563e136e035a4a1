"""GPU: the LinUCB baseline on the device (csrc/linucb.hip, cirs_hip/linucb.py, core/policy/linucb.py, evaluation.test_kuaishou)
against the recording of the reference (tests/golden/linucb.npz) and, at shapes the recording does not hold, against the host
restatement (cirs_hip/linucb_host.py).  A and b are compared in bits; everything behind the solve goes through the error protocol of
tests/linucbcase.py (E_dev <= 4 E_ref against the recorded exact values).

Measured on one MI355X when this file was written (largest E_dev / E_ref over the quantities; the device refines its solve with a
residual in twice the working precision, so theta and inv(A) equal the correctly rounded exact values in every bit and the rest is a
rounding or two away):
    case 0 epoch 2   theta 0, mean 2.4e-05, var 1.4e-04, ucb 1.4e-04, y_predict 5.8e-05
    case 1 epoch 1   theta 0, mean 1.1e-06, var 7.5e-08, ucb 1.1e-07, y_predict 4.8e-07;   epoch 5   at most 9.4e-08
    case 2 epoch 1   theta 0, mean 7.0e-04, var 2.0e-03, ucb 5.0e-03, y_predict 6.0e-04
    synthetic shapes against the restatement's extended mode: at most 0.03 (theta of the one-arm log), its own distance from exact
    linucb_trainer on case 0: val_mae / val_mse within 3.9e-13 of the recorded values (bar: rtol 1e-9)
    test_kuaishou on case 0: counts equal, click_loss / ctr / R_tra within 1.2e-14 (bar: rtol 1e-6)"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linucbcase  # noqa: E402

from cirs_hip import linucb_host  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = linucbcase.load()
METRICS = {"mae": lambda y, y_predict: torch.nn.functional.l1_loss(torch.from_numpy(y), torch.from_numpy(y_predict)).numpy(),
           "mse": lambda y, y_predict: torch.nn.functional.mse_loss(torch.from_numpy(y), torch.from_numpy(y_predict)).numpy()}


def _np(t):
    return t.cpu().numpy()


def _dataset(c):
    df = pd.DataFrame(c.photo_values, index=pd.Index(c.photo_index, name="photo_id"))
    return SimpleNamespace(df_photo_env=df, x_numpy=c.val_x, get_y=lambda: c.val_y)


def _device(c):
    from cirs_hip.linucb import DeviceLinUCB
    return DeviceLinUCB(c.K, c.d, c.alpha)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_recorded_cases(ci):
    c = CASES[ci]
    dev = _device(c)
    arm = linucb_host.arm_of_rows(c.classes, c.x[:, 1])
    val_arm = linucb_host.arm_of_rows(c.classes, c.val_x[:, 1])
    plan = dev.plan(arm)
    for e in c.epochs:
        dev.update(c.x, c.y, plan=plan)
        r = c.rec[e]
        assert np.array_equal(_np(dev.A), r.A) and np.array_equal(_np(dev.b), r.b), f"case {ci} epoch {e}: A / b differ in bits"
        if e not in c.full:
            continue
        what = f"case {ci} epoch {e} device "
        best, best_mean, ucb, mean, var = (_np(t) for t in dev.score(c.users, c.photo_values, want_full=True))
        linucbcase.check(what + "theta", _np(dev.theta), r.theta_exact, r.eref["theta"])
        linucbcase.check(what + "A_inv (bar: theta's)", _np(dev.A_inv), r.A_inv_exact, r.eref["theta"])
        linucbcase.check(what + "mean", mean, r.mean_exact, r.eref["mean"])
        linucbcase.check(what + "var", var, r.var_exact, r.eref["var"])
        linucbcase.check(what + "ucb", ucb, r.ucb_exact, r.eref["ucb"])
        linucbcase.check(what + "y_predict", _np(dev.predict(c.val_x, val_arm)).reshape(-1, 1), r.ypred_exact, r.eref["y_predict"])
        assert c.kept.sum() >= 36
        differ = int((c.classes[best][c.kept] != r.rec_item[c.kept]).sum())
        assert differ == 0, f"{what}: {differ} of {int(c.kept.sum())} arg-max arms differ from the reference's"
        assert np.array_equal(best, ucb.argmax(1)) and np.array_equal(best_mean, mean[np.arange(len(best)), best])
        linucbcase.check(what + "returned mean", best_mean[c.kept], r.mean_exact[np.arange(len(best)), best][c.kept], r.eref["mean"],
                         scale=r.mean_exact)
        best2, mean2 = dev.score(c.users, c.photo_values)          # without the full outputs: the same picks
        assert np.array_equal(_np(best2), best) and np.array_equal(_np(mean2), best_mean)


class _Logger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _env(c):
    from environments.KuaishouRec.env.kuaishouEnv import KuaishouEnv
    n_raw = int(c.classes.max()) + 1
    list_feat = [[] for _ in range(n_raw)]
    for i, rp in enumerate(c.classes):
        list_feat[int(rp)] = [int(v) for v in c.item_cats[i] if v >= 0]
    return KuaishouEnv(mat=c.mat, lbe_user=SimpleNamespace(classes_=c.raw_uid), lbe_photo=SimpleNamespace(classes_=c.classes), list_feat=list_feat,
                       df_photo_env=None, df_dist_small=c.dist, num_leave_compute=3, leave_threshold=1, max_turn=12)


def test_trainer_and_policy_on_case0():
    from core.policy.linucb import linucb_policy, linucb_trainer
    c = CASES[0]
    ds, env, logger = _dataset(c), _env(c), _Logger()
    model = linucb_policy(c.K, c.d, c.alpha)
    history = linucb_trainer(model, env, len(c.epochs), pd.DataFrame(c.x), pd.DataFrame(c.y), ds, logger, METRICS)
    assert len(history) == len(logger.lines) == len(c.epochs)
    for epo, (res, line) in enumerate(zip(history, logger.lines)):
        assert line == "Epoch: [{}], Info: [{}]".format(epo, res)
        assert list(res) == ["val_mae", "val_mse"] + ["RL_val_" + k for k in ("click_loss", "CV", "CV_turn", "ctr", "len_tra", "R_tra")]
        want = c.rec[epo + 1].metrics
        got = np.array([float(res["val_mae"]), float(res["val_mse"])])
        print(f"epoch {epo}: val_mae, val_mse relative gap to the recording {np.abs(got / want - 1).tolist()}")
        np.testing.assert_allclose(got, want, rtol=1e-9)
        assert isinstance(res["RL_val_CV"], str) and res["RL_val_len_tra"] >= 1
    r = c.rec[c.epochs[-1]]
    assert np.array_equal(_np(model.device_state.A), r.A) and np.array_equal(_np(model.device_state.b), r.b)
    bar = (1 + linucbcase.FACTOR) * r.eref["mean"] * np.abs(r.mean_exact).max()     # the reference's own error plus the device's bar
    for u in np.flatnonzero(c.kept)[:12]:
        item, reward = model.recommend_k_item(c.users[u], ds, k=1, is_softmax=False)
        assert int(item) == int(r.rec_item[u]) and isinstance(reward, float)
        assert abs(reward - r.rec_reward[u]) <= bar, (u, reward, r.rec_reward[u])
    arm = model.linucb_arms[3]
    assert (arm.arm_index, arm.alpha) == (3, c.alpha) and len(model.linucb_arms) == model.K_arms == c.K
    assert arm.A.shape == (c.d, c.d) and arm.b.shape == (c.d, 1) and arm.theta.shape == (c.d, 1) and arm.A_inv.shape == (c.d, c.d)
    x = np.r_[c.users[0], 3.0, c.photo_values[3]]
    assert arm.calc_reward(x).shape == (1, 1) and arm.calc_UCB(x).shape == (1, 1) and model.forward(3, x).shape == (1, 1)
    assert arm.calc_UCB(x)[0, 0] >= arm.calc_reward(x)[0, 0]


def test_reward_update_replays_the_batched_update_in_bits():
    from core.policy.linucb import linucb_policy
    c = CASES[0]
    arm_of_row = linucb_host.arm_of_rows(c.classes, c.x[:, 1])
    count = np.bincount(arm_of_row[arm_of_row >= 0], minlength=c.K)
    a = int(np.flatnonzero((count >= 3) & (count <= 12))[0])
    model = linucb_policy(c.K, c.d, c.alpha)
    theta0 = model.linucb_arms[a].theta
    for row in np.flatnonzero(arm_of_row == a):
        model.linucb_arms[a].reward_update(c.y[row], c.x[row])
    r = c.rec[1]
    assert np.array_equal(model.linucb_arms[a].A, r.A[a]) and np.array_equal(model.linucb_arms[a].b[:, 0], r.b[a])
    assert not theta0.any() and model.linucb_arms[a].theta.any()                # the one-row updates marked the arm dirty
    other = (a + 1) % c.K
    assert np.array_equal(model.linucb_arms[other].A, np.identity(c.d)) and not model.linucb_arms[other].theta.any()


def test_kuaishou_matches_the_reference_loop():
    import evaluation as ev
    from core.policy.linucb import linucb_policy
    c = CASES[0]
    ds, env = _dataset(c), _env(c)
    model = linucb_policy(c.K, c.d, c.alpha)
    arm = linucb_host.arm_of_rows(c.classes, c.x[:, 1])
    for e in c.epochs:
        model.device_state.update(c.x, c.y, arm)
        r = c.rec[e]
        assert len(r.rl_users) == 200
        res = ev.test_kuaishou(model, env=env, dataset_val=ds, is_softmax=False, users=r.rl_users)
        got = np.array([float(res[k]) for k in ("click_loss", "CV", "CV_turn", "ctr", "len_tra", "R_tra")])
        want = r.rl_res[:6]
        print(f"epoch {e}: test_kuaishou {got.tolist()}  recorded {want.tolist()}")
        np.testing.assert_array_equal(got[[1, 2, 4]], want[[1, 2, 4]], err_msg=f"epoch {e}: counts")          # integer-derived
        np.testing.assert_allclose(got[[0, 3, 5]], want[[0, 3, 5]], rtol=1e-6, err_msg=f"epoch {e}")         # float sums
    with pytest.raises(ValueError):
        ev.test_kuaishou(model, env=env, dataset_val=ds, epsilon=0.1)
    res = ev.test_kuaishou(model, env=env, dataset_val=ds, num_trajectory=7)                                  # users drawn here
    assert res["len_tra"] >= 1


# ---- shapes where the kernels can go wrong, against the host restatement ------------------------------------------------------------
def _against_host(K, d, B, n_rows, seed, heavy=None, n_outside=5, epochs=1, every_arm=True):
    """Device against the host restatement on a log drawn like case 1's (its id ranges, its skew, every arm with a row): bits for A
    and b, the error protocol with case 1's E_ref for the rest.  The yardstick is the restatement's extended mode: measured against
    exact rational arithmetic on these very logs, the float64 mode (a batched np.linalg.inv, as good as the reference's) is wrong by
    up to 60 x case 1's E_ref here, so nothing could pass against it, while the extended mode stays below 0.03 x E_ref."""
    from cirs_hip.linucb import DeviceLinUCB
    classes, feats, x, y, user_ids = linucbcase.synthetic_problem(seed, K, d, n_rows, heavy=heavy, n_outside=n_outside, every_arm=every_arm)
    rng = np.random.RandomState(seed + 1)
    users = rng.choice(user_ids, B).astype(np.float64)
    val = rng.choice(len(x), min(len(x), 77), replace=False)
    arm = linucb_host.arm_of_rows(classes, x[:, 1])
    host, dev = linucb_host.HostLinUCB(K, d, 1.0, extended=True), DeviceLinUCB(K, d, 1.0)
    for _ in range(epochs):
        host.update(x, y, arm)
        dev.update(x, y, arm)
    assert np.array_equal(_np(dev.A), host.A) and np.array_equal(_np(dev.b), host.b), "A / b differ in bits"
    eref = CASES[1].rec[1].eref                                       # the data is drawn at case 1's id ranges
    what = f"K={K} d={d} B={B} "
    _, theta = host.solve()
    hbest, hbest_mean, hucb, hmean, hvar = host.score(users, feats)
    best, best_mean, ucb, mean, var = (_np(t) for t in dev.score(users, feats, want_full=True))
    linucbcase.check(what + "theta", _np(dev.theta), theta.astype(np.float64), eref["theta"])
    linucbcase.check(what + "mean", mean, hmean, eref["mean"])
    linucbcase.check(what + "var", var, hvar, eref["var"])
    linucbcase.check(what + "ucb", ucb, hucb, eref["ucb"])
    linucbcase.check(what + "y_predict", _np(dev.predict(x[val], arm[val])), host.predict(x[val], arm[val]), eref["y_predict"])
    assert np.array_equal(best, ucb.argmax(1)) and np.array_equal(best_mean, mean[np.arange(B), best])
    if K > 1:        # the arg-max is the host's wherever the host's top two are further apart than 1e4 x the two sides' largest difference
        top2 = np.sort(hucb, axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) >= 1e4 * np.abs(ucb - hucb).max()
        assert np.array_equal(best[clear], hbest[clear])
    return dev, host, (classes, feats, x, y, arm)


@pytest.mark.parametrize("K,d,B", [(1, 7, 1), (63, 2, 5), (64, 16, 77), (65, 7, 5), (257, 7, 77), (257, 16, 1), (5, 3, 5)])
def test_shapes_against_the_host_restatement(K, d, B):
    _against_host(K, d, B, n_rows=30 * K, seed=K + d, heavy=18 * K if K > 1 else None)


def test_one_arm_holds_every_row():
    dev, host, (_, _, _, _, arm) = _against_host(3, 7, 5, n_rows=1000, seed=11, heavy=1000, n_outside=0, every_arm=False)
    assert np.bincount(arm, minlength=3).max() == 1000
    untouched = np.flatnonzero(np.bincount(arm, minlength=3) == 0)
    assert len(untouched) == 2 and np.array_equal(_np(dev.A)[untouched], np.tile(np.identity(7), (2, 1, 1)))


def test_log_without_a_matching_row():
    from cirs_hip.linucb import DeviceLinUCB
    classes, feats, x, y, _ = linucbcase.synthetic_problem(5, 9, 7, 30)
    dev = DeviceLinUCB(9, 7, 0.5)
    dev.update(x, y, np.full(len(x), -1, np.int64))
    assert np.array_equal(_np(dev.A), np.tile(np.identity(7), (9, 1, 1))) and not _np(dev.b).any()
    assert np.array_equal(_np(dev.A_inv), np.tile(np.identity(7), (9, 1, 1))) and not _np(dev.theta).any()
    assert not _np(dev.predict(x, np.full(len(x), -1, np.int64))).any()


def test_order_inside_an_arm_is_the_logs():
    """The rows of an arm interleave with the other arms' rows in the log; adding them in any other order changes the bits of the sums
    (shown on the host with the reversed log), and the device gives the bits of the log order."""
    dev, host, (classes, feats, x, y, arm) = _against_host(12, 7, 5, n_rows=400, seed=23, heavy=150, every_arm=False)
    rows = np.flatnonzero(arm == np.bincount(arm[arm >= 0]).argmax())
    assert (np.diff(rows) > 1).any(), "the largest arm's rows must not be contiguous in the log"
    back = linucb_host.HostLinUCB(12, 7, 1.0)
    back.update(x[::-1], y[::-1], arm[::-1])
    assert not np.array_equal(back.A, host.A), "the reversed log must give other bits: otherwise this test shows nothing"
    np.testing.assert_allclose(back.A, host.A, rtol=1e-12)


def test_select_arm_and_untouched_arms():
    from core.policy.linucb import linucb_policy
    K, d, alpha = 6, 7, 0.5
    classes, feats, x, y, _ = linucbcase.synthetic_problem(31, K, d, 60)
    arm = linucb_host.arm_of_rows(classes, x[:, 1])
    arm[arm >= 4] = -1                                   # arms 4 and 5 are never updated: they tie at alpha |x|
    model, host = linucb_policy(K, d, alpha), linucb_host.HostLinUCB(K, d, alpha)
    model.device_state.update(x, y, arm)
    host.update(x, y, arm)
    xq = np.r_[3000.0, 2.0, feats[2]]
    for k in (4, 5):
        np.testing.assert_allclose(model.linucb_arms[k].calc_UCB(xq)[0, 0], alpha * np.linalg.norm(xq), rtol=1e-14)
        assert model.linucb_arms[k].calc_reward(xq)[0, 0] == 0.0
    ucb = _np(model.device_state.score_x(xq)[0])
    assert ucb[4] == ucb[5] == ucb.max() and (ucb[:4] < ucb[4]).all()
    picks = []
    for seed in range(12):
        np.random.seed(seed)
        got = model.select_arm(xq)
        np.random.seed(seed)
        assert got == host.select_arm(xq)
        picks.append(int(got))
    assert set(picks) == {4, 5}
    # no tie: x along the rows of arm 0
    x0 = x[np.flatnonzero(arm == 0)[0]] if (arm == 0).any() else xq
    np.random.seed(1)
    got = model.select_arm(x0)
    np.random.seed(1)
    assert got == host.select_arm(x0)
