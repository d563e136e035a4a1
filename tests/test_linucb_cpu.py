"""The host restatement of the LinUCB baseline (cirs_hip/linucb_host.py) against the recording of the reference
(tests/golden/linucb.npz), and the library's argument refusals; no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linucbcase  # noqa: E402

from cirs_hip import abi, linucb_host  # noqa: E402

CASES = linucbcase.load()
METRICS = {"mae": lambda y, y_predict: torch.nn.functional.l1_loss(torch.from_numpy(y), torch.from_numpy(y_predict)).numpy(),
           "mse": lambda y, y_predict: torch.nn.functional.mse_loss(torch.from_numpy(y), torch.from_numpy(y_predict)).numpy()}


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_host_restatement_matches_the_recording(ci):
    c = CASES[ci]
    host = linucb_host.HostLinUCB(c.K, c.d, c.alpha)
    arm = linucb_host.arm_of_rows(c.classes, c.x[:, 1])
    val_arm = linucb_host.arm_of_rows(c.classes, c.val_x[:, 1])
    assert (arm < 0).sum() >= 1 and (val_arm < 0).sum() == 1
    for e in c.epochs:
        host.update(c.x, c.y, arm)
        r = c.rec[e]
        assert np.array_equal(host.A, r.A) and np.array_equal(host.b, r.b), f"case {ci} epoch {e}: A / b differ in bits"
        if e not in c.full:
            continue
        what = f"case {ci} epoch {e} host "
        A_inv, theta = host.solve()
        best, best_mean, ucb, mean, var = host.score(c.users, c.photo_values)
        y_predict = host.predict(c.val_x, val_arm).reshape(-1, 1)
        linucbcase.check(what + "theta", theta, r.theta_exact, r.eref["theta"])
        linucbcase.check(what + "mean", mean, r.mean_exact, r.eref["mean"])
        linucbcase.check(what + "var", var, r.var_exact, r.eref["var"])
        linucbcase.check(what + "ucb", ucb, r.ucb_exact, r.eref["ucb"])
        linucbcase.check(what + "y_predict", y_predict, r.ypred_exact, r.eref["y_predict"])
        assert c.kept.sum() >= 36
        assert np.array_equal(c.classes[best][c.kept], r.rec_item[c.kept])
        assert np.array_equal(c.classes[r.ucb_ref.argmax(1)], r.rec_item)
        linucbcase.check(what + "returned mean", best_mean[c.kept], r.mean_exact[np.arange(len(best)), best][c.kept], r.eref["mean"],
                         scale=r.mean_exact)
        # the metric functions of the scripts on the recorded predictions give the recorded metrics: shapes and dtypes are the reference's
        for k, name in enumerate(("mae", "mse")):
            np.testing.assert_allclose(float(METRICS[name](c.val_y, r.ypred_ref)), r.metrics[k], rtol=1e-12)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_extended_mode_is_a_yardstick(ci):
    """The restatement's extended mode (np.longdouble: 11 more bits) against the recorded exact values: it takes their place at the
    shapes of the GPU tests that have none.  11 bits are a factor 2048; the bar leaves a factor 100 of that."""
    c = CASES[ci]
    host = linucb_host.HostLinUCB(c.K, c.d, c.alpha, extended=True)
    arm = linucb_host.arm_of_rows(c.classes, c.x[:, 1])
    for e in c.epochs:
        host.update(c.x, c.y, arm)
        if e not in c.full:
            continue
        r = c.rec[e]
        _, _, ucb, mean, var = host.score(c.users, c.photo_values)
        y_predict = host.predict(c.val_x, linucb_host.arm_of_rows(c.classes, c.val_x[:, 1])).reshape(-1, 1)
        for q, got, exact in (("theta", host.solve()[1].astype(np.float64), r.theta_exact), ("mean", mean, r.mean_exact),
                              ("var", var, r.var_exact), ("ucb", ucb, r.ucb_exact), ("y_predict", y_predict, r.ypred_exact)):
            E = linucbcase.rel_err(got, exact)
            print(f"case {ci} epoch {e} extended {q}: E {E:.3e}  E_ref {r.eref[q]:.3e}  ratio {E / r.eref[q]:.3g}")
            assert E <= r.eref[q] / 20


def test_recording_is_what_the_tests_assume():
    c0, c1, c2 = CASES
    assert (c0.K, c0.d, len(c0.x), c0.alpha, c0.epochs, c0.full) == (80, 7, 600, 0.25, [1, 2], [2])
    assert (c1.K, c1.d, len(c1.x), c1.alpha, c1.epochs[-1], c1.full) == (67, 7, 2000, 1.0, 5, [1, 5])
    assert (c2.K, c2.d, len(c2.x), c2.epochs) == (5, 4, 40, [1])
    rows = np.bincount(linucb_host.arm_of_rows(c0.classes, c0.x[:, 1]) + 1, minlength=c0.K + 1)
    assert rows[0] >= 20 and (rows[1:] == 0).any() and (rows[1:] == 1).any() and (rows[1:] > 128).any()
    assert np.bincount(linucb_host.arm_of_rows(c1.classes, c1.x[:, 1]) + 1).max() >= 1200
    assert c1.x[:, 0].max() == 7175 and c1.x[:, 1].max() == 10727
    for c in CASES:
        assert len(c.val_x) == 77 and len(c.users) == 40 and c.kept.sum() >= 36
        for e in c.full:
            assert all(c.rec[e].eref[q] > 0 for q in linucbcase.QUANTITIES)


def test_tie_pick_follows_the_reference_procedure():
    # the first arm at the maximum enters the candidate list twice, later arms at the maximum once: with [0, 0, 2] as candidates
    np.random.seed(3)
    want = [int(np.random.choice([0, 0, 2])) for _ in range(20)]
    np.random.seed(3)
    got = [int(linucb_host.tie_pick(np.array([1.5, 0.2, 1.5, -3.0]))) for _ in range(20)]
    assert got == want
    with pytest.raises(ValueError):       # nothing exceeds the starting bound of -1: np.random.choice of an empty list
        linucb_host.tie_pick(np.array([-2.0, -1.0]))


def test_library_refusals_need_no_gpu():
    lib = abi.lib()
    for d in (1, 17):
        for rc in (lib.cirs_linucb_update(None, None, 4, d, None, d, 3, None, None, 3, None, None),
                   lib.cirs_linucb_solve(None, None, 4, d, None, 0, None, None, None),
                   lib.cirs_linucb_score(None, None, 4, d, None, 2, None, None, 0.5, None, None, None, None, None, None),
                   lib.cirs_linucb_predict(None, 4, d, None, d, None, 3, None, None)):
            assert rc == -3 and b"d must lie in [2, 16]" in lib.cirs_last_error()
    assert lib.cirs_linucb_update(None, None, 4, 7, None, 7, 3, None, None, 0, None, None) == 0       # m = 0: nothing to add
    assert lib.cirs_linucb_update(None, None, 0, 7, None, 7, 3, None, None, 3, None, None) == 0       # K = 0
    assert lib.cirs_linucb_solve(None, None, 0, 7, None, 0, None, None, None) == 0
    assert lib.cirs_linucb_score(None, None, 0, 7, None, 2, None, None, 0.5, None, None, None, None, None, None) == 0
    assert lib.cirs_linucb_predict(None, 0, 7, None, 7, None, 0, None, None) == 0
    assert lib.cirs_linucb_update(None, None, 4, 7, None, 7, 3, None, None, 3, None, None) == -1 and b"null" in lib.cirs_last_error()
    one = np.zeros(64)
    assert lib.cirs_linucb_predict(one.ctypes.data, 1, 7, one.ctypes.data, 6, one.ctypes.data, 1, one.ctypes.data, None) == -1
    assert b"ld < d" in lib.cirs_last_error()


def test_recommend_k_item_refuses_other_exploration():
    from core.policy.linucb import linucb_policy
    model = linucb_policy(5, 4, 0.5)
    with pytest.raises(ValueError):
        model.recommend_k_item(3, None, epsilon=0.1)
    with pytest.raises(ValueError):
        model.recommend_k_item(3, None, is_ucb=True)
