"""The host restatement of the DICE baseline (cirs_hip/dice_host.py) and the loader's score rule against the recording of the
reference (tests/golden/usertrain_dice.npz); no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dicecase  # noqa: E402
import traincase  # noqa: E402

from cirs_hip import dice_host  # noqa: E402

REC = dicecase.load()


@pytest.fixture(scope="module", params=range(len(REC["cases"])))
def trained(request):
    c = REC["cases"][request.param]
    losses, kept, final = dice_host.torch_train(c["init"], c["x"], c["y"], c["score"], c["n"], steps=c["steps"], keep=(0,), **dicecase.L2)
    return c, losses, kept[0], final


def test_host_losses_match_the_recording(trained):
    c, losses, _, _ = trained
    print("host {loss, reg}", losses[:, [0, 5]].tolist(), "recorded", c["losses"].tolist())
    np.testing.assert_allclose(losses[:, 0], c["losses"][:, 0], rtol=dicecase.LOSS_RTOL)
    np.testing.assert_allclose(losses[:, 5], c["losses"][:, 1], rtol=dicecase.LOSS_RTOL)
    np.testing.assert_allclose(losses[:, 1:5].sum(1), losses[:, 0], rtol=1e-6)


def test_host_parameters_match_the_recording(trained):
    c, _, first, final = trained
    assert set(final) == set(c["final"])
    traincase.compare_params(first, c["first"], c["init"], "host restatement, first step")
    traincase.compare_params(final, c["final"], c["init"], "host restatement, final")
    assert not final["embedding_dict.feat.weight"][0].any()


def test_all_plus_batch_has_no_int_term():
    c = REC["cases"][0]
    n = c["n"]
    assert (c["score"][n:2 * n] > 0).all()
    p = {k: torch.as_tensor(v) for k, v in c["init"].items()}
    t = lambda a: torch.as_tensor(a[n:2 * n], dtype=torch.float32)  # noqa: E731
    terms = dice_host.get_loss(p, t(c["x"]), t(c["y"]).reshape(-1), t(c["score"]).reshape(-1))
    assert float(terms[3]) == 0.0 and float(terms[2]) > 0.0


def test_loss_function_of_the_module_matches_the_recording():
    """loss_kuaishou_DICE as core.user_model_DICE exports it, over the host forwards, gives the recorded first-step loss."""
    from core.user_model_DICE import loss_kuaishou_DICE
    for c in REC["cases"]:
        n = c["n"]
        p = {k: torch.as_tensor(v) for k, v in c["init"].items()}
        x, y, s = (torch.as_tensor(a[:n], dtype=torch.float32) for a in (c["x"], c["y"], c["score"]))
        col = lambda v: v.unsqueeze(1)  # noqa: E731
        yp = col(dice_host.main_forward(p, x[:, :9])); yn = col(dice_host.main_forward(p, torch.cat([x[:, :2], x[:, 9:]], 1)))
        ypi, yni = col(dice_host.ui_forward(p, x[:, 0], x[:, 2], "int")), col(dice_host.ui_forward(p, x[:, 0], x[:, 9], "int"))
        ypc, ync = col(dice_host.ui_forward(p, x[:, 1], x[:, 3], "con")), col(dice_host.ui_forward(p, x[:, 1], x[:, 10], "con"))
        loss = float(loss_kuaishou_DICE(y, yp, yn, ypi, yni, ypc, ync, s))
        np.testing.assert_allclose(loss, c["losses"][0, 0], rtol=dicecase.LOSS_RTOL)
        assert loss_kuaishou_DICE.loss_kind == "dice"


def test_host_forward_matches_the_recording():
    f = REC["forward"]
    p = {k: torch.as_tensor(v) for k, v in REC["cases"][0]["init"].items()}
    y = dice_host.forward(p, torch.as_tensor(f["x"], dtype=torch.float32)).numpy()
    np.testing.assert_allclose(y, f["y"][:, 0], rtol=1e-5, atol=2e-6)     # the bar of the DeepFM forward tests (tests/test_gpu_deepfm.py)


def test_score_column_equals_the_recording():
    from core.user_data import dice_conformity_score
    s = REC["score"]
    got = dice_conformity_score(s["photo"], s["neg"], s["photo"])
    assert got.shape == s["score"].shape and got.dtype.kind == "i"
    assert np.array_equal(got, s["score"])
    assert set(np.unique(got)) == {-1, 1}
