"""CPU: the validation pass's host side -- the torch restatements of the two forwards against the reference's recorded predict_data,
the tagged metrics as host callables against its recorded evaluate_data, the declared entry points, the id check of ValSet."""
import os

import numpy as np
import pytest
import torch

import valcase


def test_host_restatements_reproduce_the_recorded_predictions(golden_dir):
    from cirs_hip import deepfm_host, dice_host
    cases = valcase.load(golden_dir)
    assert [(c["kind"], c["E"]) for c in cases] == [("pairwise", 8), ("pairwise", 16), ("dice", 8), ("dice", 16)]
    for c in cases:
        assert c["x"].shape == (77, 7) and c["pred"].shape == (77, 1) and c["pred"].dtype == np.float64
        u, p, f = c["x"][:, 0], c["x"][:, 1], c["x"][:, 2:6]
        assert {0, c["U"] - 1} <= set(u) and {0, c["I"] - 1} <= set(p) and {0, c["F"] - 1} <= set(f.ravel())
        prm = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
        X = torch.as_tensor(c["x"], dtype=torch.float32)
        got = (deepfm_host.pair_forward if c["kind"] == "pairwise" else dice_host.forward)(prm, X).numpy()
        np.testing.assert_allclose(got, c["pred"][:, 0], rtol=1e-5, atol=3e-6)


def test_tagged_metrics_are_the_scripts_lambdas(golden_dir):
    from core.user_model import metric_mae, metric_mse
    assert metric_mae.device_metric == "mae" and metric_mse.device_metric == "mse"
    for c in valcase.load(golden_dir):
        mae, mse = metric_mae(c["y"], c["pred"]), metric_mse(c["y"], c["pred"])
        assert np.asarray(mae).dtype == np.float64 and np.asarray(mse).dtype == np.float64 and np.ndim(mae) == 0
        np.testing.assert_allclose(float(mae), c["eval"]["mae"], rtol=1e-12)
        np.testing.assert_allclose(float(mse), c["eval"]["mse"], rtol=1e-12)
    fits = [c["fit"] for c in valcase.load(golden_dir) if "fit" in c]
    assert len(fits) == 2
    for f in fits:      # the condition of the fit_data check: consecutive records differ by at least 1 %
        mae = f["logs"][:, 1]
        assert f["logs"].shape == (3, 3) and np.isnan(f["logs"][0, 0]) and (np.abs(np.diff(mae)) / mae[:-1] >= 0.01).all()


def test_abi_declares_the_validation_entries():
    from cirs_hip import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "cirs_hip.h")) as fh:
        header = fh.read()
    for name in ("cirs_deepfm_validate_workspace_bytes", "cirs_deepfm_validate", "cirs_dice_validate_workspace_bytes", "cirs_dice_validate"):
        assert name in abi.SIGNATURES and name + "(" in header
    assert len(abi.SIGNATURES["cirs_deepfm_validate"][1]) == 13 and len(abi.SIGNATURES["cirs_dice_validate"][1]) == 13


@pytest.mark.parametrize("col,bad", [(0, 50), (0, -1), (1, 80), (3, 32), (5, -2)])
def test_valset_refuses_an_id_outside_its_table_before_any_device_work(golden_dir, col, bad):
    from cirs_hip import abi
    from cirs_hip.userval import ValSet
    c = valcase.load(golden_dir)[0]
    cfg = abi.DeepFMCfg(n_user_vocab=c["U"], n_item_vocab=c["I"], n_feat_vocab=c["F"], emb_dim=c["E"], hidden=64)
    x = c["x"].copy()
    x[40, col] = bad
    with pytest.raises(IndexError):
        ValSet(x, c["y"], cfg, device="cuda")       # raised on the host: no device is touched
    with pytest.raises(ValueError):
        ValSet(c["x"][:, :6], c["y"], cfg, device="cuda")
    with pytest.raises(ValueError):
        ValSet(c["x"][:0], c["y"][:0], cfg, device="cuda")
