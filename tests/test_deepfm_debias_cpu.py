"""CPU: the host side of the two debiasing baselines -- the torch restatement of the training step (cirs_hip.deepfm_host) against the
test oracle (loss kind 0) and against the reference recordings (kinds 1 and 2), the numpy side of the score columns against the
recorded ones, and what `compile` accepts."""
import numpy as np
import pytest
import torch

import debiascase
import nn_oracle
import traincase
from cirs_hip import deepfm_host


def test_host_restatement_kind0_equals_the_oracle(golden_dir):
    c = traincase.load(golden_dir)[0]
    want_l, want_first, want_final = nn_oracle.deepfm_train(c["init"], c["x"], c["y"], c["score"], c["n"], c["steps"], c["use_ab"], c["lambda_ab"])
    got_l, kept, got_final = deepfm_host.torch_train(c["init"], c["x"], c["y"], c["score"], c["n"], kind="pairwise", use_ab=c["use_ab"],
                                                     lambda_ab=c["lambda_ab"], keep=(0,))
    # Both are fp32 autograd over the same formulas; the graphs differ in the order in which a table row used by the positive pair, the
    # negative pair and the regulariser collects its three gradient terms, so the sums differ by fp32 rounding (a few 1e-7 relative)
    # and Adam carries that into the parameters: the bar is the one of every training comparison here (traincase.compare_params).
    np.testing.assert_allclose(got_l[:, [0, 4]], want_l, rtol=1e-6)
    traincase.compare_params(kept[0], want_first, c["init"], "kind 0 first step")
    traincase.compare_params(got_final, want_final, c["init"], "kind 0 final")
    assert set(got_final) == set(want_final)
    np.testing.assert_allclose(got_l[:, 1] + got_l[:, 2] + c["lambda_ab"] * got_l[:, 3], got_l[:, 0], rtol=1e-6)


def test_host_restatement_reproduces_the_reference_recordings(golden_dir):
    cases = debiascase.load_train(golden_dir)
    assert [c["kind"] for c in cases] == ["ips", "ips", "pd", "pd"]
    for ci, c in enumerate(cases):
        got_l, kept, final = deepfm_host.torch_train(c["init"], c["x"], c["y"], c["score"], c["n"], kind=c["kind"], keep=(0,))
        assert got_l.shape == (c["steps"], 5)
        np.testing.assert_allclose(got_l[:, [0, 4]], c["losses"], rtol=3e-5, err_msg=f"case {ci}")
        traincase.compare_params(kept[0], c["first"], c["init"], f"case {ci} first step")
        traincase.compare_params(final, c["final"], c["init"], f"case {ci} final")
        assert set(final) == set(c["final"])


def test_host_restatement_refuses_alpha_beta_with_the_debias_losses(golden_dir):
    c = debiascase.load_train(golden_dir)[0]
    for kind in ("ips", "pd"):
        with pytest.raises(ValueError):
            deepfm_host.torch_train(c["init"], c["x"], c["y"], c["score"], c["n"], kind=kind, use_ab=True)


def test_score_tables_equal_the_recorded_columns(golden_dir):
    from cirs_hip.dataprep import ips_table, popularity_table, time_bin_bounds
    for si, s in enumerate(debiascase.load_scores(golden_dir)):
        photo, ts = s["photo"], s["timestamp"]
        n_items = int(photo.max()) + 1
        counts = debiascase.host_counts(photo, np.zeros(len(photo), np.int32), 1, n_items)
        assert np.array_equal(ips_table(counts)[0, photo][:, None], s["ips"]), f"score case {si}: ips"
        bounds = time_bin_bounds(ts.min(), ts.max(), s["num_bin"])
        bins = debiascase.host_bins(ts, bounds)
        counts = debiascase.host_counts(photo, bins, s["num_bin"], n_items)
        for gamma, want in s["pd"].items():
            table = popularity_table(counts, gamma)
            got = np.where(bins >= 0, table[np.maximum(bins, 0), photo], 0.0)[:, None]
            assert np.array_equal(got, want), f"score case {si}: pd gamma {gamma}"
    # the all-equal-timestamp log: the closed last bin takes every row
    assert (bins == s["num_bin"] - 1).all()


def test_compile_accepts_the_debias_losses_and_refuses_a_plain_function():
    from core.inputs import SparseFeatP
    from core.user_model_pairwise import (UserModel_Pairwise, loss_kuaishou_IPS_pairwise, loss_kuaishou_PD_pairwise,
                                          make_loss_kuaishou_pairwise)
    from deepctr_torch.inputs import DenseFeat
    cols = [SparseFeatP("user_id", 5, embedding_dim=4), SparseFeatP("photo_id", 6, embedding_dim=4)] + \
           [SparseFeatP(f"feat{i}", 7, embedding_dim=4, embedding_name="feat", padding_idx=0) for i in range(4)] + [DenseFeat("photo_duration", 1)]
    ab = [SparseFeatP("alpha_u", 5, embedding_dim=1), SparseFeatP("beta_i", 6, embedding_dim=1)]
    build = lambda ab_columns=None: UserModel_Pairwise(cols, [DenseFeat("y", 1)], "regression", 1, dnn_hidden_units=(64, 64), ab_columns=ab_columns)  # noqa: E731
    for loss in (loss_kuaishou_IPS_pairwise, loss_kuaishou_PD_pairwise, make_loss_kuaishou_pairwise(2.0)):
        m = build()
        m.compile(optimizer="adam", loss_func=loss)
        assert m.loss_func is loss
    build(ab).compile(optimizer="adam", loss_func=make_loss_kuaishou_pairwise(2.0))
    with pytest.raises(AssertionError):
        build().compile(optimizer="adam", loss_func=lambda y, yp, yn, s: ((yp - y) ** 2).mean())
    for loss in (loss_kuaishou_IPS_pairwise, loss_kuaishou_PD_pairwise):      # both scripts build the model without ab_columns
        with pytest.raises(AssertionError):
            build(ab).compile(optimizer="adam", loss_func=loss)
    # the torch formulas the losses carry for host use are the restatement's
    g = torch.Generator().manual_seed(0)
    y, yp, yn, sc = (torch.rand(9, 1, generator=g) for _ in range(4))
    for loss, kind in ((loss_kuaishou_IPS_pairwise, "ips"), (loss_kuaishou_PD_pairwise, "pd")):
        ly, bpr, _ = deepfm_host.loss_terms(kind, y, yp, yn, sc)
        assert torch.equal(loss(y, yp, yn, sc), ly + bpr) and loss.loss_kind == kind
