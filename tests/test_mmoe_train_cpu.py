"""CPU: the VirtualTaobao user-model training surface without a device -- the recorded reference steps pin the formula (a plain-torch
restatement, cirs_hip/mmoe_host.py, reproduces them), the numpy exposure sum equals the reference's, compile() accepts what the device
step implements and refuses the rest, and the data / artefact layout of the taobao training run."""
import os
import pickle

import numpy as np
import pytest
import torch

import mmoecase
import traincase
from cirs_hip import mmoe_host


def test_torch_restatement_reproduces_the_reference_fit_data(golden_dir):
    cases, _ = mmoecase.load(golden_dir)
    assert [(c["dnn"], c["n"], c["N"]) for c in cases] == [((64, 64), 100, 300), ((128, 128), 64, 192), ((64, 64), 37, 100)]
    for ci, c in enumerate(cases):
        assert [(k, v.shape) for k, v in c["init"].items()] == [(k, s) for k, s in mmoe_host.shapes(*c["dnn"])]
        losses, kept, final = mmoe_host.torch_train(c["init"], c["x"], c["y"], c["score"], c["n"], steps=c["steps"],
                                                    l2_linear=mmoecase.L2_LINEAR, l2_all=mmoecase.L2_ALL, keep=(0,))
        print(f"case {ci}: losses {losses.tolist()} recorded {c['losses'].tolist()}")
        np.testing.assert_allclose(losses, c["losses"], rtol=3e-5, err_msg=f"case {ci}")
        traincase.compare_params(kept[0], c["first"], c["init"], f"case {ci} first step")
        traincase.compare_params(final, c["final"], c["init"], f"case {ci} final")
    # the third case ends on a short batch: 37 + 37 + 26 rows
    assert cases[2]["N"] - 2 * cases[2]["n"] == 26


def test_regulariser_lists_are_what_the_recording_needs(golden_dir):
    """Dropping the biases / the gate from the decayed parameters (a plausible misreading) misses the recorded regulariser."""
    c = mmoecase.load(golden_dir)[0][0]
    full = mmoecase.L2_ALL * sum(float((v.astype(np.float64) ** 2).sum()) for v in c["init"].values()) + \
        mmoecase.L2_LINEAR * float((c["init"]["linear_model.weight"].astype(np.float64) ** 2).sum())
    np.testing.assert_allclose(full, c["losses"][0, 1], rtol=3e-5)
    no_bias = full - mmoecase.L2_ALL * sum(float((v.astype(np.float64) ** 2).sum()) for k, v in c["init"].items() if k.endswith("bias"))
    assert abs(no_bias - c["losses"][0, 1]) > 3e-5 * c["losses"][0, 1]


def test_numpy_exposure_equals_the_reference(golden_dir):
    _, e = mmoecase.load(golden_dir)
    lens = np.diff(np.append(np.flatnonzero(e["timestamp"] == 1), len(e["timestamp"])))
    assert len(lens) == 12 and 1 in lens and len(set(lens)) > 6
    for tau, want in zip(e["taus"], e["out"]):
        got = mmoe_host.exposure_virtualtaobao(e["timestamp"], e["action"], float(tau))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert (got[e["timestamp"] == 1] == 0).all()
        assert (got > 0).any() == (tau > 0)
    with pytest.raises(ValueError, match="open a session"):
        mmoe_host.exposure_virtualtaobao(e["timestamp"][1:], e["action"][1:], 1.0)


def test_compile_accepts_adam_with_loss_taobao_and_refuses_the_rest():
    from core.user_model_mmoe import loss_taobao
    from core.user_model_pairwise import UserModel_Pairwise
    from core.inputs import SparseFeatP
    from deepctr_torch.inputs import DenseFeat
    for dnn in ((64, 64), (128, 128), (64, 128)):
        m = mmoecase.model(dnn)
        m.compile(optimizer="adam", loss_func=loss_taobao, metrics=None)
        assert m.optim == "adam" and m.metrics_names == ["loss"]
    m.compile(torch.optim.Adam(m.parameters(), lr=3e-4), loss_func=loss_taobao)
    assert m._adam["lr"] == 3e-4
    with pytest.raises(ValueError, match="Adam"):
        m.compile(optimizer="sgd", loss_func=loss_taobao)
    with pytest.raises(ValueError, match="Adam"):
        m.compile(torch.optim.SGD(m.parameters(), lr=0.1), loss_func=loss_taobao)
    with pytest.raises(ValueError, match="loss_taobao"):
        m.compile(optimizer="adam", loss_func=lambda *a: 0)
    for dnn in ((32, 32), (64,), (64, 64, 64), (256, 128)):
        with pytest.raises(ValueError, match="64, 128"):
            mmoecase.model(dnn).compile(optimizer="adam", loss_func=loss_taobao)
    # the Kuaishou model keeps its own rule
    U, I, F, E = 5, 6, 7, 4
    xc = [SparseFeatP("user_id", U, embedding_dim=E), SparseFeatP("photo_id", I, embedding_dim=E)] + \
         [SparseFeatP(f"feat{i}", F, embedding_dim=E, embedding_name="feat", padding_idx=0) for i in range(4)] + [DenseFeat("photo_duration", 1)]
    pw = UserModel_Pairwise(xc, [DenseFeat("y", 1)], "regression", 1, dnn_hidden_units=(64, 64), seed=1, device="cpu")
    with pytest.raises(AssertionError, match="make_loss_kuaishou_pairwise"):
        pw.compile(optimizer="adam", loss_func=loss_taobao)


def _write_log(path, rng, lens):
    rows = []
    for L in lens:
        user = (rng.rand(88) < 0.15).astype(float)
        for t in range(L):
            rows.append(np.concatenate([user, rng.randint(0, 10, 2), [t + 1], rng.uniform(-1, 1, 27), [rng.randint(0, 11)]]))
    rows = np.array(rows)
    with open(path, "w") as fh:
        for i, r in enumerate(rows):
            sep = "," if i % 2 else " "           # both separators of the reference's reader
            fh.write(sep.join(repr(float(v)) for v in r) + "\n")
    return rows


def test_dataset_layout_and_artefact_keys(tmp_path):
    from core.user_data_taobao import load_dataset_virtualTaobao
    from core.user_model_mmoe import UserModel_MMOE
    from core.user_model_train import train_user_model_taobao
    rows = _write_log(str(tmp_path / "dataset.txt"), np.random.RandomState(0), [5, 1, 9])
    seen = {}

    def expo(df_x, tau):
        seen["cols"], seen["tau"] = list(df_x.columns), tau
        return mmoe_host.exposure_virtualtaobao(df_x["feat90"].to_numpy(), df_x[[f"y{i}" for i in range(27)]].to_numpy(), tau)

    ds, xc, yc = load_dataset_virtualTaobao(0.5, str(tmp_path / "dataset.txt"), exposure_fn=expo)
    assert seen["cols"] == [f"feat{i}" for i in range(91)] + [f"y{i}" for i in range(27)] and seen["tau"] == 0.5
    assert [(f.name, f.dimension) for f in xc] == [("user_feat", 91), ("feat_item", 27)] and [(f.name, f.dimension) for f in yc] == [("y", 1)]
    np.testing.assert_array_equal(ds.x_numpy, rows[:, :118])
    np.testing.assert_array_equal(ds.y_numpy, rows[:, 118:])
    assert ds.score.shape == (15, 1) and ds.score[0, 0] == 0 and ds.score[5, 0] == 0 and ds.score[6, 0] == 0 and (ds.score[1:5] > 0).all()
    # epoch=0: everything of the run except the device fit
    res = train_user_model_taobao(str(tmp_path / "dataset.txt"), save_root=str(tmp_path), exposure_fn=expo, epoch=0, dnn=(128, 128), message="T")
    root = tmp_path / "saved_models" / "VirtualTB-v0" / "MLP"
    assert res.paths.params == str(root / "MLP_params_T.pickle") and res.paths.state_dict == str(root / "MLP_T.pt")
    with open(res.paths.params, "rb") as fh:
        params = pickle.load(fh)
    assert set(params) == {"feature_columns", "y_columns", "num_tasks", "tasks", "task_logit_dim", "dnn_hidden_units", "seed", "device"}
    params["device"] = "cpu"                                   # the lines of CIRS-RL-taobao.py:134-142
    user_model = UserModel_MMOE(**params)
    sd = torch.load(res.paths.state_dict)
    assert all(v.device.type == "cpu" for v in sd.values())
    user_model.load_state_dict(sd)
    x = torch.as_tensor(rows[:4, :118], dtype=torch.float32)
    assert torch.equal(user_model(x), res.model(x))
