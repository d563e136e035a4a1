"""CPU: the training surface of the VirtualTaobao two-task MLP baselines without a device -- the recorded reference steps pin the
formula (the plain-torch restatement of cirs_hip/mmoe_host.py reproduces them), the inputs of the device comparison at the script shape
leave the device its room, compile() accepts what the device step implements and refuses the rest, the struct layout, and the log
reader of MLP-taobao.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlpcase
import traincase
import vtbstaticcase
from cirs_hip import abi, mmoe_host


def test_torch_restatement_reproduces_the_reference_fit_data(golden_dir):
    cases = mlpcase.load(golden_dir)
    assert [(c["dnn"], c["experts"], c["expert_dim"], c["n"], c["N"]) for c in cases] == mlpcase.CASES
    for ci, c in enumerate(cases):
        assert [(k, v.shape) for k, v in c["init"].items()] == mmoe_host.mlp_shapes(c["dnn"], c["experts"], c["expert_dim"])
        assert mmoe_host.mlp_shape_of(c["init"]) == (list(c["dnn"]), c["experts"], c["expert_dim"])
        click = c["y"][:, 27]
        assert 0.2 < (click == 0).mean() < 0.5 and (click > 0).any() and c["x"].shape == (c["N"], 91) and c["y"].shape == (c["N"], 28)
        losses, kept, final = mmoe_host.mlp_torch_train(c["init"], c["x"], c["y"], c["n"], steps=c["steps"], l2_linear=mlpcase.L2_LINEAR,
                                                        l2_all=mlpcase.L2_ALL, keep=(0,))
        print(f"case {ci}: losses {losses.tolist()} recorded {c['losses'].tolist()}")
        np.testing.assert_allclose(losses, c["losses"], rtol=3e-5, err_msg=f"case {ci}")
        traincase.compare_params(kept[0], c["first"], c["init"], f"case {ci} first step")
        traincase.compare_params(final, c["final"], c["init"], f"case {ci} final")
    assert cases[1]["N"] - 2 * cases[1]["n"] == 26       # the second case ends on a short batch: 37 + 37 + 26 rows


def test_click_mask_and_unused_score(golden_dir):
    """Rows without a click teach the action task nothing; a plain mse over the 27 columns (a plausible misreading) misses the record."""
    c = mlpcase.load(golden_dir)[0]
    p = {k: torch.as_tensor(v) for k, v in c["init"].items()}
    x, y = (torch.as_tensor(a[:c["n"]], dtype=torch.float32) for a in (c["x"], c["y"]))
    pred = mmoe_host.mlp_forward(p, x)
    np.testing.assert_allclose(float(mmoe_host.loss_taobao_mlp(pred, y)), c["losses"][0, 0], rtol=3e-5)
    plain = float(torch.nn.functional.mse_loss(pred[:, :27], y[:, :27]) + torch.nn.functional.mse_loss(pred[:, 27:], y[:, 27:]))
    assert abs(plain - c["losses"][0, 0]) > 1e-2 * c["losses"][0, 0]
    y2 = y.clone()
    y2[y[:, 27] == 0, :27] += 5.0                         # the masked rows' action targets do not matter
    assert float(mmoe_host.loss_taobao_mlp(pred, y2)) == float(mmoe_host.loss_taobao_mlp(pred, y))


def test_script_shape_inputs_leave_the_device_its_room():
    """The GPU comparison at (256, 256), batch 100: fp32 against float64 of the same restatement passes compare_params and at least
    0.999 of every tensor's entries sit inside the tight bar, so the 0.5 % allowance is the device's."""
    init, x, y, batch = mlpcase.gpu_case("script")
    assert [v.shape[0] for k, v in init.items() if k.startswith("dnn.") and k.endswith("weight")] == [256, 256] and batch == 100
    steps = mlpcase.GPU_STEPS
    kw = dict(steps=steps, l2_linear=mlpcase.L2_LINEAR, l2_all=mlpcase.L2_ALL, keep=(0,))
    l32, k32, f32 = mmoe_host.mlp_torch_train(init, x, y, batch, **kw)
    l64, k64, f64 = mmoe_host.mlp_torch_train(init, x, y, batch, dtype=torch.float64, **kw)
    share = min(mlpcase.tight_share(k32[0], k64[0]), mlpcase.tight_share(f32, f64))
    print(f"(256, 256) dnn scale {mlpcase.dnn_scale((256, 256)):.4f}: losses {l32[:, 0].tolist()}; tight share {share:.4f}; "
          f"loss rel. error {np.abs(l32 / l64 - 1).max():.2e}")
    traincase.compare_params(k32[0], k64[0], init, "fp32 vs float64, first step")
    traincase.compare_params(f32, f64, init, "fp32 vs float64, final")
    assert share >= 0.999
    np.testing.assert_allclose(l32, l64, rtol=3e-6)
    assert l32[:, 0].min() > 1.0                          # the loss is no round-off quantity


def test_compile_accepts_the_two_task_build_and_refuses_the_rest():
    import mmoecase
    from core.user_model_mmoe import loss_taobao, loss_taobao_mlp
    for shape in (dict(dnn=(256, 256)), dict(dnn=(96,), num_experts=2, expert_dim=5), dict(dnn=(40, 72, 24), num_experts=3, expert_dim=6)):
        m = vtbstaticcase.two_task_model(stressed=False, **shape)
        m.compile(optimizer="adam", loss_func=loss_taobao_mlp, metrics=None)
        assert m.optim == "adam" and m.metrics_names == ["loss"] and m.RL_eval_fun is None
    m.compile(torch.optim.Adam(m.parameters(), lr=3e-4), loss_func=loss_taobao_mlp)
    assert m._adam["lr"] == 3e-4
    fn = lambda model: {}   # noqa: E731
    m.compile_RL_test(fn)
    assert m.RL_eval_fun is fn
    with pytest.raises(ValueError, match="one regression task"):          # the two-task model with the one-task marker
        m.compile(optimizer="adam", loss_func=loss_taobao)
    with pytest.raises(ValueError, match="two-task"):                     # a one-task model with the new marker
        mmoecase.model((64, 64)).compile(optimizer="adam", loss_func=loss_taobao_mlp)
    with pytest.raises(ValueError, match="Adam"):
        m.compile(optimizer="sgd", loss_func=loss_taobao_mlp)
    with pytest.raises(ValueError, match="Adam"):
        m.compile(torch.optim.SGD(m.parameters(), lr=0.1), loss_func=loss_taobao_mlp)
    with pytest.raises(ValueError, match="loss_taobao"):
        m.compile(optimizer="adam", loss_func=lambda *a: 0)
    for shape in (dict(dnn=(300,)), dict(dnn=(32, 32, 32, 32)), dict(dnn=(64,), num_experts=9, expert_dim=8)):   # outside the evaluator's set
        with pytest.raises(ValueError, match="static baselines"):
            vtbstaticcase.two_task_model(stressed=False, **shape).compile(optimizer="adam", loss_func=loss_taobao_mlp)
    with pytest.raises(RuntimeError, match="marker"):
        loss_taobao_mlp(None, None, None, None)
    # the one-task path keeps its own rule
    with pytest.raises(ValueError, match="64, 128"):
        mmoecase.model((32, 32)).compile(optimizer="adam", loss_func=loss_taobao)


def test_struct_layout_matches_the_header():
    assert C.sizeof(abi.VtbMmoeShape) == 10 * 4
    assert C.sizeof(abi.MlpTrainCfg) == 10 * 4 + 6 * 4
    assert abi.MlpTrainCfg.shape.offset == 0 and abi.MlpTrainCfg.l2_linear.offset == 40 and abi.MlpTrainCfg.eps.offset == 60
    for name in ("cirs_mlp_train_param_count", "cirs_mlp_train_workspace_bytes", "cirs_mlp_train_step", "cirs_mlp_train_epoch"):
        assert name in abi.SIGNATURES
    assert len(abi.SIGNATURES["cirs_mlp_train_step"][1]) == 13 and len(abi.SIGNATURES["cirs_mlp_train_epoch"][1]) == 16


def test_log_reader_returns_state_and_item_click_columns(tmp_path):
    from core.user_data_taobao import load_dataset_mlp_taobao
    rng = np.random.RandomState(0)
    rows = []
    for L in (5, 1, 9):
        user = (rng.rand(88) < 0.15).astype(float)
        for t in range(L):
            rows.append(np.concatenate([user, rng.randint(0, 10, 2), [t + 1], rng.uniform(-1, 1, 27), [rng.randint(0, 11)]]))
    rows = np.array(rows)
    with open(tmp_path / "dataset.txt", "w") as fh:
        for i, r in enumerate(rows):
            fh.write(("," if i % 2 else " ").join(repr(float(v)) for v in r) + "\n")      # both separators of the reference's reader
    ds, xc, yc = load_dataset_mlp_taobao(str(tmp_path / "dataset.txt"))
    assert [(f.name, f.dimension) for f in xc] == [("feat_user", 91)] and [(f.name, f.dimension) for f in yc] == [("feat_item", 27), ("y", 1)]
    assert ds.x_numpy.shape == (15, 91) and ds.y_numpy.shape == (15, 28) and len(ds) == 15
    np.testing.assert_array_equal(ds.x_numpy, rows[:, :91])
    np.testing.assert_array_equal(ds.y_numpy, rows[:, 91:])
    assert not np.asarray(ds.score).any()
