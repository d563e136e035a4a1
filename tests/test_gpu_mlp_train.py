"""GPU: training of the VirtualTaobao two-task MLP baselines on the device (csrc/mlp_train.hip) -- cirs_mlp_train_step against the
reference's own fit_data recordings and against the plain-torch restatement at the script shape and at the shapes where the row kernel
takes another path; bit-reproducibility and epoch == step loop; the fit_data / compile_RL_test / train_mlp_taobao surface end to end;
the refusals of the ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlpcase
import traincase
from cirs_hip import mmoe_host

pytestmark = pytest.mark.gpu


def _trainer(init, **kw):
    from cirs_hip.mmoe_train import MlpTrainer
    return MlpTrainer(init, l2_linear=mlpcase.L2_LINEAR, l2_all=mlpcase.L2_ALL, **kw)


def _steps(init, x, y, n, steps, keep=(0,)):
    tr = _trainer(init)
    losses, kept = [], {}
    for st in range(steps):
        lo = tr.step(x[st * n:(st + 1) * n], y[st * n:(st + 1) * n])
        losses.append(lo.cpu().numpy().copy())
        if st in keep:
            kept[st] = {k: v.cpu().numpy() for k, v in tr.state_dict().items()}
    return np.array(losses), kept, {k: v.cpu().numpy() for k, v in tr.state_dict().items()}, tr


def test_train_step_matches_reference_fit_data(golden_dir):
    for ci, c in enumerate(mlpcase.load(golden_dir)):
        losses, kept, final, _ = _steps(c["init"], c["x"], c["y"], c["n"], c["steps"])
        print(f"case {ci}: losses {losses.tolist()} recorded {c['losses'].tolist()}; tight share first {mlpcase.tight_share(kept[0], c['first']):.4f} "
              f"final {mlpcase.tight_share(final, c['final']):.4f}")
        np.testing.assert_allclose(losses, c["losses"], rtol=3e-5, err_msg=f"case {ci}")
        traincase.compare_params(kept[0], c["first"], c["init"], f"case {ci} first step")
        traincase.compare_params(final, c["final"], c["init"], f"case {ci} final")
        assert set(final) == set(c["final"])


@pytest.mark.parametrize("name", list(mlpcase.GPU_CASES))
def test_train_step_vs_torch(name):
    init, x, y, batch = mlpcase.gpu_case(name)
    steps = mlpcase.GPU_STEPS
    want_l, want_kept, want_final = mmoe_host.mlp_torch_train(init, x, y, batch, steps=steps, l2_linear=mlpcase.L2_LINEAR, l2_all=mlpcase.L2_ALL,
                                                              keep=(0,))
    assert want_l.shape == (steps, 2)
    got_l, got_kept, got_final, _ = _steps(init, x, y, batch, steps)
    print(f"{name}: losses {got_l.tolist()} torch {want_l.tolist()}; tight share first {mlpcase.tight_share(got_kept[0], want_kept[0]):.4f} "
          f"final {mlpcase.tight_share(got_final, want_final):.4f}")
    np.testing.assert_allclose(got_l, want_l, rtol=3e-5)
    traincase.compare_params(got_kept[0], want_kept[0], init, f"{name} first step")
    traincase.compare_params(got_final, want_final, init, f"{name} final")
    if mlpcase.GPU_CASES[name][4]:     # every click is 0: the action task's data gradient is exactly zero, only the regulariser moves its parameters
        assert y[:, 27].max() == 0
        tr = _trainer(init)
        before = tr.state_dict()
        tr.step(x[:batch], y[:batch])
        g = tr.gradients()
        for k in ("tower_network.0.weight", "out.0.bias", "mmoe_layer.gating_networks.0.weight"):
            assert torch.equal(g[k], (2.0 * mlpcase.L2_ALL) * before[k]), k
        assert not torch.equal(g["tower_network.1.weight"], (2.0 * mlpcase.L2_ALL) * before["tower_network.1.weight"])


def _snapshot(tr):
    return [t.clone() for t in (tr.flat, tr.adam_m, tr.adam_v, tr.grads)]


def test_bit_reproducible_and_epoch_equals_step_loop():
    N, bs = 1000, 96                                  # 11 steps, the last one of 40 rows
    init = mlpcase.stressed_init((72, 256))
    x, y = (torch.as_tensor(a, dtype=torch.float32).cuda() for a in mlpcase.inputs(N, seed=5))
    order = torch.randperm(N, generator=torch.Generator().manual_seed(0)).cuda()
    runs = []
    for _ in range(2):                                # two step-by-step runs from one snapshot
        tr = _trainer(init)
        losses = []
        for s0 in range(0, N, bs):
            idx = order[s0:s0 + bs]
            losses.append(tr.step(x[idx], y[idx]).clone())
        runs.append((_snapshot(tr), torch.stack(losses), tr.step_count))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1])
    tr = _trainer(init)
    ep_losses = tr.epoch(x, y, order, bs)
    assert ep_losses.shape == (11, 2) and tr.step_count == runs[0][2] == 11
    for a, b in zip(_snapshot(tr), runs[0][0]):
        assert torch.equal(a, b)
    assert torch.equal(ep_losses, runs[0][1])
    assert torch.isfinite(ep_losses).all()
    assert float((tr.flat - _trainer(init).flat).abs().min()) > 0       # every parameter moved (the regulariser reaches all of them)
    m, v = tr.moments()
    assert set(m) == set(v) == set(init)
    # a second epoch continues the optimiser state: equal to 11 more single steps
    ep2 = tr.epoch(x, y, order.flip(0), bs)
    tr_b = _trainer(init)
    tr_b.epoch(x, y, order, bs)
    for s0 in range(0, N, bs):
        idx = order.flip(0)[s0:s0 + bs]
        last = tr_b.step(x[idx], y[idx])
    assert torch.equal(tr.flat, tr_b.flat) and torch.equal(ep2[-1], last)


class _CB:
    def __init__(self):
        self.calls = []

    def on_train_begin(self): self.calls.append(("begin",))
    def on_train_end(self): self.calls.append(("end",))
    def on_epoch_begin(self, epoch): self.calls.append(("eb", epoch))
    def on_epoch_end(self, epoch, logs): self.calls.append(("ee", epoch, dict(logs)))


def _torch_epochs(init, ds, bs, epochs):
    """fit_data without shuffling in plain torch: an epoch ends on its own short batch, parameters AND the Adam state carry over."""
    n = len(ds)
    out = []
    P = {k: torch.nn.Parameter(torch.as_tensor(v).clone()) for k, v in init.items()}
    opt = torch.optim.Adam(list(P.values()), lr=1e-3)
    X, Y = torch.as_tensor(ds.x_numpy, dtype=torch.float32), torch.as_tensor(ds.y_numpy, dtype=torch.float32)
    for _ in range(epochs):
        total = 0.0
        for s0 in range(0, n, bs):
            sl = slice(s0, s0 + bs)
            loss = mmoe_host.loss_taobao_mlp(mmoe_host.mlp_forward(P, X[sl]), Y[sl])
            reg = mlpcase.L2_LINEAR * (P["linear_model.weight"] ** 2).sum() + sum(mlpcase.L2_ALL * (v ** 2).sum() for v in P.values())
            opt.zero_grad()
            (loss + reg).backward()
            opt.step()
            total += float(loss.detach()) + float(reg.detach())
        out.append(total / n)
    return out


def test_fit_data_surface(golden_dir, tmp_path):
    import functools
    import vtbcase
    import vtbstaticcase
    from cirs_hip.synthetic import write_virtualtaobao_log
    from core.user_data_taobao import load_dataset_mlp_taobao
    from core.user_model_mmoe import loss_taobao_mlp
    from core.user_model_train import train_mlp_taobao
    from evaluation import test_taobao
    log = str(tmp_path / "dataset.txt")
    base = vtbcase.base_vtb(golden_dir, 4, 2.4, 20)
    n_rows = write_virtualtaobao_log(log, 300, seed=1, vtb_env=base)
    ds, xc, yc = load_dataset_mlp_taobao(log)
    assert ds.x_numpy.shape == (n_rows, 91) and ds.y_numpy.shape == (n_rows, 28)
    assert (ds.x_numpy[:, 90] == 1).sum() == 300 and np.abs(ds.y_numpy[:, :27]).max() <= 1 and set(np.unique(ds.y_numpy[:, 27])) <= set(range(11))
    env = vtbcase.base_vtb(golden_dir, 4, 2.4, 20)
    env.set_state_mode(True)
    bs, epochs = 100, 3
    keys = {"ctr", "click_loss", "len_tra", "R_tra"}

    def fresh():
        m = vtbstaticcase.two_task_model((64, 32), stressed=True)
        m.compile(optimizer="adam", loss_func=loss_taobao_mlp, metrics=None)
        return m
    # with compile_RL_test: begin, ee(-1), (eb, ee) x epochs, end; the evaluation's keys in every epoch's logs
    model = fresh()
    init = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    model.compile_RL_test(functools.partial(test_taobao, env=env, epsilon=0, device="cuda", num_trajectory=20))
    cb = _CB()
    hist = model.fit_data(ds, batch_size=bs, epochs=epochs, shuffle=False, callbacks=[cb])
    assert [c[:2] for c in cb.calls] == [("begin",), ("ee", -1)] + [(t, e) for e in range(epochs) for t in ("eb", "ee")] + [("end",)]
    assert set(cb.calls[1][2]) == keys
    for h in hist:
        assert set(h) == keys | {"loss"} and np.isfinite(list(h.values())).all()
    ref = _torch_epochs(init, ds, bs, epochs)
    got = [h["loss"] for h in hist]
    print("fit_data losses per epoch", got, "torch restatement", ref)
    np.testing.assert_allclose(got, ref, rtol=1e-2)
    assert ref[-1] < ref[0] and got[-1] < got[0]
    trained = model._trainer.state_dict()
    assert set(trained) == set(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(v, trained[k].cpu().reshape(v.shape)), k
    # without it: today's sequence, the same losses (the evaluation does not touch the training)
    model_b = fresh()
    cb_b = _CB()
    hist_b = model_b.fit_data(ds, batch_size=bs, epochs=epochs, shuffle=False, callbacks=[cb_b])
    assert [c[:2] for c in cb_b.calls] == [("begin",)] + [(t, e) for e in range(epochs) for t in ("eb", "ee")] + [("end",)]
    assert [set(h) for h in hist_b] == [{"loss"}] * epochs and [h["loss"] for h in hist_b] == got
    # the run of MLP-taobao.py / MLP-epsilonGreedy-taobao.py end to end
    for eps in (0, 0.3):
        res = train_mlp_taobao(log, save_root=str(tmp_path), epsilon=eps, vtb_env=vtbcase.base_vtb(golden_dir, 4, 2.4, 20), dnn=(48, 40), epoch=2,
                               num_trajectory=20)
        assert len(res.history) == 2 and all(set(h) == keys | {"loss"} and np.isfinite(list(h.values())).all() for h in res.history)
        assert res.env.static


def test_unsupported_shapes_are_refused_through_the_abi():
    from cirs_hip import abi
    lib = abi.lib()

    def cfg(d_in=91, hidden=(64, 64), experts=4, expert_dim=8, n_tasks=2, task_dim=(27, 1)):
        hid = list(hidden)[:3] + [0] * (3 - min(3, len(hidden)))
        sh = abi.VtbMmoeShape(d_in=d_in, n_dnn=len(hidden), hidden=(C.c_int32 * 3)(*hid), experts=experts, expert_dim=expert_dim, n_tasks=n_tasks,
                              task_dim=(C.c_int32 * 2)(*task_dim))
        return abi.MlpTrainCfg(shape=sh, l2_linear=1e-5, l2_all=1e-2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    good = cfg()
    assert lib.cirs_mlp_train_param_count(C.byref(good)) == 91 * 64 + 64 * 64 + 40 * 64 + 64 + 64 + 32 + 28 * 8 + 28 + 91 + 91
    assert lib.cirs_mlp_train_workspace_bytes(C.byref(good), 100) > 0
    buf = torch.zeros(64, device="cuda")
    for bad in (cfg(d_in=118), cfg(hidden=()), cfg(hidden=(64, 64, 64, 64)), cfg(hidden=(257,)), cfg(hidden=(64, 0)), cfg(experts=9), cfg(expert_dim=0),
                cfg(n_tasks=1), cfg(task_dim=(1, 27))):
        assert lib.cirs_mlp_train_param_count(C.byref(bad)) == 0
        assert lib.cirs_mlp_train_workspace_bytes(C.byref(bad), 100) == 0
        rc = lib.cirs_mlp_train_step(C.byref(bad), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr(), 1,
                                     buf.data_ptr(), buf.data_ptr(), 256, None)
        assert rc == -3 and b"static baselines" in lib.cirs_last_error()
    with pytest.raises(ValueError, match="static baselines"):
        _trainer(mlpcase.stressed_init((300,)))
    tr = _trainer(mlpcase.stressed_init((8,), 2, 2))
    with pytest.raises(ValueError, match="28"):
        tr.step(torch.zeros(4, 91), torch.zeros(4, 1))
