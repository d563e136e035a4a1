"""GPU: training of the VirtualTaobao MMoE user model on the device (csrc/mmoe_train.hip) -- cirs_mmoe_train_step against the
reference's own fit_data recordings and, at scale, against the plain-torch restatement; bit-reproducibility and epoch == step loop;
cirs_vtb_exposure_history against the recorded reference values; the fit_data / train_user_model_taobao surface end to end."""
import pickle

import numpy as np
import pytest
import torch

import mmoecase
import traincase
from cirs_hip import mmoe_host

pytestmark = pytest.mark.gpu


def _trainer(init, **kw):
    from cirs_hip.mmoe_train import MMoETrainer
    return MMoETrainer(init, l2_linear=mmoecase.L2_LINEAR, l2_all=mmoecase.L2_ALL, **kw)


def _steps(init, x, y, score, n, steps, keep=(0,), order=None):
    tr = _trainer(init)
    losses, kept = [], {}
    order = np.arange(len(x)) if order is None else order
    for st in range(steps):
        idx = order[st * n:(st + 1) * n]
        lo = tr.step(x[idx], y[idx], score[idx])
        losses.append(lo.cpu().numpy().copy())
        if st in keep:
            kept[st] = {k: v.cpu().numpy() for k, v in tr.state_dict().items()}
    return np.array(losses), kept, {k: v.cpu().numpy() for k, v in tr.state_dict().items()}, tr


def _tight_share(got, want):
    return min(float((np.abs(np.asarray(got[k], np.float64).reshape(w.shape) - w) <= 2e-6 + 2e-5 * np.abs(w)).mean()) for k, w in want.items())


def test_train_step_matches_reference_fit_data(golden_dir):
    for ci, c in enumerate(mmoecase.load(golden_dir)[0]):
        losses, kept, final, _ = _steps(c["init"], c["x"], c["y"], c["score"], c["n"], c["steps"])
        print(f"case {ci}: losses {losses.tolist()} recorded {c['losses'].tolist()}; tight share first {_tight_share(kept[0], c['first']):.4f} "
              f"final {_tight_share(final, c['final']):.4f}")
        np.testing.assert_allclose(losses, c["losses"], rtol=3e-5, err_msg=f"case {ci}")
        traincase.compare_params(kept[0], c["first"], c["init"], f"case {ci} first step")
        traincase.compare_params(final, c["final"], c["init"], f"case {ci} final")
        assert set(final) == set(c["final"])


@pytest.mark.parametrize("batch", [2048, 100])
def test_train_step_vs_torch_at_scale(batch):
    N, steps = 8192, 8
    init = mmoecase.stressed_init((128, 128))
    x, y, score = mmoecase.inputs(N)
    order = np.tile(np.arange(N), 2)                  # 8 steps of 2048 rows are two passes over the data
    want_l, want_kept, want_final = mmoe_host.torch_train(init, x, y, score, batch, steps=steps, order=order, l2_linear=mmoecase.L2_LINEAR,
                                                          l2_all=mmoecase.L2_ALL, keep=(0,))
    assert want_l.shape == (steps, 2)
    got_l, got_kept, got_final, _ = _steps(init, x, y, score, batch, steps, order=order)
    print(f"batch {batch}: losses {got_l.tolist()} torch {want_l.tolist()}; tight share first {_tight_share(got_kept[0], want_kept[0]):.4f} "
          f"final {_tight_share(got_final, want_final):.4f}")
    np.testing.assert_allclose(got_l, want_l, rtol=3e-5)
    traincase.compare_params(got_kept[0], want_kept[0], init, f"batch {batch} first step")
    traincase.compare_params(got_final, want_final, init, f"batch {batch} final")


def _snapshot(tr):
    return [t.clone() for t in (tr.flat, tr.adam_m, tr.adam_v, tr.grads)]


def test_bit_reproducible_and_epoch_equals_step_loop():
    N, bs = 1000, 96                                  # 11 steps, the last one of 40 rows
    init = mmoecase.stressed_init((64, 128))
    x, y, score = (torch.as_tensor(a, dtype=torch.float32).cuda() for a in mmoecase.inputs(N, seed=5))
    order = torch.randperm(N, generator=torch.Generator().manual_seed(0)).cuda()
    runs = []
    for _ in range(2):                                # two step-by-step runs from one snapshot
        tr = _trainer(init)
        losses = []
        for s0 in range(0, N, bs):
            idx = order[s0:s0 + bs]
            losses.append(tr.step(x[idx], y[idx].reshape(-1), score[idx].reshape(-1)).clone())
        runs.append((_snapshot(tr), torch.stack(losses), tr.step_count))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1])
    tr = _trainer(init)
    ep_losses = tr.epoch(x, y, score, order, bs)
    assert ep_losses.shape == (11, 2) and tr.step_count == runs[0][2] == 11
    for a, b in zip(_snapshot(tr), runs[0][0]):
        assert torch.equal(a, b)
    assert torch.equal(ep_losses, runs[0][1])
    assert float((tr.flat - _trainer(init).flat).abs().min()) > 0       # every parameter moved (the regulariser reaches all of them)
    # a second epoch continues the optimiser state: equal to 11 more single steps
    ep2 = tr.epoch(x, y, score, order.flip(0), bs)
    tr_b = _trainer(init)
    tr_b.epoch(x, y, score, order, bs)
    for s0 in range(0, N, bs):
        idx = order.flip(0)[s0:s0 + bs]
        last = tr_b.step(x[idx], y[idx].reshape(-1), score[idx].reshape(-1))
    assert torch.equal(tr.flat, tr_b.flat) and torch.equal(ep2[-1], last)


def test_exposure_history(golden_dir):
    from cirs_hip.mmoe_train import vtb_exposure_history
    from cirs_hip import abi
    _, e = mmoecase.load(golden_dir)
    for tau, want in zip(e["taus"], e["out"]):
        got = vtb_exposure_history(e["timestamp"], e["action"], float(tau)).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    rng = np.random.RandomState(3)                    # 50 k rows, sessions of 1..120 rows
    lens = []
    while sum(lens) < 50000:
        lens.append(int(rng.randint(1, 121)))
    ts = np.concatenate([np.arange(1, L + 1) for L in lens])[:50000]
    act = rng.uniform(-1, 1, (50000, 27))
    for tau in (0.01, 2.0):
        got = vtb_exposure_history(ts, act, tau).cpu().numpy()
        np.testing.assert_allclose(got, mmoe_host.exposure_virtualtaobao(ts, act, tau), rtol=1e-12, atol=0)
    with pytest.raises(abi.CirsHipError, match="open a session"):
        vtb_exposure_history(ts[1:], act[1:], 1.0)


def test_fit_data_surface_and_artefacts(golden_dir, tmp_path):
    import vtbcase
    from cirs_hip.synthetic import write_virtualtaobao_log
    from cirs_hip.virtualtb import DeviceVirtualTB
    from core.collector import Collector
    from core.env.simulatedEnv.simulated_env import SimulatedEnv
    from core.user_data_taobao import load_dataset_virtualTaobao
    from core.user_model_mmoe import UserModel_MMOE, loss_taobao
    from core.user_model_train import train_user_model_taobao
    from tianshou.env import DummyVectorEnv
    import vtbrolloutcase as rcase
    log = str(tmp_path / "dataset.txt")
    base = vtbcase.base_vtb(golden_dir, 4, 2.4, 20)
    n_rows = write_virtualtaobao_log(log, 300, seed=1, vtb_env=base)
    ds, xc, yc = load_dataset_virtualTaobao(0.01, log)
    ts = ds.x_numpy[:, 90]
    assert len(ds) == n_rows and ts[0] == 1 and (ts == 1).sum() == 300 and ts.max() <= 20 and ds.x_numpy[:, :88].sum(1).max() == 11
    assert np.abs(ds.x_numpy[:, 91:]).max() <= 1 and set(np.unique(ds.y_numpy)) <= set(range(11))
    np.testing.assert_allclose(ds.score, mmoe_host.exposure_virtualtaobao(ts, ds.x_numpy[:, 91:], 0.01), rtol=1e-12)
    # fit_data against the torch restatement, 3 epochs without shuffling
    bs, epochs = 100, 3
    model = mmoecase.model((128, 128))
    model.load_state_dict({k: torch.as_tensor(v) for k, v in mmoecase.stressed_init((128, 128)).items()})
    init = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    model.compile(optimizer="adam", loss_func=loss_taobao, metrics=None)
    calls = []

    class CB:
        def on_train_begin(self): calls.append("begin")
        def on_train_end(self): calls.append("end")
        def on_epoch_begin(self, epoch): calls.append(("eb", epoch))
        def on_epoch_end(self, epoch, logs): calls.append(("ee", epoch, logs["loss"]))
    hist = model.fit_data(ds, batch_size=bs, epochs=epochs, shuffle=False, callbacks=[CB()])
    ref = _torch_epochs(init, ds, bs, epochs)
    got = [h["loss"] for h in hist]
    print("fit_data losses per epoch", got, "torch restatement", ref)
    assert calls[0] == "begin" and calls[-1] == "end" and [c[0] for c in calls[1:-1]] == ["eb", "ee"] * epochs
    np.testing.assert_allclose(got, ref, rtol=1e-2)
    assert ref[-1] < ref[0]
    # forward of the module after fit_data == the env kernel's forward on the trained weights
    x = torch.as_tensor(ds.x_numpy[:512], dtype=torch.float32)
    env = DeviceVirtualTB(base, 4, user_model=model)
    np.testing.assert_allclose(model(x).detach().numpy()[:, 0], env.mmoe_forward(x).cpu().numpy(), rtol=1e-5, atol=1e-4)
    trained = model._trainer.state_dict()
    for k, v in model.state_dict().items():
        assert torch.equal(v, trained[k].cpu()), k
    # the training run and its artefacts through the lines of CIRS-RL-taobao.py:134-142
    res = train_user_model_taobao(log, save_root=str(tmp_path), dnn=(128, 128), epoch=2, batch_size=100, message="T")
    assert len(res.history) == 2 and np.isfinite([h["loss"] for h in res.history]).all()
    with open(res.paths.params, "rb") as fh:
        model_params = pickle.load(fh)
    model_params["device"] = "cpu"
    user_model = UserModel_MMOE(**model_params)
    user_model.load_state_dict(torch.load(res.paths.state_dict))
    assert all(torch.equal(a, b) for a, b in zip(user_model.state_dict().values(), res.model.state_dict().values()))
    n_env, T = 8, 20

    def sim():
        env = vtbcase.base_vtb(golden_dir, 4, 2.4, T)
        s = SimulatedEnv.__new__(SimulatedEnv)
        s.__dict__.update(dict(user_model=user_model, env_task=env, observation_space=env.observation_space, action_space=env.action_space,
                               env_name="VirtualTB-v0", version="v1", tau=10.0, use_exposure_intervention=True, alpha_u=None, beta_i=None,
                               normed_mat=None, gamma_exposure=3.0, r_decay=1, cum_reward=0, total_turn=0))
        s._reset_history()
        return s
    one = sim()
    venv = DummyVectorEnv([lambda: one for _ in range(n_env)], device="cuda")
    tracker, actor, critic, policy = rcase.stack(one.env_task, n_env, T)
    venv.seed(3)
    c = Collector(policy, venv, None, preprocess_fn=tracker.build_state, rollout="device")
    out = c.collect(n_episode=n_env)
    assert out["n/ep"] == n_env and np.isfinite(out["rews"]).all() and np.isfinite(out["rew"])


def _torch_epochs(init, ds, bs, epochs):
    n = len(ds)
    # an epoch ends on its own short batch: run epoch by epoch, carrying parameters AND the Adam state
    import torch as T
    p = {k: T.nn.Parameter(T.as_tensor(v).clone()) for k, v in init.items()}
    opt = T.optim.Adam(list(p.values()), lr=1e-3)
    X, Y, E = (T.as_tensor(a, dtype=T.float32) for a in (ds.x_numpy, ds.y_numpy.reshape(-1, 1), np.asarray(ds.score).reshape(-1, 1)))
    out = []
    for _ in range(epochs):
        total = 0.0
        for s0 in range(0, n, bs):
            sl = slice(s0, s0 + bs)
            loss = mmoe_host.loss_taobao(mmoe_host.forward(p, X[sl]), Y[sl], E[sl])
            reg = mmoecase.L2_LINEAR * (p["linear_model.weight"] ** 2).sum() + sum(mmoecase.L2_ALL * (v ** 2).sum() for v in p.values())
            opt.zero_grad()
            (loss + reg).backward()
            opt.step()
            total += float(loss.detach()) + float(reg.detach())
        out.append(total / n)
    return out
