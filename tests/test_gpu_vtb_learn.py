"""GPU: the VirtualTaobao PPO update on the device (csrc/vtb_learn.hip, cirs_hip/vtb_learn.py, core/vtb_learner.py) against the merged host
path on the same collect: the device collect's states rebuilt in torch with the collect's masks (DeviceVtbCollector.rebuild_states), the rows
added in HostCollector's order, and HostPPOPolicy.update with the same numpy seed."""
import copy

import numpy as np
import pytest
import torch

import vtbrolloutcase as case

pytestmark = pytest.mark.gpu

STATE_TOL = dict(rtol=1e-5, atol=1e-6)
BAR = dict(rtol=2e-3, atol=2e-5)
SCRIPT = dict(discount_factor=0.95, max_grad_norm=0.5, eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, reward_normalization=1,
              advantage_normalization=1, recompute_advantage=0, value_clip=1, gae_lambda=0.95)


def _setup(golden_dir, n, T, simulated=True, dropout=0.0, seed=2022, **hyper):
    from core.collector import Collector
    from core.policy.ppo import PPOPolicy
    from tianshou.data import VectorReplayBuffer
    from torch.distributions import Independent, Normal
    env, base = case.venv(golden_dir, n, simulated, T)
    tracker, actor, critic, _ = case.stack(base, n, T, dropout=dropout, seed=seed)
    kw = dict(SCRIPT, **hyper)
    dist = lambda *logits: Independent(Normal(*logits), 1)     # noqa: E731
    optim = [torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=1e-3), torch.optim.Adam(tracker.parameters(), lr=1e-3)]
    dev = PPOPolicy(actor, critic, optim, dist, action_space=base.action_space, learner="device", **kw)
    host = PPOPolicy(actor, critic, optim, dist, action_space=base.action_space, **kw)
    env.seed(7)
    c = Collector(dev, env, VectorReplayBuffer(n * T, n), preprocess_fn=tracker.build_state, rollout="device")
    return c, tracker, actor, critic, dev, host


def _reference_buffer(c, n, T):
    """DeviceVtbCollector's merged host fill: states rebuilt with autograd, rows added in HostCollector's order."""
    from tianshou.data import Batch, VectorReplayBuffer
    ro = c.rollout()
    tr = {k: ro.traj[k].cpu() for k in ("obs0", "obs", "rew", "done", "ctr", "act", "state")}
    lens = ro.traj["len"].cpu().numpy().astype(np.int64)
    states = c.rebuild_states(ro, tr, lens, c.last_collect[2])
    ref = VectorReplayBuffer(n * T, n)
    for t, ids, rew, done, info in c._transitions(tr, lens):
        tid = torch.as_tensor(ids)
        ref.add(Batch(obs=states[t, tid], act=tr["act"].numpy()[t, ids], rew=rew, done=done, obs_next=states[t + 1, tid], info=info,
                      policy=Batch()), buffer_ids=ids)
    return ref


def _snapshot(mods, optim):
    return [copy.deepcopy(m.state_dict()) for m in mods], [copy.deepcopy(o.state_dict()) for o in optim]


def _restore(mods, optim, snap):
    for m, s in zip(mods, snap[0]):
        m.load_state_dict(s)
    for o, s in zip(optim, snap[1]):
        o.load_state_dict(s)


def _run(policy, buf, batch_size, repeat, sample_size=0, seed=5):
    from core.host_rl import ReturnScale
    policy.ret_rms = ReturnScale()
    np.random.seed(seed)
    torch.manual_seed(seed)
    return policy.update(sample_size, buf, batch_size=batch_size, repeat=repeat)


def _params(mods):
    return [p.detach().clone() for m in mods for p in m.parameters()]


def _compare(mods, tracker, got_l, want_l, got_p, want_p, got_state, want_state, got_rms, want_rms):
    for k in want_l:
        assert len(got_l[k]) == len(want_l[k]), k
        np.testing.assert_allclose(got_l[k], want_l[k], **BAR, err_msg=k)
    names = [f"{i}.{k}" for i, m in enumerate(mods) for k, _ in m.named_parameters()]
    D = tracker.dim_model
    n_trk = len(list(tracker.parameters()))
    for j, (name, a, b) in enumerate(zip(names, got_p, want_p)):
        a, b = a.numpy().reshape(-1), b.numpy().reshape(-1)
        keep = np.ones(a.size, bool)
        if name.endswith("self_attn.in_proj_bias"):
            keep[D:2 * D] = False
        if j < n_trk:
            # the tracker takes ONE Adam step, lr * g / (|g| + eps): where the reference gradient is at round-off level (below 1e-4 of
            # the tensor's largest) both sides move by a round-off-driven fraction of lr.  Those elements are held to the first-moment
            # bar below instead; there may be at most 0.1% of them.
            g = np.abs(want_state[j][1]["exp_avg"].numpy().reshape(-1))
            tiny = g < 1e-4 * g.max()
            miss = ~np.isclose(a, b, **BAR) & keep
            assert not (miss & ~tiny).any() and miss.sum() <= max(1, a.size // 1000), name
            keep &= ~tiny
        np.testing.assert_allclose(a[keep], b[keep], **BAR, err_msg=name)
    for (ka, sa), (kb, sb) in zip(got_state, want_state):
        assert float(sa["step"]) == float(sb["step"])
        if ka.endswith("self_attn.in_proj_bias"):
            continue
        for key in ("exp_avg", "exp_avg_sq"):
            np.testing.assert_allclose(sa[key].numpy(), sb[key].numpy(), **BAR, err_msg=ka + key)
    assert got_rms[2] == want_rms[2]
    np.testing.assert_allclose(got_rms[:2], want_rms[:2], rtol=1e-4)


def _opt_states(mods, optim):
    out = []
    for i, m in enumerate(mods):
        opt = optim[1] if i == 0 else optim[0]
        for k, p in m.named_parameters():
            out.append((f"{i}.{k}", {key: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for key, v in opt.state[p].items()}))
    return out


def _device_vs_host(golden_dir, n, T, simulated, dropout, batch_size, repeat=2, sample_size=0, **hyper):
    c, tracker, actor, critic, dev, host = _setup(golden_dir, n, T, simulated, dropout, **hyper)
    res = c.collect(n_episode=n)
    mods = (tracker, actor, critic)
    snap = _snapshot(mods, dev.optim)
    p0 = _params(mods)
    assert len(c.buffer) == res["n/st"]
    got_l = _run(dev, c.buffer, batch_size, repeat, sample_size)
    got_p, got_s = _params(mods), _opt_states(mods, dev.optim)
    got_rms = (dev.ret_rms.mean, dev.ret_rms.var, dev.ret_rms.count)
    dev_buf = c.buffer
    _restore(mods, dev.optim, snap)
    ref = _reference_buffer(c, n, T)
    np.testing.assert_array_equal(dev_buf.sample_index(0), ref.sample_index(0))
    for key in ("act", "rew", "done"):
        np.testing.assert_array_equal(np.asarray(getattr(dev_buf, key)), np.asarray(getattr(ref, key)), err_msg=key)
    np.testing.assert_array_equal(dev_buf.info.CTR, ref.info.CTR)
    np.testing.assert_array_equal(dev_buf.info.env_id, ref.info.env_id)
    np.testing.assert_allclose(dev_buf.obs.numpy(), ref.obs.detach().numpy(), **STATE_TOL)
    want_l = _run(host, ref, batch_size, repeat, sample_size)
    want_p, want_s = _params(mods), _opt_states(mods, dev.optim)
    want_rms = (host.ret_rms.mean, host.ret_rms.var, host.ret_rms.count)
    if not hyper.get("reward_normalization", 1):
        got_rms = want_rms = (0.0, 1.0, 1.0)
    _compare(mods, tracker, got_l, want_l, got_p, want_p, got_s, want_s, np.asarray(got_rms), np.asarray(want_rms))
    n_trk = len(list(tracker.parameters()))
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(got_p[:n_trk], p0[:n_trk]))      # the gradient reached the tracker


@pytest.mark.parametrize("n,T,simulated,dropout,batch_size", [
    (16, 10, True, 0.0, 32),      # leaves a tail
    (16, 10, False, 0.1, 8),
    (16, 10, True, 0.1, 4096),    # larger than n
    (100, 50, True, 0.1, 2048),
    (100, 50, False, 0.0, 512),
])
def test_device_update_equals_host_update(golden_dir, n, T, simulated, dropout, batch_size):
    _device_vs_host(golden_dir, n, T, simulated, dropout, batch_size)


def test_batch_size_that_divides_n(golden_dir):
    c, tracker, actor, critic, dev, host = _setup(golden_dir, 16, 10, True, 0.0)
    c.collect(n_episode=16)
    n = len(c.buffer)
    divisors = [d for d in range(2, n) if n % d == 0 and n // d >= 2]
    if divisors:
        _device_vs_host(golden_dir, 16, 10, True, 0.0, divisors[-1])


@pytest.mark.parametrize("hyper", [
    dict(ent_coef=0.01, max_grad_norm=None, reward_normalization=0, value_clip=0, advantage_normalization=0),
    dict(dual_clip=2.0, recompute_advantage=1),
])
def test_hyper_parameter_cases(golden_dir, hyper):
    _device_vs_host(golden_dir, 16, 10, True, 0.1, 32, **hyper)


def test_sample_size_above_zero(golden_dir):
    _device_vs_host(golden_dir, 16, 10, True, 0.0, 32, sample_size=100)


def test_returns_stage_and_states(golden_dir):
    n, T = 16, 10
    c, tracker, actor, critic, dev, host = _setup(golden_dir, n, T, True, 0.1)
    c.collect(n_episode=n)
    from cirs_hip.vtb_learn import DeviceVtbLearner  # noqa: F401
    from core.host_rl import ReturnScale
    buf = c.buffer
    rows = buf.sample_index(0)
    dev.ret_rms = ReturnScale()
    ln = dev._get_learner(buf._traj)
    ln.prepare(dev, buf._traj, rows, buf)
    v_s, adv, ret, logp_old = (x.cpu().numpy() for x in ln.row_block())
    states = ln.states().cpu()
    ref = _reference_buffer(c, n, T)
    lens = buf._traj.lens
    env, t = rows // buf.size, rows % buf.size
    np.testing.assert_allclose(states[t, env].numpy(), ref.obs[rows].detach().numpy(), **STATE_TOL)
    np.testing.assert_allclose(states[t + 1, env].numpy(), ref.obs_next[rows].detach().numpy(), **STATE_TOL)
    host.ret_rms = ReturnScale()
    torch.manual_seed(0)
    with torch.no_grad():
        batch = host.process_fn(ref[rows], ref, rows)
    np.testing.assert_allclose(v_s, batch.v_s.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(adv, batch.adv.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ret, batch.returns.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(logp_old, batch.logp_old.numpy(), rtol=1e-5, atol=1e-4)
    assert lens.sum() == len(rows)


def test_two_device_updates_from_one_snapshot_are_bit_identical(golden_dir):
    c, tracker, actor, critic, dev, host = _setup(golden_dir, 16, 10, True, 0.1)
    c.collect(n_episode=16)
    mods = (tracker, actor, critic)
    snap = _snapshot(mods, dev.optim)
    l1 = _run(dev, c.buffer, 32, 2)
    p1 = _params(mods)
    _restore(mods, dev.optim, snap)
    l2 = _run(dev, c.buffer, 32, 2)
    p2 = _params(mods)
    assert l1 == l2
    for a, b in zip(p1, p2):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_checkpoint_reload_continues_bit_identically(golden_dir, tmp_path):
    """optim[i].state_dict() + the modules after one device update, reloaded over clobbered objects: the next collect + update equals
    continuing without the reload, bit for bit."""
    def run(reload):
        c, tracker, actor, critic, dev, host = _setup(golden_dir, 16, 10, True, 0.1)
        mods = (tracker, actor, critic)
        c.collect(n_episode=16)
        _run(dev, c.buffer, 32, 2)
        if reload:
            path = tmp_path / "ckpt.pt"
            torch.save({"mods": [m.state_dict() for m in mods], "optim": [o.state_dict() for o in dev.optim]}, path)
            with torch.no_grad():
                for m in mods:
                    for p in m.parameters():
                        p.add_(1.0)
            for o in dev.optim:
                o.state.clear()
            ck = torch.load(path, weights_only=False)
            for m, s in zip(mods, ck["mods"]):
                m.load_state_dict(s)
            for o, s in zip(dev.optim, ck["optim"]):
                o.load_state_dict(s)
        c.collect(n_episode=16)
        np.random.seed(9)
        losses = dev.update(0, c.buffer, batch_size=32, repeat=2)
        return losses, _params(mods), _opt_states(mods, dev.optim)

    la, pa, sa = run(False)
    lb, pb, sb = run(True)
    assert la == lb
    for a, b in zip(pa, pb):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    for (_, x), (_, y) in zip(sa, sb):
        assert float(x["step"]) == float(y["step"])
        torch.testing.assert_close(x["exp_avg_sq"], y["exp_avg_sq"], rtol=0, atol=0)


def test_buffer_from_the_host_collector_is_refused(golden_dir):
    from core.collector import Collector
    from tianshou.data import VectorReplayBuffer
    c, tracker, actor, critic, dev, host = _setup(golden_dir, 4, 3, True, 0.0)
    env, _ = case.venv(golden_dir, 4, True, 3, device=None)
    hc = Collector(host, env, VectorReplayBuffer(12, 4), preprocess_fn=tracker.build_state)
    hc.collect(n_episode=4)
    with pytest.raises(ValueError, match="device collect"):
        dev.update(0, hc.buffer, batch_size=8, repeat=1)


def _trainer_run(golden_dir, seed):
    from core.collector import Collector
    from core.trainer.onpolicy import onpolicy_trainer
    from tianshou.data import VectorReplayBuffer
    n, T = 100, 9
    train_env, base = case.venv(golden_dir, n, True, T)
    test_env, _ = case.venv(golden_dir, n, False, T)
    c, tracker, actor, critic, dev, host = _setup(golden_dir, n, T, True, 0.1)
    train_env.seed(seed)
    test_env.seed(seed + 1)
    torch.manual_seed(seed)
    np.random.seed(seed)
    train_c = Collector(dev, train_env, VectorReplayBuffer(n * T, n), preprocess_fn=tracker.build_state, rollout="device")
    test_c = Collector(dev, test_env, preprocess_fn=tracker.build_state, rollout="device")
    before = _params((tracker, actor))
    got = []
    orig = train_c.collect

    def spy(**kw):
        res = orig(**kw)
        got.append((res, len(train_c.buffer)))
        return res
    train_c.collect = spy
    onpolicy_trainer(dev, train_c, test_c, tracker, max_epoch=2, step_per_epoch=150, repeat_per_collect=2, episode_per_test=n,
                     batch_size=64, episode_per_collect=n, verbose=False)
    return got, before, _params((tracker, actor))


def test_onpolicy_trainer_two_epochs_device_learner(golden_dir):
    got, before, after = _trainer_run(golden_dir, 11)
    assert len(got) >= 2
    for res, rows in got:
        assert rows == res["n/st"]
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(after, before))
    assert all(torch.isfinite(a).all() for a in after)
    _, _, after2 = _trainer_run(golden_dir, 11)
    for a, b in zip(after, after2):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
