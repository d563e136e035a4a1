"""GPU: the VirtualTaobao PPO rollout on the device (csrc/vtb_rollout.hip, cirs_hip/vtb_rollout.py, core/vtb_collector.py) against the
host procedures it replaces: HostStateTracker.build_state step by step (states), the host ActorProb with the device's own Gaussian draws
(actions), DeviceVirtualTB.step fed the recorded actions (env), the functional rebuild with the exported masks (dropout), and
HostPPOPolicy.update on a buffer built from the build_state replay (gradient path)."""
import numpy as np
import pytest
import torch

import vtbrolloutcase as case

pytestmark = pytest.mark.gpu

STATE_TOL = dict(rtol=1e-5, atol=1e-6)


def _collector(golden_dir, n, T, simulated=True, version="v1", dropout=0.0, buffer=True, force_length=0, env_seed=7, seed=2022):
    from core.collector import Collector
    from tianshou.data import VectorReplayBuffer
    env, base = case.venv(golden_dir, n, simulated, T, version=version)
    tracker, actor, critic, policy = case.stack(base, n, T, dropout=dropout, seed=seed)
    env.seed(env_seed)
    buf = VectorReplayBuffer(n * T, n) if buffer else None
    c = Collector(policy, env, buf, preprocess_fn=tracker.build_state, rollout="device", force_length=force_length)
    return c, env, tracker, actor, critic, policy


def _host_traj(c):
    ro = c.rollout()
    return {k: v.cpu() for k, v in ro.traj.items()}


CASES = [(1, 50, "v1"), (4, 3, "raw"), (4, 50, "v2"), (100, 50, "raw"), (100, 3, "v1"), (1024, 50, "v1"), (1024, 3, "raw"), (4, 1, "v1")]


@pytest.mark.parametrize("n,T,kind", CASES)
def test_states_and_actions_match_the_host_procedures(golden_dir, n, T, kind):
    c, env, tracker, actor, _, policy = _collector(golden_dir, n, T, simulated=kind != "raw", version="v2" if kind == "v2" else "v1",
                                                   buffer=False)
    res = c.collect(n_episode=n)
    tr = _host_traj(c)
    lens = tr["len"].numpy().astype(int)
    assert res["n/ep"] == n and res["n/st"] == lens.sum() and (lens >= 1).all() and (lens <= T).all()
    if T == 1:
        assert (lens == 1).all()      # every episode ends at turn 0
    # states: HostStateTracker.build_state, step by step over the recorded inputs
    steps = case.replay_states(tracker, tr["obs0"].numpy(), tr["obs"].numpy(), tr["rew"].numpy(), lens)
    for t, (ids, s) in enumerate(steps):
        np.testing.assert_allclose(tr["state"][t, ids].numpy(), s.numpy(), **STATE_TOL, err_msg=f"state t={t}")
    # actor: the host ActorProb on the device states, with the device's z
    seed, cid, _ = c.last_collect
    rows = [(t, e) for t in range(int(lens.max())) for e in np.flatnonzero(lens > t)]
    ts, es = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    z = c.rollout().noise(seed, cid, es, ts).cpu()
    with torch.no_grad():
        (mu, sigma), _ = actor(tr["state"][ts, es])
    act = tr["act"][ts, es]
    np.testing.assert_allclose(act.numpy(), (mu + sigma * z).numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(tr["act_mapped"][ts, es].numpy(), policy.map_action(act.numpy()))
    np.testing.assert_array_equal(tr["obs"][ts, es, :27].numpy(), tr["act_mapped"][ts, es].numpy().astype(np.float64))


def test_force_length_ends_every_episode_there(golden_dir):
    c, *_ = _collector(golden_dir, 8, 10, buffer=False, force_length=1)
    res = c.collect(n_episode=8)
    assert (res["lens"] == 1).all() and res["n/st"] == 8
    c2, *_ = _collector(golden_dir, 8, 10, buffer=False, force_length=6)
    res = c2.collect(n_episode=8)
    assert (res["lens"] == 6).all()


def test_noise_is_gaussian_and_restated_bit_for_bit(golden_dir):
    from cirs_hip import abi
    from cirs_hip.vtb_host import gauss_noise
    n, T = 2000, 25
    ids = torch.as_tensor(np.repeat(np.arange(n), T).astype(np.int32), device="cuda")
    ts = torch.as_tensor(np.tile(np.arange(T), n).astype(np.int32), device="cuda")
    out = torch.empty((n * T, 27), dtype=torch.float32, device="cuda")
    abi.check(abi.lib().cirs_vtb_rollout_noise(123456789, 3, ids.data_ptr(), ts.data_ptr(), n * T, 27, out.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "noise")
    z = out.cpu().numpy()
    m = z.astype(np.float64)
    assert abs(m.mean()) < 5 / np.sqrt(m.size) and abs(m.var() - 1) < 5 * np.sqrt(2 / m.size)
    assert abs(np.mean(m > 1.0) - 0.158655) < 5 * np.sqrt(0.158655 * 0.841345 / m.size)
    host = gauss_noise(123456789, 3, np.repeat(np.arange(300), T), np.tile(np.arange(T), 300))
    np.testing.assert_array_equal(z[:300 * T], host)


@pytest.mark.parametrize("simulated", [True, False])
def test_env_replay_reproduces_the_recorded_steps(golden_dir, simulated):
    n, T = 64, 20
    c, env, *_ = _collector(golden_dir, n, T, simulated=simulated, buffer=False)
    vtb = env.vtb_env()
    ev0 = vtb.event.clone()
    c.collect(n_episode=n)
    tr = _host_traj(c)
    lens = tr["len"].numpy().astype(int)
    vtb.event.copy_(ev0)
    np.testing.assert_array_equal(vtb.reset().cpu().numpy(), tr["obs0"].numpy())
    for t in range(int(lens.max())):
        ids = np.flatnonzero(lens > t)
        obs, rew, done, ctr = vtb.step(tr["act_mapped"][t, ids].cuda(), ids)
        np.testing.assert_array_equal(obs.cpu().numpy(), tr["obs"][t, ids].numpy())
        np.testing.assert_array_equal(rew.cpu().numpy(), tr["rew"][t, ids].numpy())
        np.testing.assert_array_equal(done.cpu().numpy(), tr["done"][t, ids].numpy())
        np.testing.assert_array_equal(ctr.cpu().numpy(), tr["ctr"][t, ids].numpy())


def test_dropout_rebuild_masks_and_rates(golden_dir):
    from cirs_hip import vtb_host
    n, T, p = 100, 50, 0.1
    c, env, tracker, *_ = _collector(golden_dir, n, T, dropout=p, buffer=False)
    c.collect(n_episode=n)
    tr = _host_traj(c)
    lens = tr["len"].numpy().astype(int)
    ro = c.rollout()
    _, _, dseed = c.last_collect
    Tm = int(lens.max())
    masks = ro.masks(dseed, Tm + 1)
    with torch.no_grad():
        st = vtb_host.tracker_states(tracker, tr["obs0"][:, :-3].float(), tr["rew"][:Tm].float(), tr["obs"][:Tm, :, :-3].float(), masks)
        plain = vtb_host.tracker_states(tracker, tr["obs0"][:, :-3].float(), tr["rew"][:Tm].float(), tr["obs"][:Tm, :, :-3].float())
    live = [(t, np.flatnonzero(lens >= t)) for t in range(Tm + 1)]
    for t, ids in live:
        np.testing.assert_allclose(tr["state"][t, ids].numpy(), st[t, ids].numpy(), rtol=1e-5, atol=1e-5, err_msg=f"t={t}")
    assert max(float((tr["state"][t, ids] - plain[t, ids]).abs().max()) for t, ids in live) > 1e-3     # the masks did act
    inv = np.float32(1) / (np.float32(1) - np.float32(p))
    for key, m in masks.items():
        v = m.numpy()
        assert set(np.unique(v)) <= {0.0, inv}, key
        k = v.size
        assert abs((v == 0).mean() - p) < 5 * np.sqrt(p * (1 - p) / k), key
    # position-keyed: the masks of a position do not depend on the range they are requested with (a later vector step sees the same ones)
    later = ro.masks(dseed, Tm + 1)
    for key in masks:
        torch.testing.assert_close(masks[key], later[key], rtol=0, atol=0)
    from cirs_hip import abi
    full = ro.masks(dseed, 12)
    part = torch.empty((n, 5, 27), dtype=torch.float32, device="cuda")
    abi.check(abi.lib().cirs_vtb_rollout_masks(dseed, p, 0, n, 7, 5, 0, 0, 27, part.data_ptr(), torch.cuda.current_stream().cuda_stream), "m")
    torch.testing.assert_close(part.cpu(), full["pos"][:, 7:12], rtol=0, atol=0)
    torch.testing.assert_close(full["pos"][:, :min(12, Tm + 1)], masks["pos"][:, :min(12, Tm + 1)], rtol=0, atol=0)


def test_update_from_the_device_buffer_equals_the_build_state_replay(golden_dir):
    import copy
    from core.host_rl import ReturnScale
    from tianshou.data import Batch, VectorReplayBuffer
    n, T = 16, 10
    c, env, tracker, actor, critic, policy = _collector(golden_dir, n, T, dropout=0.0)
    c.collect(n_episode=n)
    tr = _host_traj(c)
    lens = tr["len"].numpy().astype(int)
    mods = (tracker, actor, critic)
    snap = [copy.deepcopy(m.state_dict()) for m in mods]
    opt_snap = [copy.deepcopy(o.state_dict()) for o in policy.optim]
    p0 = [p.detach().clone() for m in mods for p in m.parameters()]

    def reference_buffer():
        """build_state with grad, rows added in HostCollector's order"""
        steps = case.replay_states(tracker, tr["obs0"].numpy(), tr["obs"].numpy(), tr["rew"].numpy(), lens, grad=True)
        ref = VectorReplayBuffer(n * T, n)
        for t in range(int(lens.max())):
            ids = np.flatnonzero(lens > t)
            prev_ids, prev = steps[t]
            pos = np.searchsorted(prev_ids, ids)
            ref.add(Batch(obs=prev[torch.as_tensor(pos)], act=tr["act"][t, ids].numpy(), rew=tr["rew"][t, ids].numpy(),
                          done=tr["done"][t, ids].numpy().astype(bool), obs_next=steps[t + 1][1],
                          info=Batch(CTR=tr["ctr"][t, ids].numpy(), env_id=ids), policy=Batch()), buffer_ids=ids)
        return ref

    def update(b):
        policy.ret_rms = ReturnScale()
        torch.manual_seed(5)
        np.random.seed(5)
        losses = policy.update(0, b, batch_size=32, repeat=2)
        return losses, [p.detach().clone() for m in mods for p in m.parameters()]

    buf = c.buffer
    assert len(buf) == lens.sum()
    got_l, got_p = update(buf)              # (the device buffer's graph was recorded at the snapshot's parameters)
    for m, s in zip(mods, snap):
        m.load_state_dict(s)
    for o, s in zip(policy.optim, opt_snap):
        o.load_state_dict(s)
    ref = reference_buffer()
    np.testing.assert_array_equal(buf.sample_index(0), ref.sample_index(0))
    np.testing.assert_allclose(buf.obs.detach().numpy(), ref.obs.detach().numpy(), **STATE_TOL)
    np.testing.assert_allclose(buf.obs_next.detach().numpy(), ref.obs_next.detach().numpy(), **STATE_TOL)
    want_l, want_p = update(ref)
    for k in want_l:
        np.testing.assert_allclose(got_l[k], want_l[k], rtol=2e-3, atol=2e-5, err_msg=k)
    # the key part of each in_proj bias has an exactly zero gradient (softmax is shift-invariant), so both gradients there are round-off
    # that Adam scales to +-lr steps: those 27 elements per layer are left out
    names = [f"{i}.{k}" for i, m in enumerate(mods) for k, _ in m.named_parameters()]
    D = tracker.dim_model
    for name, a, b in zip(names, got_p, want_p):
        a, b = a.numpy(), b.numpy()
        if name.endswith("self_attn.in_proj_bias"):
            a, b = np.r_[a[:D], a[2 * D:]], np.r_[b[:D], b[2 * D:]]
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-5, err_msg=name)
    n_trk = len(list(tracker.parameters()))
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(got_p[:n_trk], p0[:n_trk]))      # the gradient reached the tracker


def _plugin_run(golden_dir, seed):
    from core.collector import Collector
    from core.trainer.onpolicy import onpolicy_trainer
    from tianshou.data import VectorReplayBuffer
    n, T = 100, 9
    train_env, base = case.venv(golden_dir, n, True, T)
    test_env, _ = case.venv(golden_dir, n, False, T)
    tracker, actor, critic, policy = case.stack(base, n, T, dropout=0.1, seed=2022)
    train_env.seed(seed)
    test_env.seed(seed + 1)
    torch.manual_seed(seed)
    np.random.seed(seed)
    train_c = Collector(policy, train_env, VectorReplayBuffer(n * T, n), preprocess_fn=tracker.build_state, rollout="device")
    test_c = Collector(policy, test_env, preprocess_fn=tracker.build_state, rollout="device")
    before = [p.detach().clone() for m in (tracker, actor) for p in m.parameters()]
    got = []
    orig = train_c.collect

    def spy(**kw):
        res = orig(**kw)
        got.append((res, len(train_c.buffer), res["lens"].sum()))
        return res
    train_c.collect = spy
    info = onpolicy_trainer(policy, train_c, test_c, tracker, max_epoch=2, step_per_epoch=150, repeat_per_collect=2, episode_per_test=n,
                            batch_size=64, episode_per_collect=n, verbose=False)
    after = [p.detach().clone() for m in (tracker, actor) for p in m.parameters()]
    return got, info, before, after


def test_plugin_onpolicy_trainer_two_epochs(golden_dir):
    got, info, before, after = _plugin_run(golden_dir, 11)
    keys = {"rews", "lens", "idxs", "n/st", "n/ep", "rew", "rew_std", "len", "len_std"}
    assert len(got) >= 2
    for res, rows, total in got:
        assert set(res) == keys
        assert rows == total == res["n/st"]
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(after, before))
    assert all(torch.isfinite(a).all() for a in after)
    got2, info2, _, after2 = _plugin_run(golden_dir, 11)
    for a, b in zip(after, after2):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    for (r1, _, _), (r2, _, _) in zip(got, got2):
        np.testing.assert_array_equal(r1["rews"], r2["rews"])
        np.testing.assert_array_equal(r1["lens"], r2["lens"])
