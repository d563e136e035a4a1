"""GPU: the exact-redraw tracker dropout of the device VirtualTaobao path (Collector(..., rollout="device", dropout_redraw=True);
cirs_vtb_rollout_collect_redraw, cirs_vtb_learn_*_redraw).  The oracle is the torch restatement vtb_host.redraw_states -- one causal pass
per call with that call's masks, every call's graph kept -- fed the device's own recorded inputs and exported masks; the learner is held
against HostPPOPolicy.update on a buffer whose obs carry those graphs, at the bars of tests/test_gpu_vtb_learn.py."""
import numpy as np
import pytest
import torch

import vtbrolloutcase as case
from test_gpu_vtb_learn import BAR, SCRIPT, _compare, _opt_states, _params, _reference_buffer, _restore, _run, _snapshot
from test_gpu_vtb_rollout import CASES

pytestmark = pytest.mark.gpu

TRAJ_KEYS = ("state", "act", "act_mapped", "obs", "rew", "done", "ctr", "len")


def _collector(golden_dir, n, T, kind="v1", dropout=0.0, redraw=True, buffer=False, learner=None, **hyper):
    """The script's stack over a device vector env; the same arguments give the same weights, env seed and collect keys."""
    from core.collector import Collector
    from core.policy.ppo import PPOPolicy
    from tianshou.data import VectorReplayBuffer
    from torch.distributions import Independent, Normal
    env, base = case.venv(golden_dir, n, kind != "raw", T, version="v2" if kind == "v2" else "v1")
    tracker, actor, critic, policy = case.stack(base, n, T, dropout=dropout)
    host = policy
    if learner is not None or hyper:
        dist = lambda *logits: Independent(Normal(*logits), 1)     # noqa: E731
        kw = dict(SCRIPT, **hyper)
        host = PPOPolicy(actor, critic, policy.optim, dist, action_space=base.action_space, **kw)
        if learner is not None:
            policy = PPOPolicy(actor, critic, policy.optim, dist, action_space=base.action_space, learner=learner, **kw)
    env.seed(7)
    torch.manual_seed(99)      # the collector's key
    c = Collector(policy, env, VectorReplayBuffer(n * T, n) if buffer else None, preprocess_fn=tracker.build_state, rollout="device",
                  dropout_redraw=redraw)
    return c, tracker, actor, critic, policy, host


def _traj(c):
    return {k: v.cpu() for k, v in c.rollout().traj.items()}


@pytest.mark.parametrize("n,T,kind", CASES)
def test_without_dropout_the_collect_is_the_ordinary_one(golden_dir, n, T, kind):
    got_c, *_ = _collector(golden_dir, n, T, kind, redraw=True)
    want_c, *_ = _collector(golden_dir, n, T, kind, redraw=False)
    got_c.collect(n_episode=n)
    want_c.collect(n_episode=n)
    assert got_c.last_collect == want_c.last_collect
    got, want = _traj(got_c), _traj(want_c)
    for k in TRAJ_KEYS:
        torch.testing.assert_close(got[k], want[k], rtol=0, atol=0, msg=k)


@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("n,T,kind", CASES)
def test_states_and_actions_match_the_per_call_restatement(golden_dir, n, T, kind, p):
    from cirs_hip import vtb_host
    c, tracker, actor, _, policy, _ = _collector(golden_dir, n, T, kind, dropout=p)
    keyed, *_ = _collector(golden_dir, n, T, kind, dropout=p, redraw=False)
    res = c.collect(n_episode=n)
    keyed.collect(n_episode=n)
    assert c.last_collect == keyed.last_collect
    ro = c.rollout()
    assert ro.dropout_redraw and not keyed.rollout().dropout_redraw
    tr, ktr = _traj(c), _traj(keyed)
    lens = tr["len"].numpy().astype(int)
    assert res["n/ep"] == n and res["n/st"] == lens.sum() and (lens >= 1).all() and (lens <= T).all()
    seed, cid, dseed = c.last_collect
    Tm = int(lens.max())
    with torch.no_grad():
        want = vtb_host.redraw_states(tracker, tr["obs0"][:, :-3].float(), tr["rew"][:Tm].float(), tr["obs"][:Tm, :, :-3].float(),
                                      lambda call: ro.masks(dseed, call + 1, env0=call * n))
    for call in range(Tm + 1):
        ids = np.flatnonzero(lens >= call)
        np.testing.assert_allclose(tr["state"][call, ids].numpy(), want[call, ids].numpy(), rtol=1e-5, atol=1e-5, err_msg=f"call {call}")
    # call 0 has the position-keyed key; from call 1 on the masks are the call's own
    torch.testing.assert_close(tr["state"][0], ktr["state"][0], rtol=0, atol=0)
    torch.testing.assert_close(tr["act"][0], ktr["act"][0], rtol=0, atol=0)
    for call in range(1, Tm + 1):
        ids = np.flatnonzero((lens >= call) & (ktr["len"].numpy() >= call))
        if len(ids):
            assert not torch.equal(tr["state"][call, ids], ktr["state"][call, ids]), f"call {call}"
    # actor: the host ActorProb on the redraw states, with the device's z
    rows = [(t, e) for t in range(Tm) for e in np.flatnonzero(lens > t)]
    ts, es = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    z = ro.noise(seed, cid, es, ts).cpu()
    with torch.no_grad():
        (mu, sigma), _ = actor(tr["state"][ts, es])
    act = tr["act"][ts, es]
    np.testing.assert_allclose(act.numpy(), (mu + sigma * z).numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(tr["act_mapped"][ts, es].numpy(), policy.map_action(act.numpy()))
    np.testing.assert_array_equal(tr["obs"][ts, es, :27].numpy(), tr["act_mapped"][ts, es].numpy().astype(np.float64))


def _update_vs_host(golden_dir, n, T, kind, dropout, batch_size, repeat=2):
    """-> (device parameters after the redraw update, the collector and its pieces, the snapshot before it)."""
    c, tracker, actor, critic, dev, host = _collector(golden_dir, n, T, kind, dropout=dropout, buffer=True, learner="device")
    res = c.collect(n_episode=n)
    mods = (tracker, actor, critic)
    snap = _snapshot(mods, dev.optim)
    p0 = _params(mods)
    assert len(c.buffer) == res["n/st"] and c.buffer._traj.dropout_redraw
    got_l = _run(dev, c.buffer, batch_size, repeat)
    got_p, got_s = _params(mods), _opt_states(mods, dev.optim)
    got_rms = (dev.ret_rms.mean, dev.ret_rms.var, dev.ret_rms.count)
    _restore(mods, dev.optim, snap)
    ref = _reference_buffer(c, n, T)                       # rebuild_states: redraw_states with the collect's masks, graphs kept
    np.testing.assert_array_equal(c.buffer.sample_index(0), ref.sample_index(0))
    np.testing.assert_allclose(c.buffer.obs.numpy(), ref.obs.detach().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(c.buffer.obs_next.numpy(), ref.obs_next.detach().numpy(), rtol=1e-5, atol=1e-5)
    want_l = _run(host, ref, batch_size, repeat)
    want_p, want_s = _params(mods), _opt_states(mods, dev.optim)
    want_rms = (host.ret_rms.mean, host.ret_rms.var, host.ret_rms.count)
    _compare(mods, tracker, got_l, want_l, got_p, want_p, got_s, want_s, np.asarray(got_rms), np.asarray(want_rms))
    n_trk = len(list(tracker.parameters()))
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(got_p[:n_trk], p0[:n_trk]))      # the gradient reached the tracker
    _restore(mods, dev.optim, snap)
    return got_p, (c, tracker, actor, critic, dev), snap


@pytest.mark.parametrize("n,T,kind,dropout,batch_size", [
    (16, 10, "v1", 0.1, 32),
    (16, 10, "raw", 0.3, 8),
    (16, 3, "v1", 0.3, 4096),
    (100, 50, "v1", 0.1, 2048),
    (100, 50, "raw", 0.3, 512),
])
def test_redraw_update_equals_host_update_through_per_call_graphs(golden_dir, n, T, kind, dropout, batch_size):
    got_p, (c, tracker, actor, critic, dev), snap = _update_vs_host(golden_dir, n, T, kind, dropout, batch_size)
    # the same trajectory through the position-keyed learner: another graph, another tracker gradient
    mods = (tracker, actor, critic)
    c.buffer._traj.dropout_redraw = False
    try:
        _run(dev, c.buffer, batch_size, 2)
    finally:
        c.buffer._traj.dropout_redraw = True
    names = [k for k, _ in tracker.named_parameters()]
    j = names.index("transformer_encoder.layers.0.linear1.weight")
    assert not torch.equal(_params(mods)[j], got_p[j])
    _restore(mods, dev.optim, snap)


@pytest.mark.parametrize("n,T,kind", [(16, 10, "v1"), (100, 50, "raw")])
def test_without_dropout_the_redraw_update_is_the_ordinary_one(golden_dir, n, T, kind):
    out = []
    for redraw in (True, False):
        c, tracker, actor, critic, dev, _ = _collector(golden_dir, n, T, kind, redraw=redraw, buffer=True, learner="device")
        c.collect(n_episode=n)
        mods = (tracker, actor, critic)
        losses = _run(dev, c.buffer, 64, 2)
        out.append((mods, tracker, losses, _params(mods), _opt_states(mods, dev.optim),
                    np.asarray((dev.ret_rms.mean, dev.ret_rms.var, dev.ret_rms.count))))
    (mods, tracker, gl, gp, gs, gr), (_, _, wl, wp, ws, wr) = out
    _compare(mods, tracker, gl, wl, gp, wp, gs, ws, gr, wr)


def test_two_redraw_updates_from_one_snapshot_are_bit_identical(golden_dir):
    c, tracker, actor, critic, dev, _ = _collector(golden_dir, 16, 10, dropout=0.1, buffer=True, learner="device")
    c.collect(n_episode=16)
    mods = (tracker, actor, critic)
    snap = _snapshot(mods, dev.optim)
    l1 = _run(dev, c.buffer, 32, 2)
    p1 = _params(mods)
    _restore(mods, dev.optim, snap)
    l2 = _run(dev, c.buffer, 32, 2)
    assert l1 == l2
    for a, b in zip(p1, _params(mods)):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_a_second_collect_draws_other_masks(golden_dir):
    c, *_ = _collector(golden_dir, 16, 10, dropout=0.1)
    c.collect(n_episode=16)
    first = c.last_collect
    c.collect(n_episode=16)
    assert c.last_collect[2] != first[2]
    ro = c.rollout()
    a, b = ro.call_masks(first[2], 2), ro.call_masks(c.last_collect[2], 2)
    assert not torch.equal(a["pos"], b["pos"]) and not torch.equal(a[(1, 3)], b[(1, 3)])
    # and a call's masks are not its neighbour's, nor the position-keyed ones of the same positions
    assert not torch.equal(a["pos"][:, :2], ro.call_masks(first[2], 1)["pos"])
    assert not torch.equal(a["pos"], ro.masks(first[2], 3)["pos"])


def test_redraw_rollout_works_with_the_host_learner(golden_dir):
    """rollout="device", dropout_redraw=True under HostPPOPolicy: the buffer's obs carry the per-call graphs of redraw_states."""
    n, T = 16, 6
    c, tracker, actor, critic, policy, _ = _collector(golden_dir, n, T, dropout=0.1, buffer=True)
    before = _params((tracker,))
    c.collect(n_episode=n)
    assert c.buffer.obs.requires_grad
    losses = _run(policy, c.buffer, 32, 1)
    assert np.isfinite(losses["loss"]).all()
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(_params((tracker,)), before))


def test_onpolicy_trainer_two_epochs_redraw(golden_dir):
    from core.collector import Collector
    from core.trainer.onpolicy import onpolicy_trainer
    from tianshou.data import VectorReplayBuffer
    n, T = 100, 9
    train_env, base = case.venv(golden_dir, n, True, T)
    test_env, _ = case.venv(golden_dir, n, False, T)
    _, tracker, actor, critic, dev, _ = _collector(golden_dir, n, T, dropout=0.1, buffer=True, learner="device")
    train_env.seed(11)
    test_env.seed(12)
    torch.manual_seed(11)
    np.random.seed(11)
    train_c = Collector(dev, train_env, VectorReplayBuffer(n * T, n), preprocess_fn=tracker.build_state, rollout="device", dropout_redraw=True)
    test_c = Collector(dev, test_env, preprocess_fn=tracker.build_state, rollout="device", dropout_redraw=True)
    before = _params((tracker, actor))
    got = []
    orig = train_c.collect

    def spy(**kw):
        res = orig(**kw)
        got.append((res, len(train_c.buffer)))
        return res
    train_c.collect = spy
    losses = []
    orig_update = dev.update

    def spy_update(*a, **kw):
        out = orig_update(*a, **kw)
        losses.append(out)
        return out
    dev.update = spy_update
    onpolicy_trainer(dev, train_c, test_c, tracker, max_epoch=2, step_per_epoch=150, repeat_per_collect=2, episode_per_test=n,
                     batch_size=64, episode_per_collect=n, verbose=False)
    keys = {"rews", "lens", "idxs", "n/st", "n/ep", "rew", "rew_std", "len", "len_std"}
    assert len(got) >= 2 and len(losses) >= 2
    for res, rows in got:
        assert set(res) == keys and rows == res["n/st"]
    for rep in losses:
        assert set(rep) == {"loss", "loss/clip", "loss/vf", "loss/ent"} and all(np.isfinite(v).all() for v in rep.values())
    after = _params((tracker, actor))
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(after, before))
    assert all(torch.isfinite(a).all() for a in after)
