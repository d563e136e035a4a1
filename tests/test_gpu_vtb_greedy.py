"""GPU: deterministic evaluation of the VirtualTaobao policy on the device rollout (reference core/policy/ppo.py:152-153: in eval mode a
continuous actor's action is logits[0], the mean): act = mu, no Gaussian draw, in the position-keyed and the exact-redraw collect."""
import numpy as np
import pytest
import torch

import vtbrolloutcase as case

pytestmark = pytest.mark.gpu

T = 8
DROPOUTS = {"none": dict(dropout=0.0), "position_keyed": dict(dropout=0.1), "redraw": dict(dropout=0.1, dropout_redraw=True)}


def _collector(golden_dir, n, flag, dropout=0.0, dropout_redraw=False, buffer=False):
    from core.collector import Collector
    from tianshou.data import VectorReplayBuffer
    env, base = case.venv(golden_dir, n, True, T)
    tracker, actor, critic, policy = case.stack(base, n, T, dropout=dropout, seed=2022)
    policy._deterministic_eval = flag            # what PPOPolicy(..., deterministic_eval=True) stores
    env.seed(7)
    buf = VectorReplayBuffer(n * T, n) if buffer else None
    c = Collector(policy, env, buf, preprocess_fn=tracker.build_state, rollout="device", dropout_redraw=dropout_redraw)
    return c, actor, policy


def _traj(c):
    return {k: v.cpu().clone() for k, v in c.rollout().traj.items()}


@pytest.mark.parametrize("mode", list(DROPOUTS))
@pytest.mark.parametrize("n", [4, 37])
def test_eval_collect_takes_the_mean_action(golden_dir, n, mode):
    c, actor, policy = _collector(golden_dir, n, True, **DROPOUTS[mode])
    policy.eval()
    res = c.collect(n_episode=n)
    tr = _traj(c)
    lens = tr["len"].numpy().astype(int)
    assert res["n/ep"] == n and res["n/st"] == lens.sum() and (lens >= 1).all() and (lens <= T).all()
    rows = [(t, e) for t in range(int(lens.max())) for e in np.flatnonzero(lens > t)]
    ts, es = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    with torch.no_grad():
        (mu, sigma), _ = actor(tr["state"][ts, es])      # the host actor on the recorded states
    act = tr["act"][ts, es]
    np.testing.assert_allclose(act.numpy(), mu.numpy(), rtol=1e-5, atol=1e-5)
    assert float(sigma.min()) > 1e-3                      # a sampled action would sit about sigma away
    np.testing.assert_array_equal(tr["act_mapped"][ts, es].numpy(), policy.map_action(act.numpy()))
    np.testing.assert_array_equal(tr["obs"][ts, es, :27].numpy(), tr["act_mapped"][ts, es].numpy().astype(np.float64))
    # train(): the sampled collect of a collector built without the flag, bit for bit (fresh stacks: a collect moves the env's event counters)
    c1, _, policy1 = _collector(golden_dir, n, True, **DROPOUTS[mode])
    c0, _, policy0 = _collector(golden_dir, n, False, **DROPOUTS[mode])
    policy1.train(); policy0.train()
    c1.collect(n_episode=n); c0.collect(n_episode=n)
    a, b = _traj(c1), _traj(c0)
    for k in ("act", "act_mapped", "state", "obs", "rew", "done", "len"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["act"], tr["act"])          # ... and a different one from the evaluation


def test_training_collector_in_eval_mode_fills_a_well_formed_buffer(golden_dir):
    n = 37
    c, actor, policy = _collector(golden_dir, n, True, buffer=True)
    policy.eval()
    res = c.collect(n_episode=n)
    assert res["n/ep"] == n and set(res) == {"rews", "lens", "idxs", "n/st", "n/ep", "rew", "rew_std", "len", "len_std"}
    assert len(c.buffer) == res["n/st"] == int(res["lens"].sum())
    batch, _ = c.buffer.sample(0)
    assert batch.act.shape == (res["n/st"], 27) and int(np.asarray(batch.done).sum()) == n
