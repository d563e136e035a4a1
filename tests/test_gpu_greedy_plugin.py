"""GPU: PPOPolicy(deterministic_eval=True) through the plugin surface (reference core/policy/ppo.py:56,149-151): in train() nothing changes,
in eval() forward / Collector.collect take the arg-max item; PPOPolicy.topk lists the k best items of a state."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--n-users", "100", "--n-items", "300", "--training-num", "16", "--episode-per-collect", "16", "--test-num", "8", "--batch-size", "64",
        "--max_turn", "12", "--tau", "10", "--dropout", "0", "--force_length", "5", "--leave_threshold", "0", "--num_leave_compute", "1",
        "--epoch", "1", "--step-per-epoch", "60"]


def _build(flag):
    spec = importlib.util.spec_from_file_location("cirs_rl_kuaishou_synth", os.path.join(ROOT, "examples", "cirs_rl_kuaishou_synth.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    args = ex.get_args(ARGS + (["--deterministic-eval"] if flag else []))
    return (ex, args) + tuple(ex.build(args))


def _traj(coll):
    """act, logp, rew, done whole; value and obs where an env was alive (rows behind an episode's end keep an older collect's entries)."""
    tr = coll._rollout.traj
    live = tr.act >= 0
    return [t.clone() for t in (tr.act, tr.logp, tr.rew, tr.done)] + [tr.value[live].clone(), tr.obs[:-1][live].clone()]


def test_flag_changes_eval_collects_only():
    users = np.random.RandomState(5).randint(0, 100, 16)
    ex, args, tab, envs, st, policy, coll = _build(True)
    assert policy._deterministic_eval is True
    _, _, _, _, st0, policy0, coll0 = _build(False)
    assert policy0._deterministic_eval is False and torch.equal(policy.flat, policy0.flat)
    # train(): the sampled collect of a policy built without the flag, bit for bit
    policy.train(); policy0.train()
    coll.collect(n_episode=16, users=users); coll0.collect(n_episode=16, users=users)
    sampled = _traj(coll)
    for a, b in zip(sampled, _traj(coll0)):
        assert torch.equal(a, b)
    # eval(): the greedy rollout (tests/test_gpu_greedy.py), here driven directly on the other stack's engines
    policy.eval()
    res = coll.collect(n_episode=16, users=users)
    assert res["n/ep"] == 16 and res["n/st"] == int(res["lens"].sum()) == len(coll.buffer)
    greedy = _traj(coll)
    ro0 = coll0._get_rollout()
    ro0.collect(torch.as_tensor(users), seed=123, rng_base=9, greedy=True)
    for a, b in zip(greedy, _traj(coll0)):
        assert torch.equal(a, b)
    assert not torch.equal(greedy[0], sampled[0])
    # without the flag eval() still samples; _collect_count advanced in eval mode too, so later sampled collects keep their draws
    policy0.eval()
    assert coll._collect_count == 2
    policy.train()
    coll.collect(n_episode=16, users=users); third = _traj(coll)
    coll0.collect(n_episode=16, users=users)                       # coll0's second counted collect ...
    coll0.collect(n_episode=16, users=users)                       # ... and its third: the same rng_base as coll's third
    for a, b in zip(third, _traj(coll0)):
        assert torch.equal(a, b)


def test_forward_and_topk():
    from tianshou.data import Batch
    ex, args, tab, envs, st, policy, coll = _build(True)
    obs = torch.randn(16, 20, generator=torch.Generator().manual_seed(1))
    policy.eval()
    out = policy.forward(Batch(obs=obs))
    act, logp, value = policy.device_policy().greedy(obs.cuda())
    assert torch.equal(out.act, act) and torch.equal(out.policy.logp, logp) and torch.equal(out.policy.value, value)
    again = policy.forward(Batch(obs=obs))
    assert torch.equal(again.act, act)
    policy.train()
    drawn = torch.stack([policy.forward(Batch(obs=obs)).act for _ in range(4)])
    assert not all(torch.equal(d, act) for d in drawn)              # train(): sampled, as without the flag
    top = policy.topk(Batch(obs=obs), 5)
    assert top.act.shape == (16, 5) and top.act.dtype == torch.int64 and top.policy.logp.shape == (16, 5)
    assert torch.equal(top.act[:, 0], act) and torch.equal(top.policy.logp[:, 0], logp)
    assert bool((top.act >= 0).all()) and all(len(set(r.tolist())) == 5 for r in top.act.cpu())
    assert bool((top.policy.logp[:, 1:] <= top.policy.logp[:, :-1]).all())
    with pytest.raises(ValueError):
        policy.topk(Batch(obs=obs), 33)


def _trainer_run(seed):
    from core.trainer.onpolicy import onpolicy_trainer
    ex, args, tab, envs, st, policy, coll = _build(True)
    policy.seed = seed                                              # the two runs differ in the sampler seed only
    cs = ex.build_test_collectors(args, policy, st)
    for k, c in enumerate(cs.collector_dict.values()):
        c.env.seed(100 + k)                                         # the users the test envs draw
    calls, orig = [], cs.collect

    def spy(*a, **kw):
        res = orig(*a, **kw)
        calls.append((policy.training, res))
        return res
    cs.collect = spy
    np.random.seed(args.seed)
    info = onpolicy_trainer(policy, coll, cs, st, args.epoch, args.step_per_epoch, args.repeat_per_collect, args.test_num, args.batch_size,
                            episode_per_collect=args.episode_per_collect, save_model_fn=lambda epoch, policy: None, verbose=False)
    return info, calls, cs


def test_trainer_epoch_with_collector_set_is_seed_independent_before_training():
    info, calls, cs = _trainer_run(11)
    assert info["test_episode"] == 2 * 8 and len(calls) == 2        # the evaluation before training + one per epoch
    assert all(not training for training, _ in calls), "test collects run with the policy in eval()"
    first = calls[0][1]
    assert {"n/st", "rew", "NX_0_n/st", "NX_0_rew", "NX_5_lens"} <= set(first) and (first["NX_5_lens"] == 5).all()
    acts = cs.collector_dict["NX_0"].buffer._traj.act.cpu().numpy()
    lens = cs.collector_dict["NX_0"].buffer._lengths
    for b in range(8):
        a = acts[:lens[b], b]
        assert len(set(a.tolist())) == len(a) and (a >= 0).all()
    # the evaluation of the untrained policy is its mode: a policy that differs only in its sampler seed gives the same FB / NX_0 / NX_k
    # results (the training collects in between are sampled, so the parameters -- and the later evaluations -- part ways)
    _, calls2, _ = _trainer_run(12)
    other = calls2[0][1]
    assert set(first) == set(other)
    for k in first:
        np.testing.assert_array_equal(np.asarray(first[k]), np.asarray(other[k]), err_msg=k)
