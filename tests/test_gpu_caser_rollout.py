"""GPU: DeviceRollout.collect with the convolutional window tracker (cirs_rollout_collect_caser) against the same vector steps issued one entry point at
a time from Python, bit for bit, in every mode; and against the float64 restatement of the tracker, teacher-forced on the device's own
actions.  The stepwise collect and the checks are the LSTM rollout test's, with the Caser engine in the stack."""
import numpy as np
import pytest
import torch

import casercase
import envcase
import policycase
import rolloutcase
from cirs_hip import caser_host
from test_gpu_lstm_rollout import I, RNG_BASE, S, SEED, T, U, assert_same, check_contract, stepwise

pytestmark = pytest.mark.gpu
W, HEIGHTS, PSEED = 4, (2, 3), 2      # T = 8: the window slides from position 5 on


@pytest.fixture(scope="module")
def tables():
    from cirs_hip.synthetic import make_tables
    return make_tables(U, I, seed=0)


def build_stack(tab, B, **rollout_kw):
    from cirs_hip.caser_tracker import DeviceCaserTracker
    from cirs_hip.env import DeviceEnv, DeviceEnvTables
    from cirs_hip.policy import DevicePolicy
    from cirs_hip.rollout import DeviceRollout
    a_env, b_env = envcase.ab_env_tables(tab.raw_uid, tab.raw_pid, tab.alpha_u, tab.beta_i, U, I)
    dt = DeviceEnvTables(tab.mat, tab.normed_mat, tab.item_cats, alpha_env=a_env, beta_env=b_env)
    env = DeviceEnv(dt, B, num_leave_compute=3, leave_threshold=1, max_turn=T, tau=10.0, gamma_exposure=10.0, version="v1")
    p = casercase.caser_param_dict(U, I, PSEED, W, HEIGHTS, S=S)
    trk = DeviceCaserTracker({k: v.float().cuda().contiguous() for k, v in p.items()}, U, I, B, T, dim_state=S, window_size=W, filter_sizes=HEIGHTS)
    arrs = policycase.random_weights(np.random.RandomState(2), I)
    pol = DevicePolicy({rolloutcase.POLICY_NAMES[k]: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in arrs.items()}, I)
    return DeviceRollout(env, trk, pol, **rollout_kw), p


def check_against_float64(ro, p, users, lengths):
    """the independent check: the float64 restatement, teacher-forced on the device's users / acts / rews, reproduces traj.obs"""
    act = ro.traj.act.cpu().numpy().T.copy(); rew = ro.traj.rew.cpu().numpy().T.copy()
    ln = lengths.cpu().numpy()
    s64 = caser_host.states(caser_host.cast_params(p, torch.float64), users, act, rew, W).numpy()
    s32 = caser_host.states(caser_host.cast_params(p, torch.float32), users, act, rew, W).numpy()
    live = np.arange(T + 1)[None, :] <= ln[:, None]      # an env of length n has states 0 .. n
    got = ro.traj.obs.cpu().numpy().transpose(1, 0, 2)
    scale = np.abs(s64[live]).max()
    err, err32 = np.abs(got[live] - s64[live]).max() / scale, np.abs(s32[live] - s64[live]).max() / scale
    bar = casercase.bar_for(casercase.STATE_BAR, err32)
    print(f"rollout obs B={len(ln)}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("B", [6, 70])
@pytest.mark.parametrize("mode", ["sampled", "greedy", "remove", "force"])
def test_collect_equals_the_steps_issued_one_at_a_time(tables, B, mode):
    kw = dict(remove=dict(remove_recommended_ids=True), force=dict(force_length=5)).get(mode, {})
    users = np.random.RandomState(B).randint(0, U, B)
    ro, p = build_stack(tables, B, **kw)
    ref_ro, _ = build_stack(tables, B, **kw)
    want = stepwise(ref_ro, users, greedy=mode == "greedy", remove=mode == "remove", force_length=5 if mode == "force" else 0)
    lengths = ro.collect(torch.as_tensor(users), seed=SEED, rng_base=RNG_BASE, greedy=mode == "greedy")
    assert_same(ro, lengths, want)
    check_contract(ro, lengths)
    check_against_float64(ro, p, users, lengths)
    act, ln = ro.traj.act.cpu().numpy(), lengths.cpu().numpy()
    if mode == "remove":
        for b in range(B):
            a = act[:ln[b], b]
            assert len(set(a.tolist())) == len(a), f"env {b} lists an item twice"
    if mode == "force":
        assert (ln == 5).all()
    # a second collect on the same objects: every entry is rewritten, nothing is left over from the first
    lengths2 = ro.collect(torch.as_tensor(users), seed=SEED, rng_base=RNG_BASE, greedy=mode == "greedy")
    live = torch.arange(T + 1, device="cuda")[:, None] <= lengths[None, :].to(torch.int64)
    assert torch.equal(lengths2, lengths) and torch.equal(ro.traj.act, want["act"]) and torch.equal(ro.traj.obs[live], want["obs"][live])


def test_harness_noise_is_the_sampler_with_that_noise(tables):
    B = 6
    users = np.random.RandomState(1).randint(0, U, B)
    ro, p = build_stack(tables, B)
    g = -np.log(np.random.RandomState(3).exponential(size=(T, B, I))).astype(np.float32)
    lengths = ro.collect(torch.as_tensor(users), gumbel=g)
    ref_ro, _ = build_stack(tables, B)
    env, trk, pol = ref_ro.env, ref_ro.tracker, ref_ro.policy
    users_d = torch.as_tensor(users).to("cuda", torch.int32)
    env.reset(users_d); trk.reset()
    obs = trk.init(users_d)
    gd = torch.as_tensor(g).cuda()
    for t in range(T):
        act, logp, value = pol.sample(obs, gumbel=gd[t], skip=env.done)
        assert torch.equal(act, ro.traj.act[t]) and torch.equal(logp, ro.traj.logp[t])
        _, r, d, c, _ = env.step(act)
        nxt = torch.zeros_like(obs)
        trk.step(act, r, out=nxt, out_stride=S)
        obs = nxt
    check_contract(ro, lengths)
    check_against_float64(ro, p, users, lengths)


def test_what_is_not_built_is_refused(tables):
    from cirs_hip.rollout import DeviceRollout
    ro, _ = build_stack(tables, 6)
    with pytest.raises(NotImplementedError, match="online-reward.*Caser tracker"):
        DeviceRollout(ro.env, ro.tracker, ro.policy, online=object())
    with pytest.raises(NotImplementedError, match="sync_every.*Caser tracker"):
        ro.collect(torch.zeros(6, dtype=torch.int64), sync_every=2)
    with pytest.raises(NotImplementedError, match=r"run_steps.*Caser tracker.*use collect\(\)"):
        ro.run_steps(0, 1, SEED, RNG_BASE)
    with pytest.raises(ValueError, match="window_size"):
        from cirs_hip.caser_tracker import DeviceCaserTracker
        DeviceCaserTracker(ro.tracker.params, U, I, 6, T, dim_state=S, window_size=17, filter_sizes=HEIGHTS)
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cirs_rl_kuaishou_synth", os.path.join(root, "examples", "cirs_rl_kuaishou_synth.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    args = ex.get_args(["--n-users", "60", "--n-items", "70", "--training-num", "4", "--max_turn", "6", "--tracker", "caser", "--window-size", "3", "--filter-sizes", "1,3"])
    tab, train_envs, st, policy, coll = ex.build(args)
    assert type(st).__name__ == "StateTrackerCaser" and st.window_size == 3 and st.filter_sizes == (1, 3)
    from core.collector import Collector
    with pytest.raises(ValueError, match="dropout_redraw"):
        Collector(policy, train_envs, preprocess_fn=st.build_state, dropout_redraw=True)
