"""GPU: DeviceRollout.collect with a slot tracker (cirs_rollout_collect_{gru,lstm,avg,caser}) against the same vector steps issued one entry
point at a time from Python, bit for bit, in every mode; and against the float64 restatement of the tracker, teacher-forced on the device's
own actions.

The checks are written once here, over a record of tests/slotcase.py, which also holds the stepwise collect;
tests/test_gpu_{gru,lstm,avg,caser}_rollout.py bind them to their tracker under the test names and ids those files have always had.  (This
file is named like a test module so that pytest rewrites its assertions; it collects no item of its own.)"""
import numpy as np
import pytest
import torch

from slotcase import I, RNG_BASE, S, SEED, T, U, assert_same, build_stack, check_against_float64, check_contract, load_example, stepwise


@pytest.fixture(scope="module")
def tables():
    from cirs_hip.synthetic import make_tables
    return make_tables(U, I, seed=0)


def collect_equals_the_steps_issued_one_at_a_time(tables, slot, B, mode):
    kw = dict(remove=dict(remove_recommended_ids=True), force=dict(force_length=5)).get(mode, {})
    users = np.random.RandomState(B).randint(0, U, B)
    ro, p = build_stack(slot, tables, B, **kw)
    ref_ro, _ = build_stack(slot, tables, B, **kw)
    want = stepwise(ref_ro, users, greedy=mode == "greedy", remove=mode == "remove", force_length=5 if mode == "force" else 0)
    lengths = ro.collect(torch.as_tensor(users), seed=SEED, rng_base=RNG_BASE, greedy=mode == "greedy")
    assert_same(ro, lengths, want)
    check_contract(ro, lengths)
    check_against_float64(slot, ro, p, users, lengths)
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


def harness_noise_is_the_sampler_with_that_noise(tables, slot):
    B = 6
    users = np.random.RandomState(1).randint(0, U, B)
    ro, p = build_stack(slot, tables, B)
    g = -np.log(np.random.RandomState(3).exponential(size=(T, B, I))).astype(np.float32)
    lengths = ro.collect(torch.as_tensor(users), gumbel=g)
    ref_ro, _ = build_stack(slot, tables, B)
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
    check_against_float64(slot, ro, p, users, lengths)


def what_is_not_built_is_refused(tables, slot):
    from cirs_hip.rollout import DeviceRollout
    ro, _ = build_stack(slot, tables, 6)
    with pytest.raises(NotImplementedError, match=f"online-reward.*{slot.display} tracker"):
        DeviceRollout(ro.env, ro.tracker, ro.policy, online=object())
    with pytest.raises(NotImplementedError, match=f"sync_every.*{slot.display} tracker"):
        ro.collect(torch.zeros(6, dtype=torch.int64), sync_every=2)
    with pytest.raises(NotImplementedError, match=rf"run_steps.*{slot.display} tracker.*use collect\(\)"):
        ro.run_steps(0, 1, SEED, RNG_BASE)
    for exc, pattern, build in slot.engine_refusals(ro.tracker.params):
        with pytest.raises(exc, match=pattern):
            build()
    ex = load_example()
    args = ex.get_args(["--n-users", "60", "--n-items", "70", "--training-num", "4", "--max_turn", "6", "--tracker", slot.name,
                        *slot.flags(slot.example_model)])
    tab, train_envs, st, policy, coll = ex.build(args)
    assert type(st).__name__ == "StateTracker" + slot.display
    for k, v in slot.plugin_kw(slot.example_model).items():
        assert getattr(st, k) == v, k
    from core.collector import Collector
    with pytest.raises(ValueError, match="dropout_redraw"):
        Collector(policy, train_envs, preprocess_fn=st.build_state, dropout_redraw=True)
