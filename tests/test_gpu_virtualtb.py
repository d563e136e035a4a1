"""GPU: the batched device VirtualTaobao env (csrc/virtualtb.hip, cirs_hip/virtualtb.py) against the CPU mirror of VirtualTB /
SimulatedEnv(VirtualTB-v0) (pinned to the reference by tests/test_virtualtb_cpu.py) fed with the device's own Philox noise
(tests/vtbcase.py).  Exit decisions, click and user draws are exact (draws under the top-2 margin protocol), the fp32 user-model
reward within rtol 1e-5, the fp64 exposure effect within rtol 1e-12."""
import numpy as np
import pytest
import torch

import vtbcase
from vtbcase import GROUPS, STATS

pytestmark = pytest.mark.gpu

N_LEAVE, THR, T = 5, 3.0, 50
# The user-model reward: the device sums the MMoE in fp64 (one rounding per layer output), the mirror is torch's fp32 CPU forward.
# torch's fp32 result itself is off from the fp64 one by up to ~3e-5 absolute (3000 random Taobao inputs, outputs in [-11, 8]: the
# 118-128-term sums cancel), so the absolute part of the bar is 1e-4 instead of 1e-6.
SIM_TOL = dict(rtol=1e-5, atol=1e-4)


def _engine(golden_dir, n, simulated, version="v1", tau=1.0, gamma=1.0, use_exposure=True, seed=1234, T_=T):
    from cirs_hip.virtualtb import DeviceVirtualTB
    base = vtbcase.base_vtb(golden_dir, N_LEAVE, THR, T_)
    model = vtbcase.golden_mmoe(golden_dir)[0] if simulated else None
    eng = DeviceVirtualTB(base, n, user_model=model, version=version, tau=tau, gamma_exposure=gamma,
                          use_exposure_intervention=use_exposure, seed=seed, device="cuda")
    return eng, base, model


def _onehot(pos):
    o = np.zeros(88)
    o[pos] = 1.0
    return o


@pytest.mark.parametrize("n", [4, 257, 1024])
def test_user_draw_matches_cpu(golden_dir, n):
    eng, base, _ = _engine(golden_dir, n, False, seed=99 + n)
    obs = eng.reset().cpu().numpy()
    tu = eng.task_user.cpu().numpy()
    nz = vtbcase.fetch_noise(eng, n, 1)[:, 0]
    with torch.no_grad():
        x = base.generator(torch.from_numpy(nz[:, 21:149].copy()))
    before = STATS["forced"]
    for i in range(n):
        for gi, (lo, hi) in enumerate(GROUPS):
            vtbcase.pick(x[i, lo:hi], nz[i, 149 + lo:149 + hi], tu[i, gi] - lo, f"env {i} group {gi}")
        np.testing.assert_array_equal(obs[i], np.r_[_onehot(tu[i]), 0, 0, 0])
    assert STATS["forced"] == before, "no draw disagreements expected on the fixed seeds"
    print(f"user draws: {n * 11}, smallest CPU top-2 margin seen {STATS['min_gap']:.3g}")


def _pick_actions(rng, mirrors, ids, repeat_p):
    """fp32 actions: uniform [-1, 1]^27 or an exact repeat of a window entry (d = 0 forces the exit); fresh draws closer than 1e-3 to
    the exit threshold are redrawn so that exit decisions do not hinge on round-off."""
    acts = np.empty((len(ids), 27), np.float32)
    for j, i in enumerate(ids):
        env = vtbcase.inner(mirrors[i])
        t = env.total_turn
        window = [np.asarray(env.history_action[k], np.float64) for k in range(max(0, t - N_LEAVE + 1), t) if k in env.history_action]
        if window and rng.rand() < repeat_p[i]:
            acts[j] = window[rng.randint(len(window))]
            continue
        while True:
            a = rng.uniform(-1, 1, 27).astype(np.float32)
            if all(abs(np.linalg.norm(a.astype(np.float64) - w) - THR) > 1e-3 for w in window):
                break
        acts[j] = a
    return acts


def _run_parity(golden_dir, n, simulated, steps, version="v1", tau=1.0, gamma=1.0, use_exposure=True, seed=5):
    eng, base, model = _engine(golden_dir, n, simulated, version, tau, gamma, use_exposure, seed=seed)
    events = 2 * steps + 2
    noise = vtbcase.fetch_noise(eng, n, events)
    mirrors = vtbcase.make_mirrors(base, n, noise, model, version, tau, gamma, use_exposure)
    rng = np.random.RandomState(seed)
    keeps = np.arange(n) % 3 == 0       # a third of the envs repeat no action and are never reset after done: they reach max_turn
    repeat_p = np.where(keeps, 0.0, 0.25)
    forced0 = STATS["forced"]
    obs0 = eng.reset().cpu().numpy()
    tu = eng.task_user.cpu().numpy()
    for i in range(n):
        vtbcase.inner(mirrors[i]).force_user = tu[i]
        np.testing.assert_array_equal(mirrors[i].reset(), obs0[i])
    n_exit = n_maxturn = n_cont = 0
    last_done = np.zeros(n, bool)
    for step in range(steps):
        turns = eng.host_turn.copy()
        # done envs are reset only half of the time (the others keep stepping, as HostCollector does); the simulated kind must reset
        # past max_turn; a random tenth of the envs sits the step out (id subsets)
        want_reset = np.flatnonzero((last_done & ~keeps & (rng.rand(n) < 0.5)) | (simulated & (turns > T)))
        if len(want_reset):
            ob = eng.reset(want_reset).cpu().numpy()
            tu = eng.task_user.cpu().numpy()
            for j, i in enumerate(want_reset):
                vtbcase.inner(mirrors[i]).force_user = tu[i]
                np.testing.assert_array_equal(mirrors[i].reset(), ob[j])
            last_done[want_reset] = False
            turns = eng.host_turn.copy()
        ids = np.flatnonzero(rng.rand(n) >= 0.1)
        if len(ids) == 0:
            continue
        n_cont += int(last_done[ids].sum())
        acts = _pick_actions(rng, mirrors, ids, repeat_p)
        o, r, d, c, x = (v.cpu().numpy() for v in eng.step(torch.from_numpy(acts), ids, want_exposure=True))
        d = d.astype(bool)
        tu = eng.task_user.cpu().numpy()
        for j, i in enumerate(ids):
            m, t = mirrors[i], int(turns[i])
            env = vtbcase.inner(m)
            env.force_user = tu[i]
            env.force_ab = (int(r[j]), None if d[j] else int(o[j, 28])) if not simulated else (None, None)
            s, rr, dd, info = m.step(acts[j])
            what = f"step {step} env {i} t {t}"
            assert bool(dd) == d[j], what
            np.testing.assert_array_equal(o[j, :27], np.asarray(s[:27], np.float64), err_msg=what)
            assert o[j, 29] == s[29] == t + 1, what
            if simulated:
                np.testing.assert_allclose([o[j, 27], r[j], c[j]], [float(s[27]), float(rr), float(info["CTR"])], err_msg=what, **SIM_TOL)
                assert o[j, 28] == 0.0
                if t < T and use_exposure:
                    np.testing.assert_allclose(x[j], m.history_exposure[t], rtol=1e-12, atol=0, err_msg=what)
            else:
                np.testing.assert_array_equal(o[j], np.asarray(s, np.float64), err_msg=what)
                assert r[j] == rr, what
                np.testing.assert_allclose(c[j], info["CTR"], rtol=1e-12, err_msg=what)
            if d[j]:
                n_maxturn += t >= T - 1
                n_exit += t < T - 1
                np.testing.assert_array_equal(env.cur_user, _onehot(tu[i]), err_msg=what)
        last_done[ids] = d
    forced = STATS["forced"] - forced0
    print(f"{'simulated' if simulated else 'raw'} n={n}: exits {n_exit}, max_turn ends {n_maxturn}, steps of done envs {n_cont}, "
          f"forced draws {forced} of {STATS['draws']}, smallest margin {STATS['min_gap']:.3g}")
    assert n_exit > 0 and n_maxturn > 0 and n_cont > 0
    return eng


@pytest.mark.parametrize("n", [4, 100])
@pytest.mark.parametrize("version", ["v1", "v2"])
@pytest.mark.parametrize("expo", ["on", "off", "tau0"])
def test_step_parity_simulated(golden_dir, n, version, expo):
    tau = 0.0 if expo == "tau0" else 10.0
    _run_parity(golden_dir, n, True, 80, version=version, tau=tau, gamma=3.0, use_exposure=expo != "off", seed=11 + n)


def test_step_parity_simulated_1000(golden_dir):
    _run_parity(golden_dir, 1000, True, 70, version="v2", tau=10.0, gamma=3.0, seed=3)


@pytest.mark.parametrize("n", [4, 100, 1000])
def test_step_parity_raw(golden_dir, n):
    _run_parity(golden_dir, n, False, 80 if n < 1000 else 70, seed=21 + n)


def test_noise_contract(golden_dir):
    rng = np.random.RandomState(0)
    acts = rng.uniform(-1, 1, (6, 64, 27)).astype(np.float32)

    def run(seed):
        eng, _, _ = _engine(golden_dir, 64, True, seed=seed)
        outs = [eng.reset().cpu().numpy()]
        for k in range(6):
            outs += [v.cpu().numpy() for v in eng.step(torch.from_numpy(acts[k]))]
        return eng, outs

    e1, o1 = run(77)
    _, o2 = run(77)
    for a, b in zip(o1, o2):
        np.testing.assert_array_equal(a, b)
    _, o3 = run(78)
    assert not np.array_equal(o1[0], o3[0])
    # seed() restarts the stream: the same seed replays the same draws
    e1.seed(77)
    np.testing.assert_array_equal(e1.reset().cpu().numpy(), o1[0])
    # a reset of some ids leaves the others untouched
    e1.step(torch.from_numpy(acts[0]))
    snap = {k: getattr(e1, k).clone() for k in ("task_user", "sim_user", "turn", "event", "prev_reward", "cum_reward", "lst_action", "hist")}
    ids = np.array([3, 17, 40])
    e1.reset(ids)
    keep = np.setdiff1d(np.arange(64), ids)
    for k, v in snap.items():
        assert torch.equal(getattr(e1, k)[keep], v[keep]), k
    assert (e1.turn[ids] == 0).all() and (e1.event[ids] == snap["event"][ids] + 1).all()
    # simulated kind: a step past max_turn is refused; the raw kind keeps stepping with done set
    es, _, _ = _engine(golden_dir, 2, True, T_=3)
    er, _, _ = _engine(golden_dir, 2, False, T_=3)
    es.reset(); er.reset()
    a = torch.zeros(2, 27)
    for t in range(4):
        es.step(a + t)
        d = er.step(a + t)[2].cpu().numpy()
        if t >= 2:
            assert d.all()
    with pytest.raises(ValueError):
        es.step(a)
    for _ in range(3):
        d = er.step(a)[2].cpu().numpy()
        assert d.all()


def test_user_distribution(golden_dir):
    """Group frequencies of 65 536 user draws against the generator's soft-max averaged over the same z, within 5 sigma."""
    n = 65536
    eng, base, _ = _engine(golden_dir, n, False, seed=4242, T_=2)
    eng.reset()
    tu = eng.task_user.cpu().numpy()
    z = vtbcase.fetch_noise(eng, n, 1)[:, 0, 21:149]
    with torch.no_grad():
        x = base.generator(torch.from_numpy(z.copy()))
    for gi, (lo, hi) in enumerate(GROUPS):
        p = torch.softmax(x[:, lo:hi].double(), 1).mean(0).numpy()
        f = np.bincount(tu[:, gi] - lo, minlength=hi - lo) / n
        sigma = np.sqrt(np.maximum(p * (1 - p), 1e-12) / n)
        assert (np.abs(f - p) <= 5 * sigma + 1e-9).all(), (gi, f, p)


def test_mmoe_kernel_matches_golden(golden_dir):
    eng, _, model = _engine(golden_dir, 4, True)
    _, z = vtbcase.golden_mmoe(golden_dir)
    y = eng.mmoe_forward(torch.from_numpy(z["mmoe_x"])).cpu().numpy()
    np.testing.assert_allclose(y, z["mmoe_y"][:, 0], rtol=1e-5, atol=1e-5)
    with torch.no_grad():
        np.testing.assert_allclose(y, model(torch.from_numpy(z["mmoe_x"])).numpy()[:, 0], rtol=1e-5, atol=1e-5)


# ---- plugin surface: DummyVectorEnv(..., device="cuda") under Collector / PPOPolicy ----------------------------------------------
def _recording(venv, log):
    step = venv.step

    def rec(action, id=None):
        ids = np.arange(venv.env_num) if id is None else np.atleast_1d(id)
        out = step(action, id)
        log.append((ids.copy(), np.asarray(action, np.float32).copy(), *[np.array(v) for v in out[:3]], np.array(out[3]["CTR"])))
        assert out[0].dtype == np.float64 and out[0].shape == (len(ids), 30) and out[2].dtype == bool
        return out

    venv.step = rec


PN, PTHR, PT = 4, 2.4, 9      # the plugin test's env: CIRS-RL-taobao.py's shape at the c1rl golden's size (tests/test_c1_rl_cpu.py)


def _replay(golden_dir, venv, log, simulated, model=None, version="v1", tau=10.0, gamma=3.0):
    """Every env's recorded actions, in order, through the noise-fed CPU mirror for that env's events."""
    n = venv.env_num
    eng = venv.vtb_env()
    steps = np.zeros(n, int)
    for ids, *_ in log:
        steps[ids] += 1
    noise = vtbcase.fetch_noise(eng, n, int(steps.max()) + 1)
    base = vtbcase.base_vtb(golden_dir, PN, PTHR, PT)
    mirrors = vtbcase.make_mirrors(base, n, noise, model, version, tau, gamma, True)
    for m in mirrors:      # the collect's one reset() is event 0 (seed() restarted the counters); draws checked by margin only
        m.reset()
    for ids, acts, o, r, d, c in log:
        for j, i in enumerate(ids):
            s, rr, dd, info = mirrors[i].step(acts[j])
            assert bool(dd) == d[j]
            np.testing.assert_array_equal(o[j, [0, 26, 29]], np.asarray(s, np.float64)[[0, 26, 29]])
            tol = SIM_TOL if simulated else dict(rtol=1e-12, atol=0)
            np.testing.assert_allclose(o[j], np.asarray(s, np.float64), **tol)
            np.testing.assert_allclose([r[j], c[j]], [float(rr), float(info["CTR"])], **tol)


def test_plugin_collect_and_update(golden_dir):
    import gym
    from gym.envs.registration import register
    from torch.distributions import Independent, Normal
    from core.collector import Collector
    from core.inputs import get_dataset_columns
    from core.policy.ppo import PPOPolicy
    from core.state_tracker import StateTrackerTransformer
    from tianshou.data import VectorReplayBuffer
    from tianshou.env import DummyVectorEnv
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ActorProb, Critic
    from cirs_hip import gymlite
    gymlite.install()
    B, dim_model, dim_state = 100, 27, 20
    model, _ = vtbcase.golden_mmoe(golden_dir)
    register(id="VirtualTB-v0", entry_point="environments.VirtualTaobao.virtualTB.envs.virtualTB:VirtualTB",
             kwargs=dict(num_leave_compute=PN, leave_threshold=PTHR, max_turn=PT, data_dir=golden_dir + "/virtualtb"))
    register(id="SimulatedEnv-v0", entry_point="core.env.simulatedEnv.simulated_env:SimulatedEnv",
             kwargs=dict(user_model=model, task_name="VirtualTB-v0", version="v1", tau=10.0, gamma_exposure=3.0))
    sim = gym.make("SimulatedEnv-v0")
    train_envs = DummyVectorEnv([lambda: gym.make("SimulatedEnv-v0") for _ in range(B)], device="cuda")
    test_envs = DummyVectorEnv([lambda: gym.make("VirtualTB-v0") for _ in range(B)], device="cuda")
    assert train_envs.host_mode and test_envs.host_mode
    uc, ac, fc, hu, ha, hf = get_dataset_columns(dim_model, envname="VirtualTB-v0")
    tracker = StateTrackerTransformer(uc, ac, fc, dim_model=dim_model, dim_state=dim_state, dim_max_batch=B, dataset="VirtualTB-v0",
                                      has_user_embedding=hu, has_action_embedding=ha, has_feedback_embedding=hf, nhead=3, d_hid=128,
                                      nlayers=2, dropout=0.1, device="cpu", seed=2022, MAX_TURN=PT)
    net = Net(dim_state, hidden_sizes=[64, 64], device="cpu")
    actor = ActorProb(net, sim.action_space.shape, max_action=sim.action_space.high[0], device="cpu")
    critic = Critic(net, device="cpu")
    optim = [torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=1e-3), torch.optim.Adam(tracker.parameters(), lr=1e-3)]
    policy = PPOPolicy(actor, critic, optim, lambda *logits: Independent(Normal(*logits), 1), discount_factor=0.95, max_grad_norm=0.5,
                       eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, reward_normalization=1, advantage_normalization=1, recompute_advantage=0,
                       value_clip=1, gae_lambda=0.95, action_space=sim.action_space)
    collector = Collector(policy, train_envs, VectorReplayBuffer(B * 4 * PT, B), preprocess_fn=tracker.build_state)
    assert type(collector).__name__ == "HostCollector"
    train_envs.seed(3)
    log = []
    _recording(train_envs, log)
    torch.manual_seed(0)
    res = collector.collect(n_episode=B)
    assert res["n/ep"] >= B and res["n/st"] == sum(len(e[0]) for e in log)
    n_done = sum(int(e[4].sum()) for e in log)
    assert n_done == res["n/ep"]
    assert (res["lens"] >= 1).all() and (res["lens"] <= PT).all()
    buf = collector.buffer
    idx = buf.sample_index(0)
    assert len(idx) == res["n/st"]
    np.testing.assert_allclose(np.sort(np.asarray(buf[idx].rew, np.float64)), np.sort(np.concatenate([e[3] for e in log])), rtol=1e-6)
    _replay(golden_dir, train_envs, log, True, model)
    before = [p.detach().clone() for p in list(tracker.parameters()) + list(actor.parameters())]
    losses = policy.update(0, buf, batch_size=64, repeat=2)
    for k, v in losses.items():
        assert np.isfinite(np.asarray(v, np.float64)).all(), k
    after = list(tracker.parameters()) + list(actor.parameters())
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(after, before))
    assert float((torch.cat([p.detach().reshape(-1) for p in tracker.parameters()]) -
                  torch.cat([p.reshape(-1) for p in before[:len(list(tracker.parameters()))]])).abs().max()) > 0
    # raw kind: a test collector over VirtualTB-v0
    test_collector = Collector(policy, test_envs, preprocess_fn=tracker.build_state)
    test_envs.seed(9)
    tlog = []
    _recording(test_envs, tlog)
    r2 = test_collector.collect(n_episode=B)
    assert r2["n/ep"] >= B and all(e[3].dtype == np.int64 for e in tlog)
    _replay(golden_dir, test_envs, tlog, False)
