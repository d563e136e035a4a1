"""CPU: the host side of the device VirtualTaobao rollout.  (a) The functional teacher-forced rebuild of the tracker states
(cirs_hip/vtb_host.py) equals HostStateTracker.forward at every prefix; with masks it applies exactly the given scales.  (b) The Box-Muller
restatement's fused multiply-add is single-rounding.  (c) Collector(..., rollout="device") refuses every configuration it does not serve,
with a clear message, and without the keyword the dispatch is unchanged."""
import numpy as np
import pytest
import torch

import vtbrolloutcase as case


def _tracker(T, dropout=0.0, seed=3):
    from core.inputs import get_dataset_columns
    from core.state_tracker import StateTrackerTransformer
    uc, ac, fc, hu, ha, hf = get_dataset_columns(27, envname="VirtualTB-v0")
    torch.manual_seed(seed)
    return StateTrackerTransformer(uc, ac, fc, dim_model=27, dim_state=20, dim_max_batch=4, dataset="VirtualTB-v0", has_user_embedding=hu,
                                   has_action_embedding=ha, has_feedback_embedding=hf, nhead=3, d_hid=128, nlayers=2, dropout=dropout,
                                   device="cpu", seed=seed, MAX_TURN=T)


def test_rebuild_with_unit_masks_equals_tracker_forward():
    from cirs_hip import vtb_host
    T, B = 12, 5
    tr = _tracker(T)
    g = torch.Generator().manual_seed(0)
    user = (torch.rand(B, 88, generator=g) < 0.1).float()
    rew = torch.rand(T, B, generator=g) * 3
    act = torch.randn(T, B, 27, generator=g)
    ones = {"pos": torch.ones(B, T + 1, 27)}
    for l in range(2):
        ones.update({(l, vtb_host.DROP_ATTN): torch.ones(B, T + 1, (T + 1) * 3), (l, vtb_host.DROP_RES1): torch.ones(B, T + 1, 27),
                     (l, vtb_host.DROP_FF): torch.ones(B, T + 1, 128), (l, vtb_host.DROP_RES2): torch.ones(B, T + 1, 27)})
    with torch.no_grad():
        slots = vtb_host.input_slots(tr, user, rew, act)
        got = vtb_host.states_from_slots(tr, slots, ones)
        plain = vtb_host.states_from_slots(tr, slots)
        assert got.shape == (T + 1, B, 20)
        torch.testing.assert_close(got, plain, rtol=0, atol=0)
        for j in range(T + 1):
            want = tr.forward(slots[:j + 1], tr._causal_mask(j + 1))
            np.testing.assert_allclose(got[j].numpy(), want.numpy(), rtol=1e-5, atol=1e-6)


def test_rebuild_slots_follow_build_state_and_carry_gradients():
    from cirs_hip import vtb_host
    T, B = 4, 3
    tr = _tracker(T)
    rng = np.random.RandomState(1)
    obs0 = np.concatenate([(rng.rand(B, 88) < 0.1).astype(np.float64), np.zeros((B, 3))], 1)
    obs = rng.randn(T, B, 30)
    rew = rng.rand(T, B)
    lens = np.array([T, 2, 1])
    steps = case.replay_states(tr, obs0, obs, rew, lens)
    st = vtb_host.tracker_states(tr, torch.as_tensor(obs0[:, :-3], dtype=torch.float32), torch.as_tensor(rew, dtype=torch.float32),
                                 torch.as_tensor(obs[:, :, :-3], dtype=torch.float32))
    for t, (ids, s) in enumerate(steps):
        np.testing.assert_allclose(st[t, ids].detach().numpy(), s.numpy(), rtol=1e-5, atol=1e-6)
    st.sum().backward()
    for name in ("ffn_user", "fnn_gate", "decoder"):
        assert float(getattr(tr, name).weight.grad.abs().sum()) > 0, name


def test_rebuild_applies_given_masks():
    from cirs_hip import vtb_host
    T, B = 3, 2
    tr = _tracker(T)
    g = torch.Generator().manual_seed(5)
    slots = torch.randn(T + 1, B, 27, generator=g)
    m = {"pos": torch.ones(B, T + 1, 27)}
    for l in range(2):
        m.update({(l, vtb_host.DROP_ATTN): torch.ones(B, T + 1, (T + 1) * 3), (l, vtb_host.DROP_RES1): torch.ones(B, T + 1, 27),
                  (l, vtb_host.DROP_FF): torch.ones(B, T + 1, 128), (l, vtb_host.DROP_RES2): torch.ones(B, T + 1, 27)})
    m["pos"][1, 2, 5] = 0.0                  # one dropped input element of env 1 at position 2
    with torch.no_grad():
        base = vtb_host.states_from_slots(tr, slots, None)
        got = vtb_host.states_from_slots(tr, slots, m)
    torch.testing.assert_close(got[:, 0], base[:, 0], rtol=0, atol=0)       # other env untouched
    torch.testing.assert_close(got[:2, 1], base[:2, 1], rtol=0, atol=0)     # causal: earlier positions untouched
    assert float((got[2:, 1] - base[2:, 1]).abs().max()) > 1e-4


def test_host_fma_is_single_rounding():
    from cirs_hip.vtb_host import fmaf
    # a*b + c lands exactly on a float32 midpoint after the float64 rounding, the exact value lies just above it
    a, b = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 + 2.0 ** -23)
    c = np.float32(-1.0)
    exact = (1.0 + 2.0 ** -23) ** 2 - 1.0        # 2^-22 + 2^-46, exactly representable in float64
    assert fmaf(a, b, c) == np.float32(exact)
    rng = np.random.RandomState(0)
    x, y, z = (rng.randn(10000).astype(np.float32) for _ in range(3))
    ref = np.array([float(np.float32(float(np.longdouble(p) * np.longdouble(q) + np.longdouble(r)))) for p, q, r in zip(x[:200], y[:200], z[:200])])
    np.testing.assert_array_equal(fmaf(x[:200], y[:200], z[:200]), ref.astype(np.float32))


def test_host_gaussian_is_standard_normal():
    from cirs_hip.vtb_host import gauss_noise
    z = gauss_noise(11, 2, np.repeat(np.arange(300), 20), np.tile(np.arange(20), 300)).astype(np.float64)
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert not np.array_equal(z, gauss_noise(11, 3, np.repeat(np.arange(300), 20), np.tile(np.arange(20), 300)))


# ---- routing -----------------------------------------------------------------------------------------------------------------------
def _taobao(golden_dir, device, simulated=True, n=3, T=5):
    env, base = case.venv(golden_dir, n, simulated, T, device=device)
    tracker, actor, critic, policy = case.stack(base, n, T)
    return env, tracker, policy


def test_device_rollout_collector_is_selected_by_the_keyword(golden_dir):
    from core.collector import Collector
    from core.vtb_collector import DeviceVtbCollector
    env, tracker, policy = _taobao(golden_dir, "cuda")
    c = Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="device")     # nothing touches the GPU before collect
    assert isinstance(c, DeviceVtbCollector) and c.env_num == 3
    with pytest.raises(NotImplementedError, match="host loop"):
        c.collect(n_episode=3, random=True)
    with pytest.raises(ValueError, match="n_episode"):
        c.collect(n_episode=2)
    with pytest.raises(ValueError, match="rollout must be"):
        Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="gpu")


def test_without_the_keyword_dispatch_is_unchanged(golden_dir):
    from core.collector import Collector
    from core.host_rl import HostCollector
    env, tracker, policy = _taobao(golden_dir, None)
    assert type(Collector(policy, env, None, preprocess_fn=tracker.build_state)) is HostCollector


def test_device_rollout_refuses_a_host_env_without_device(golden_dir):
    from core.collector import Collector
    env, tracker, policy = _taobao(golden_dir, None)
    with pytest.raises(ValueError, match=r"device='cuda'"):
        Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="device")


def test_device_rollout_refuses_a_kuaishou_env():
    from core.collector import Collector
    from environments.KuaishouRec.env.kuaishouEnv import KuaishouEnv
    from tianshou.env import DummyVectorEnv
    spec = KuaishouEnv(mat=np.zeros((3, 4)), lbe_user=np.arange(3), lbe_photo=np.arange(4), list_feat=[[0]] * 4, df_photo_env=None,
                       df_dist_small=None, max_turn=5)
    env = DummyVectorEnv([lambda: spec for _ in range(2)])
    assert not env.host_mode
    with pytest.raises(ValueError, match="KuaishouEnv"):
        Collector(object(), env, None, preprocess_fn=None, rollout="device")


def test_device_rollout_refuses_a_discrete_actor(golden_dir):
    from torch.distributions import Categorical
    from core.collector import Collector
    from core.host_rl import HostPPOPolicy
    from gym import spaces
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import Actor, Critic
    env, tracker, _ = _taobao(golden_dir, "cuda")
    net = Net(20, hidden_sizes=[16], device="cpu")
    actor, critic = Actor(net, 27, device="cpu"), Critic(net, device="cpu")
    opt = [torch.optim.Adam(list(actor.parameters()) + list(critic.parameters())), torch.optim.Adam(tracker.parameters())]
    policy = HostPPOPolicy(actor, critic, opt, Categorical, action_space=spaces.Discrete(27))
    with pytest.raises(ValueError, match="discrete"):
        Collector(policy, env, None, preprocess_fn=tracker.build_state, rollout="device")
