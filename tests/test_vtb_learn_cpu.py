"""CPU: the dispatch of PPOPolicy(..., learner="device") (core/policy/ppo.py, core/vtb_learner.py), what the device VirtualTaobao learner
refuses, and the host side of its parameter images (cirs_hip/vtb_learn.py: packing, write-back, the shared trunk's double Adam clock).
No GPU and no library needed."""
import numpy as np
import pytest
import torch
from torch.distributions import Independent, Normal

DIST = lambda *logits: Independent(Normal(*logits), 1)      # noqa: E731


def _stack(conditioned_sigma=False, mu_hidden=(), optim=None, seed=3):
    from core.inputs import get_dataset_columns
    from core.state_tracker import StateTrackerTransformer
    from gym import spaces
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ActorProb, Critic
    torch.manual_seed(seed)
    uc, ac, fc, hu, ha, hf = get_dataset_columns(27, envname="VirtualTB-v0")
    tracker = StateTrackerTransformer(uc, ac, fc, dim_model=27, dim_state=20, dim_max_batch=4, dataset="VirtualTB-v0", has_user_embedding=hu,
                                      has_action_embedding=ha, has_feedback_embedding=hf, nhead=3, d_hid=128, nlayers=2, dropout=0.0,
                                      device="cpu", seed=seed, MAX_TURN=5)
    net = Net(20, hidden_sizes=[64, 64], device="cpu")
    space = spaces.Box(low=-1.0, high=1.0, shape=(27,), dtype=np.float32)
    actor = ActorProb(net, space.shape, hidden_sizes=mu_hidden, max_action=1.0, device="cpu", conditioned_sigma=conditioned_sigma)
    critic = Critic(net, device="cpu")
    make = optim or (lambda ps: torch.optim.Adam(ps, lr=1e-3))
    opt = [make(list(actor.parameters()) + list(critic.parameters())), make(list(tracker.parameters()))]
    return tracker, actor, critic, opt, space


def _policy(**kw):
    from core.policy.ppo import PPOPolicy
    stack_kw = {k: kw.pop(k) for k in ("conditioned_sigma", "mu_hidden", "optim") if k in kw}
    tracker, actor, critic, opt, space = _stack(**stack_kw)
    return PPOPolicy(actor, critic, opt, DIST, action_space=space, **kw), (tracker, actor, critic, opt)


def test_learner_device_dispatches_to_the_device_vtb_policy():
    from core.host_rl import HostPPOPolicy
    from core.vtb_learner import DeviceVtbPPOPolicy
    pol, _ = _policy(learner="device")
    assert type(pol) is DeviceVtbPPOPolicy and isinstance(pol, HostPPOPolicy)


@pytest.mark.parametrize("kw", [{}, {"learner": None}])
def test_without_learner_the_policy_is_exactly_the_host_one(kw):
    from core.host_rl import HostPPOPolicy
    pol, _ = _policy(**kw)
    assert type(pol) is HostPPOPolicy


@pytest.mark.parametrize("bad", ["host", "cuda", 1, True])
def test_bad_learner_values_are_refused(bad):
    with pytest.raises(ValueError, match="learner"):
        _policy(learner=bad)


def test_discrete_actor_with_the_keyword_is_refused():
    from core.policy.ppo import PPOPolicy
    with pytest.raises(ValueError, match="learner='device'"):
        PPOPolicy(torch.nn.Linear(2, 2), torch.nn.Linear(2, 1), [None, None], None, learner="device")


@pytest.mark.parametrize("kw,match", [
    (dict(optim=lambda ps: torch.optim.SGD(ps, lr=1e-3)), "Adam only"),
    (dict(optim=lambda ps: torch.optim.Adam(ps, lr=1e-3, amsgrad=True)), "amsgrad"),
    (dict(optim=lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-4)), "weight_decay"),
    (dict(optim=lambda ps: torch.optim.Adam(ps, lr=1e-3, maximize=True)), "maximize"),
    (dict(mu_hidden=(16,)), "hidden layers"),
])
def test_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        _policy(learner="device", **kw)


def test_conditioned_sigma_is_accepted():
    from core.vtb_learner import DeviceVtbPPOPolicy
    pol, _ = _policy(learner="device", conditioned_sigma=True)
    assert isinstance(pol, DeviceVtbPPOPolicy)


def test_update_refuses_a_buffer_that_is_not_from_a_device_collect():
    from tianshou.data import Batch, VectorReplayBuffer
    pol, _ = _policy(learner="device")
    buf = VectorReplayBuffer(8, 2)
    buf.add(Batch(obs=torch.zeros(2, 20), act=np.zeros((2, 27), np.float32), rew=np.zeros(2), done=np.ones(2, bool),
                  obs_next=torch.zeros(2, 20), info=Batch(), policy=Batch()), buffer_ids=np.arange(2))
    with pytest.raises(ValueError, match="device collect"):
        pol.update(0, buf, batch_size=2, repeat=1)


def _host_adam_steps(opt, params, k, seed=0):
    """k steps of the torch optimiser on random gradients (the reference's own clock)."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(k):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()


def test_image_round_trip_and_the_shared_trunk_clock():
    from cirs_hip.vtb_learn import check_optimisers, pack_image, policy_params, tracker_params, unpack_image
    tracker, actor, critic, opt, _ = _stack()
    ppar, tpar = policy_params(actor, critic), tracker_params(tracker)
    assert {id(p) for p in tpar} == {id(p) for p in tracker.parameters()} and len(tpar) == len(list(tracker.parameters()))
    n_trunk = check_optimisers(opt, ppar, tpar)
    assert n_trunk == 4                                   # Net(20, [64, 64]): two weights, two biases, listed twice in optim_RL
    # empty state = the first step: zero moments, step 0
    flat, m, v, steps = pack_image(ppar, opt[0])
    assert steps == {0} and float(m.abs().sum()) == 0 and float(v.abs().sum()) == 0
    assert flat.numel() == sum(p.numel() for p in ppar)
    # torch's own clock over the duplicated trunk: one state entry per parameter, the trunk's step advances by 2 per optimiser step
    _host_adam_steps(opt[0], ppar, 3)
    assert len(opt[0].state) == len(ppar)
    assert [int(float(opt[0].state[p]["step"])) for p in ppar] == [6] * n_trunk + [3] * (len(ppar) - n_trunk)
    flat, m, v, _ = pack_image(ppar, opt[0])
    want = [(p.detach().clone(), opt[0].state[p]["exp_avg"].clone(), opt[0].state[p]["exp_avg_sq"].clone()) for p in ppar]
    with torch.no_grad():
        for p in ppar:
            p.zero_()
    steps = [6] * n_trunk + [3] * (len(ppar) - n_trunk)
    unpack_image(ppar, opt[0], flat, m, v, steps)
    for p, (w, em, ev) in zip(ppar, want):
        torch.testing.assert_close(p.detach(), w, rtol=0, atol=0)
        torch.testing.assert_close(opt[0].state[p]["exp_avg"], em, rtol=0, atol=0)
        torch.testing.assert_close(opt[0].state[p]["exp_avg_sq"], ev, rtol=0, atol=0)
    # a fresh optimiser gets state entries torch itself can step and checkpoint
    fresh = torch.optim.Adam(tpar, lr=1e-3)
    tflat, tm, tv, tsteps = pack_image(tpar, fresh)
    unpack_image(tpar, fresh, tflat, tm + 0.5, tv + 0.25, [1] * len(tpar))
    sd = fresh.state_dict()
    assert len(sd["state"]) == len(tpar) and all(float(s["step"]) == 1.0 for s in sd["state"].values())
    _host_adam_steps(fresh, tpar, 1)
    assert all(float(fresh.state[p]["step"]) == 2.0 for p in tpar)


def test_sample_layout_segments_follow_the_host_boundaries():
    from cirs_hip.vtb_learn import sample_layout
    rows = np.array([0, 1, 2, 10, 11, 20])
    done = np.array([False, False, True, False, False, True])
    env, t, boundary, ends = sample_layout(rows, 10, None, done, np.array([11]))
    np.testing.assert_array_equal(env, [0, 0, 0, 1, 1, 2])
    np.testing.assert_array_equal(t, [0, 1, 2, 0, 1, 0])
    np.testing.assert_array_equal(boundary, [False, False, True, False, True, True])
    np.testing.assert_array_equal(ends, [3, 5, 6])
