"""Test-side builder of the CIRS-RL-taobao.py stack (tracker, ActorProb / Critic over a shared Net, PPOPolicy with Independent(Normal) and
action scaling) over VirtualTB-v0 / SimulatedEnv(VirtualTB-v0) vector envs built from the golden VirtualTB weights."""
import numpy as np
import torch

import vtbcase

N_LEAVE, THR = 4, 2.4


def make_env_fn(golden_dir, simulated, max_turn, version="v1", n_leave=N_LEAVE, thr=THR):
    """-> a factory of independent envs (each call builds its own VirtualTB; the user model is shared)."""
    from core.env.simulatedEnv.simulated_env import SimulatedEnv
    if not simulated:
        return lambda: vtbcase.base_vtb(golden_dir, n_leave, thr, max_turn)
    model = vtbcase.golden_mmoe(golden_dir)[0]

    def sim():
        base = vtbcase.base_vtb(golden_dir, n_leave, thr, max_turn)
        s = SimulatedEnv.__new__(SimulatedEnv)
        s.__dict__.update(dict(user_model=model, env_task=base, observation_space=base.observation_space, action_space=base.action_space,
                               env_name="VirtualTB-v0", version=version, tau=10.0, use_exposure_intervention=True, alpha_u=None,
                               beta_i=None, normed_mat=None, gamma_exposure=3.0, r_decay=1, cum_reward=0, total_turn=0))
        s._reset_history()
        return s
    return sim


def venv(golden_dir, n, simulated, max_turn, device="cuda", version="v1", **kw):
    """-> (vector env, one of its envs).  A device vector env only reads its first env's parameters: its n specs are one object."""
    from tianshou.env import DummyVectorEnv
    make = make_env_fn(golden_dir, simulated, max_turn, version, **kw)
    one = make()
    if device is None:
        return DummyVectorEnv([lambda: one] + [make for _ in range(n - 1)]), one
    return DummyVectorEnv([lambda: one for _ in range(n)], device=device), one


def stack(base, n, max_turn, dropout=0.0, seed=2022, dim_state=20, hidden=(64, 64)):
    """(tracker, actor, critic, policy) in the script's shapes (D = 27, nhead 3, d_hid 128, 2 layers)."""
    from torch.distributions import Independent, Normal
    from core.inputs import get_dataset_columns
    from core.policy.ppo import PPOPolicy
    from core.state_tracker import StateTrackerTransformer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ActorProb, Critic
    torch.manual_seed(seed)
    dim_model = 27
    uc, ac, fc, hu, ha, hf = get_dataset_columns(dim_model, envname="VirtualTB-v0")
    tracker = StateTrackerTransformer(uc, ac, fc, dim_model=dim_model, dim_state=dim_state, dim_max_batch=n, dataset="VirtualTB-v0",
                                      has_user_embedding=hu, has_action_embedding=ha, has_feedback_embedding=hf, nhead=3, d_hid=128,
                                      nlayers=2, dropout=dropout, device="cpu", seed=seed, MAX_TURN=max_turn)
    net = Net(dim_state, hidden_sizes=list(hidden), device="cpu")
    space = base.action_space
    actor = ActorProb(net, space.shape, max_action=space.high[0], device="cpu")
    critic = Critic(net, device="cpu")
    optim = [torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=1e-3), torch.optim.Adam(tracker.parameters(), lr=1e-3)]
    policy = PPOPolicy(actor, critic, optim, lambda *logits: Independent(Normal(*logits), 1), discount_factor=0.95, max_grad_norm=0.5,
                       eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, reward_normalization=1, advantage_normalization=1, recompute_advantage=0,
                       value_clip=1, gae_lambda=0.95, action_space=space)
    return tracker, actor, critic, policy


def replay_states(tracker, obs0, obs, rew, lens, grad=False):
    """The reference procedure: HostStateTracker.build_state step by step over a recorded collect (host arrays: obs0 [B, 91], obs [T, B, 30],
    rew [T, B], lens [B]) -> list over t of (active ids, states [k, S] at position t) for t = 0..max(lens)."""
    B = len(lens)
    out = []
    with torch.set_grad_enabled(grad):
        tracker.build_state(dim_batch=B, reset=True)
        ids = np.arange(B)
        out.append((ids, tracker.build_state(obs=obs0, env_id=ids)["obs"]))
        for t in range(int(lens.max())):
            ids = np.flatnonzero(lens > t)
            s = tracker.build_state(obs_next=obs[t, ids], rew=rew[t, ids], env_id=ids)["obs_next"]
            out.append((ids, s))
    return out
