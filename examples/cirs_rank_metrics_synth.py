"""Offline ranking evaluation on synthetic files in the KuaiRec layout: the DeepFM user model fitted for an epoch and an (untrained) PPO policy
over the same env catalogue, both scored at k = 10 on all env users against the fully observed env matrix -- Precision / Recall / HR / MRR /
NDCG / ILD / CV @k (cirs_rows_topk, cirs_actor_topk, cirs_rank_metrics).  The KuaiRec files of the reference are not shipped.

    python examples/cirs_rank_metrics_synth.py [--k 10] [--rel-threshold 1.0] [--epoch 1]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))


def build_policy(env, dim_state=20, dim_model=32, seed=2023):
    """The RL script's model wiring (examples/cirs_rl_kuaishou_synth.py) for `env`: (state tracker, PPOPolicy), untrained."""
    import warnings

    import torch

    from core.inputs import get_dataset_columns
    from core.policy.ppo import PPOPolicy
    from core.state_tracker import StateTrackerTransformer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.discrete import Actor, Critic
    device = torch.device("cuda:0")
    torch.manual_seed(seed)
    n_users, n_items = env.mat.shape
    user_columns, action_columns, feedback_columns, has_u, has_a, has_f = get_dataset_columns(dim_model, envname="KuaishouEnv-v0", env=env)
    tracker = StateTrackerTransformer(user_columns, action_columns, feedback_columns, dim_model=dim_model, dim_state=dim_state,
                                      dim_max_batch=n_users, dataset="KuaishouEnv-v0", has_user_embedding=has_u, has_action_embedding=has_a,
                                      has_feedback_embedding=has_f, nhead=4, d_hid=128, nlayers=2, dropout=0.0, device=device, seed=seed,
                                      MAX_TURN=env.max_turn).to(device)
    net = Net(dim_state, hidden_sizes=[64, 64], device=device)
    actor, critic = Actor(net, n_items, device=device).to(device), Critic(net, device=device).to(device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # the shared trunk appears twice in the parameter list, like the reference
        optim_RL = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=1e-3)
    policy = PPOPolicy(actor, critic, [optim_RL, torch.optim.Adam(tracker.parameters(), lr=1e-3)], torch.distributions.Categorical,
                       reward_normalization=1, value_clip=1, action_bound_method="", action_scaling=False)
    return tracker, policy


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rel-threshold", type=float, default=1.0, help="an item is relevant iff its watch ratio is at least this")
    ap.add_argument("--epoch", type=int, default=1)
    ap.add_argument("--users", type=int, default=48)
    args = ap.parse_args(argv)
    import numpy as np

    import evaluation
    from cirs_hip.synthetic import write_kuairec_workspace
    from core.user_model_train import train_user_model
    from environments.KuaishouRec.env.kuaishouEnv import KuaishouEnv
    from tianshou.data import Batch
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        write_kuairec_workspace(data, n_users=args.users, n_env_users=args.users // 2)
        run = train_user_model(data, save_root=tmp, tau=800.0, feature_dim=8, batch_size=256, epoch=args.epoch, lr=5e-3)
        env = KuaishouEnv(*KuaishouEnv.load_mat(data), num_leave_compute=1, leave_threshold=0, max_turn=30)
        n_users, n_items = env.mat.shape
        print(f"{n_users} env users x {n_items} env items, k = {args.k}, relevant: watch ratio >= {args.rel_threshold}")
        res = evaluation.test_ranking_kuaishou(run.model, env, run.val_set, k=args.k, rel_threshold=args.rel_threshold)
        user_model = {name: v for name, v in res.items() if name not in ("per_row", "ids")}
        print("user model:", user_model)
        tracker, policy = build_policy(env)
        users = np.arange(n_users)
        tracker.build_state(dim_batch=n_users, reset=True)
        state = tracker.build_state(obs=users, env_id=users)["obs"]          # the state in front of every user's first recommendation
        res = policy.rank_metrics(Batch(obs=state), users, env, args.k, rel_threshold=args.rel_threshold)
        ppo = {name: v for name, v in res.items() if name != "per_row"}
        print("PPO policy (untrained):", ppo)
    return user_model, ppo


if __name__ == "__main__":
    main()
