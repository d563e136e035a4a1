"""The Kuaishou LinUCB baseline (reference core/policy/linucb.py) on synthetic files in the KuaiRec layout: one arm per item of the
evaluation env, the training log added to the arms' A and b on the device once per epoch (cirs_linucb_update, bit-identical to the
reference's per-row loop), and after every epoch the validation mae / mse (cirs_linucb_solve, cirs_linucb_predict) and the
evaluation loop test_kuaishou (cirs_linucb_score, then one lock-step rollout), one line per epoch.  The KuaiRec files of the reference
are not shipped.

    python examples/cirs_linucb_kuaishou_synth.py [--epoch 3] [--alpha 0.25] [--users 48]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))


class Lines:
    def info(self, msg):
        print(msg, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=0.25)
    ap.add_argument("--users", type=int, default=48)
    args = ap.parse_args()
    from cirs_hip.synthetic import write_kuairec_workspace
    from core.user_model_train import train_linucb_kuaishou
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        made = write_kuairec_workspace(data, n_users=args.users, n_env_users=args.users // 2)
        print(f"{len(made['big'])} log rows, {args.users} users, {len(made['env_items'])} arms")
        run = train_linucb_kuaishou(data, save_root=tmp, epoch=args.epoch, alpha=args.alpha, logger=Lines(), num_leave_compute=3,
                                    leave_threshold=1, max_turn=30)
        state = run.model.device_state
        touched = int((state.b.abs().sum(1) > 0).sum())
        print(f"{touched} of {state.K} arms saw a log row; d = {state.d}")
        user = int(made["env_users"][0])
        item, reward = run.model.recommend_k_item(user, run.val_set, k=1, is_softmax=False)
        print(f"recommendation for user {user}: item {int(item)}, predicted reward {reward:.4f}")
        for e, h in enumerate(run.history):
            print(f"epoch {e}: val mae {float(h['val_mae']):.4f} mse {float(h['val_mse']):.4f}  RL click_loss {h['RL_val_click_loss']:.4f} "
                  f"CV {h['RL_val_CV']} len_tra {h['RL_val_len_tra']:.2f} R_tra {h['RL_val_R_tra']:.3f}")


if __name__ == "__main__":
    main()
