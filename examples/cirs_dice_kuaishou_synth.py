"""The Kuaishou DICE debiasing baseline (reference DICE.py) on synthetic files in the KuaiRec layout: the 16-column training set with the
conformity score of every (positive, negative) pair, UserModel_DICE trained on the device (cirs_dice_train_epoch), a top-k
recommendation of the static-policy evaluation after every epoch (cirs_dice_forward), the validation mae / mse (cirs_dice_validate)
and the loss printed per epoch, epoch -1 (the untrained model) first.  The KuaiRec files
of the reference are not shipped.

    python examples/cirs_dice_kuaishou_synth.py [--epoch 5] [--batch_size 256] [--feature_dim 16]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch", type=int, default=5)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--feature_dim", type=int, default=16, choices=(8, 16, 32))
    ap.add_argument("--users", type=int, default=48)
    args = ap.parse_args()
    from cirs_hip.synthetic import write_kuairec_workspace
    from core.user_data import load_static_validate_data_kuaishou
    from core.user_model import metric_mae, metric_mse
    from core.user_model_train import EpochLines, train_dice_kuaishou
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        made = write_kuairec_workspace(data, n_users=args.users, n_env_users=args.users // 2)
        print(f"{len(made['big'])} log rows, {args.users} users")
        val_set = load_static_validate_data_kuaishou(args.feature_dim, args.feature_dim, data)
        user = int(made["big"]["user_id"].iloc[0])

        def rl_test(model):          # in the place of the script's test_static_model_in_RL_env partial
            _, raw, value = model.recommend_k_item(user, val_set, k=3, is_softmax=False)
            return {"top3": raw.tolist(), "top_value": float(value[0])}
        run = train_dice_kuaishou(data, save_root=tmp, epoch=args.epoch, batch_size=args.batch_size, feature_dim=args.feature_dim, lr=5e-3,
                                  rl_test=rl_test, metric_fun={"mae": metric_mae, "mse": metric_mse}, callbacks=[EpochLines()])
        score = run.train_set.score
        print(f"score column: {int((score > 0).sum())} rows +1, {int((score < 0).sum())} rows -1")
        for e, h in enumerate(run.history):
            print(f"epoch {e}: loss {h['loss']:.4f}  val mae {h['mae']:.4f} mse {h['mse']:.4f}  top-3 for user {user}: {h['top3']} (value {h['top_value']:.4f})")
        print("artefact:", os.path.basename(run.paths.params))


if __name__ == "__main__":
    main()
