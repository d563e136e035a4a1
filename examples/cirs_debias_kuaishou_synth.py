"""The two Kuaishou debiasing baselines (reference DeepFM-IPS-pairwise.py, PD-pairwise.py) on synthetic files in the KuaiRec layout:
the score column counted on the device (cirs_item_bin_counts / cirs_item_bin_gather), UserModel_Pairwise trained on the device with
the method's loss (cirs_deepfm_train_epoch), the validation mae / mse (cirs_deepfm_validate) and the loss printed per epoch, epoch -1
(the untrained model) first.  The KuaiRec files of the reference are not shipped.

    python examples/cirs_debias_kuaishou_synth.py [--method ips pd] [--epoch 5] [--batch_size 256] [--gamma 0.1]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", nargs="+", choices=("ips", "pd"), default=("ips", "pd"))
    ap.add_argument("--epoch", type=int, default=5)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--users", type=int, default=48)
    args = ap.parse_args()
    from cirs_hip.synthetic import write_kuairec_workspace
    from core.user_model import metric_mae, metric_mse
    from core.user_model_train import EpochLines, train_debias_kuaishou
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        made = write_kuairec_workspace(data, n_users=args.users, n_env_users=args.users // 2)
        print(f"{len(made['big'])} log rows, {args.users} users")
        for method in args.method:
            run = train_debias_kuaishou(data, method=method, save_root=tmp, epoch=args.epoch, batch_size=args.batch_size, gamma=args.gamma, lr=5e-3,
                                        metric_fun={"mae": metric_mae, "mse": metric_mse}, callbacks=[EpochLines()])
            score = run.model._trainer._data[9]
            print(f"{method}: score column in [{float(score.min()):.4f}, {float(score.max()):.4f}]; loss per epoch "
                  + " ".join(f"{h['loss']:.4f}" for h in run.history)
                  + ("; artefacts: " + ", ".join(os.path.basename(p) for p in vars(run.paths).values()) if run.paths else "; no artefacts (as the script)"))


if __name__ == "__main__":
    main()
