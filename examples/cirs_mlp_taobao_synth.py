"""The static baselines' run (reference MLP-taobao.py / MLP-epsilonGreedy-taobao.py) on a device-written log: a VirtualTaobao log from
the device env under random actions -> the two-task UserModel_MMOE trained on the device (cirs_mlp_train_epoch), evaluated after every
epoch by test_taobao on the device (cirs_vtb_static_eval).  `dataset.txt` of the reference is not shipped; the log has its format.

    python examples/cirs_mlp_taobao_synth.py [--sessions 2000] [--epoch 5] [--epsilon 0.0] [--dnn 256 256]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=2000)
    ap.add_argument("--epoch", type=int, default=5)
    ap.add_argument("--batch_size", type=int, default=100)
    ap.add_argument("--epsilon", type=float, default=0.0)
    ap.add_argument("--dnn", type=int, nargs="+", default=(256, 256))
    args = ap.parse_args()
    from cirs_hip.synthetic import write_virtualtaobao_log
    from core.user_model_train import train_mlp_taobao
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "dataset.txt")
        rows = write_virtualtaobao_log(log, args.sessions, seed=0)
        print(f"{rows} log rows in {args.sessions} sessions")
        res = train_mlp_taobao(log, save_root=tmp, epsilon=args.epsilon, dnn=tuple(args.dnn), epoch=args.epoch, batch_size=args.batch_size)
    for e, h in enumerate(res.history):
        print(f"epoch {e}: " + ", ".join(f"{k} {v:.4f}" for k, v in h.items()))


if __name__ == "__main__":
    main()
