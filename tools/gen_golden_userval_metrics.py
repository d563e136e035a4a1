"""Generate tests/golden/userval_metrics.npz by running the REFERENCE implementation (development machine only; no test calls this).

Run as `python tools/gen_golden_userval_metrics.py` from the repository root.  Built like tools/gen_golden_usertrain_dice.py, through
oracle/ref_harness.py: core/user_model_pairwise.py supplies UserModel_Pairwise, core/user_model_DICE.py UserModel_DICE, the script
modules DeepFM-IPS-pairwise.py and DICE.py their loss functions; predict_data / evaluate_data / fit_data are the reference's own
(core/user_model.py:87-248, 351-399).

  cases         UserModel_Pairwise (no alpha/beta) at E = 8 and 16, UserModel_DICE at E = 8 and 16.  Embedding and linear tables scaled
                up the way gen_golden_usertrain_debias.py does; the DNN weights, which the reference draws with std 1e-4, are scaled
                up too, so that both dense layers carry a visible share of the prediction.
  validation    77 rows [user, photo, feat0..3, duration] (no multiple of any tile) holding user id 0 and U - 1, photo id 0 and I - 1,
                feat id 0 (the padding row) and F - 1; y uniform in [0, 5).
  recorded      x, y, the state dict, predict_data(val) and evaluate_data(val) with the scripts' two metric lambdas
                (CIRS-UserModel-kuaishou.py:207-210).
  fit cases     for the pairwise E = 8 case (IPS loss) and the DICE E = 8 case: fit_data(train, val, epochs=2, shuffle=False) on a
                training set of 256 rows, batch 64, with a recording callback -> the logs of epochs -1, 0 and 1.  The learning rate is
                the first of LRS at which `mae` moves by at least 1 % between consecutive records (asserted): a run that validated
                stale weights would miss the recorded values by that much.

Only arrays are written."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _no_network_get(*args, **kwargs):
    raise OSError("network access is disabled in the fixture generator")


# DeepCTR-Torch starts a version check against the package index when it is imported: give it a `requests` that refuses at once
sys.modules["requests"] = types.SimpleNamespace(get=_no_network_get, codes=types.SimpleNamespace(ok=200))
try:
    import tqdm  # noqa: F401
except ImportError:
    sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, **kw: it)

import ref_harness  # noqa: E402

ref_harness.install()

import pandas as pd  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [("pairwise", 50, 80, 8), ("pairwise", 40, 60, 16), ("dice", 50, 80, 8), ("dice", 40, 60, 16)]   # (model, U, I, E)
FIT_CASES = (0, 2)
F, N_VAL, N_TRAIN, BATCH, EPOCHS = 32, 77, 256, 64, 2
LRS = (1e-3, 2e-3, 5e-3, 1e-2, 2e-2)
METRICS = {"mae": lambda y, y_predict: nn.functional.l1_loss(torch.from_numpy(y), torch.from_numpy(y_predict)).numpy(),
           "mse": lambda y, y_predict: nn.functional.mse_loss(torch.from_numpy(y), torch.from_numpy(y_predict)).numpy()}


def _script(name):
    spec = importlib.util.spec_from_file_location(name.replace("-", "_").replace(".", "_"), os.path.join(ref_harness.REF_ROOT, name))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def _columns(kind, U, I, E):
    from core.inputs import SparseFeatP
    from deepctr_torch.inputs import DenseFeat
    feat = lambda sfx: [SparseFeatP(f"feat{i}{sfx}", F, embedding_dim=E, embedding_name="feat", padding_idx=0) for i in range(4)]  # noqa: E731
    if kind == "pairwise":
        xc = [SparseFeatP("user_id", U, embedding_dim=E), SparseFeatP("photo_id", I, embedding_dim=E)] + feat("") + [DenseFeat("photo_duration", 1)]
    else:
        xc = [SparseFeatP("user_id_int", U, embedding_dim=E, embedding_name="user_int"),
              SparseFeatP("user_id_con", U, embedding_dim=E, embedding_name="user_con"),
              SparseFeatP("photo_id_int", I, embedding_dim=E, embedding_name="photo_int"),
              SparseFeatP("photo_id_con", I, embedding_dim=E, embedding_name="photo_con")] + feat("") + [DenseFeat("photo_duration", 1)] + \
             [SparseFeatP("photo_id_int_neg", I, embedding_dim=E, embedding_name="photo_int"),
              SparseFeatP("photo_id_con_neg", I, embedding_dim=E, embedding_name="photo_con")] + feat("_neg") + [DenseFeat("photo_duration_neg", 1)]
    return xc, [DenseFeat("y", 1)]


def _build(kind, U, I, E, ci):
    from core.user_model_DICE import UserModel_DICE
    from core.user_model_pairwise import UserModel_Pairwise
    xc, yc = _columns(kind, U, I, E)
    torch.manual_seed(61 + ci)
    cls = UserModel_Pairwise if kind == "pairwise" else UserModel_DICE
    model = cls(xc, yc, "regression", 1, dnn_hidden_units=(64, 64), seed=2021, l2_reg_dnn=0.1, device="cpu")
    rng = np.random.RandomState(300 + ci)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if "embedding_dict" in name:
                prm.copy_(torch.as_tensor(rng.normal(0, 0.3, prm.shape).astype(np.float32)))
                if name == "embedding_dict.feat.weight":
                    prm[0] = 0
            elif name.startswith("dnn") or name.startswith("last"):
                std = 0.05 if name.endswith("bias") else (0.12 if "linears.0" in name else 0.2)
                prm.copy_(torch.as_tensor(rng.normal(0, std, prm.shape).astype(np.float32)))
    return model, xc, yc, rng


def _rows(rng, U, I, n):
    """n seven-column rows [user, photo, feat0..3, duration]; the first rows hold the corners of every id range."""
    feats = np.where(np.arange(4)[None, :] < rng.randint(1, 5, n)[:, None], rng.randint(1, F, (n, 4)), 0)
    u, p = rng.randint(0, U, n), rng.randint(0, I, n)
    u[:4] = [0, U - 1, 0, U - 1]
    p[:4] = [0, I - 1, I - 1, 0]
    feats[0] = [F - 1, 0, 0, 0]
    feats[1] = [1, F - 1, 2, F - 1]
    return u, p, feats, rng.uniform(2, 60, n)


def _col(v):
    return np.asarray(v, np.float64)[:, None]


def _train_set(kind, rng, U, I, xc, yc, ips_script):
    from core.static_dataset import StaticDataset
    n = N_TRAIN
    u, p, feats, dur = _rows(rng, U, I, n)
    un, pn, featsn, durn = _rows(rng, U, I, n)
    if kind == "pairwise":
        x = np.concatenate([_col(u), _col(p), feats, _col(dur), _col(u), _col(pn), featsn, _col(durn)], axis=1)
        df = pd.DataFrame({"photo_id": p})
        sc = ips_script.compute_IPS_kuaishouRec(df, df)
    else:
        x = np.concatenate([_col(u), _col(u), _col(p), _col(p), feats, _col(dur), _col(pn), _col(pn), featsn, _col(durn)], axis=1)
        sc = np.where(rng.uniform(size=(n, 1)) < 0.5, 1, -1).astype(np.int64)
    y = rng.uniform(0, 5, (n, 1))
    ds = StaticDataset(xc, yc, num_workers=0)
    ds.compile_dataset(pd.DataFrame(x), pd.DataFrame(y), sc)
    return ds, x, y, np.asarray(sc, np.float64)


class _Record:
    def __init__(self): self.logs = []
    def on_train_begin(self): pass
    def on_train_end(self): pass
    def on_epoch_begin(self, epoch): pass
    def on_epoch_end(self, epoch, logs): self.logs.append((epoch, dict(logs)))


def main():
    from core.static_dataset import StaticDataset
    ips_script, dice_script = _script("DeepFM-IPS-pairwise.py"), _script("DICE.py")
    loss_of = {"pairwise": ips_script.loss_kuaishou_IPS_pairwise, "dice": dice_script.loss_kuaishou_DICE}
    out = {}
    for ci, (kind, U, I, E) in enumerate(CASES):
        model, xc, yc, rng = _build(kind, U, I, E, ci)
        u, p, feats, dur = _rows(rng, U, I, N_VAL)
        x = np.concatenate([_col(u), _col(p), feats, _col(dur)], axis=1)
        y = rng.uniform(0, 5, (N_VAL, 1))
        assert x.shape == (N_VAL, 7) and {0, U - 1} <= set(u) and {0, I - 1} <= set(p) and {0, F - 1} <= set(feats.ravel())
        val = StaticDataset(xc[:7] if kind == "pairwise" else xc[:9], yc, num_workers=0)
        val.compile_dataset(pd.DataFrame(x), pd.DataFrame(y))
        model.compile(optimizer="adam", loss_func=loss_of[kind], metric_fun=METRICS, metrics=None)
        model.RL_eval_fun = None
        init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
        pred = model.predict_data(val, 32)
        ev = model.evaluate_data(val, 32)
        assert pred.shape == (N_VAL, 1) and pred.dtype == np.float64
        pre = f"c{ci}_"
        out[pre + "cfg"] = np.array([U, I, F, E, 0 if kind == "pairwise" else 1], np.int64)
        out[pre + "x"], out[pre + "y"], out[pre + "pred"] = x, y, pred
        out[pre + "eval"] = np.array([ev["mae"], ev["mse"]], np.float64)
        for k, v in init.items():
            out[pre + "sd_" + k] = v
        print(f"case {ci} {kind} U={U} I={I} E={E}: pred in [{pred.min():.3f}, {pred.max():.3f}] std {pred.std():.3f}  mae {ev['mae']:.6f} mse {ev['mse']:.6f}")
        if ci not in FIT_CASES:
            continue
        train, xt, yt, sct = _train_set(kind, rng, U, I, xc, yc, ips_script)
        chosen = None
        for lr in LRS:
            m = type(model)(xc, yc, "regression", 1, dnn_hidden_units=(64, 64), seed=2021, l2_reg_dnn=0.1, device="cpu")
            m.load_state_dict({k: torch.as_tensor(v) for k, v in init.items()})
            m.compile(optimizer=torch.optim.Adam(m.parameters(), lr=lr), loss_func=loss_of[kind], metric_fun=METRICS, metrics=None)
            m.RL_eval_fun = None
            rec = _Record()
            m.fit_data(train, val, batch_size=BATCH, epochs=EPOCHS, shuffle=False, callbacks=[rec])
            mae = [lg["mae"] for _, lg in rec.logs]
            moves = [abs(b - a) / a for a, b in zip(mae, mae[1:])]
            print(f"  fit lr={lr}: epochs {[e for e, _ in rec.logs]} mae {mae} relative moves {moves}")
            if min(moves) >= 0.01:
                chosen = (lr, rec)
                break
        assert chosen is not None, "no learning rate of LRS moves mae by 1 % per epoch"
        lr, rec = chosen
        assert [e for e, _ in rec.logs] == [-1, 0, 1] and list(rec.logs[1][1]) == ["loss", "mae", "mse"] and list(rec.logs[0][1]) == ["mae", "mse"]
        out[pre + "fit_x"], out[pre + "fit_y"], out[pre + "fit_score"] = xt, yt, sct
        out[pre + "fit_lr"] = np.float64(lr)
        out[pre + "fit_logs"] = np.array([[lg.get("loss", np.nan), lg["mae"], lg["mse"]] for _, lg in rec.logs], np.float64)   # rows: epochs -1, 0, 1
    out["n_cases"] = len(CASES)
    out["fit_cases"] = np.array(FIT_CASES, np.int64)
    out["fit_shape"] = np.array([N_TRAIN, BATCH, EPOCHS], np.int64)
    path = os.path.join(GOLDEN, "userval_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
