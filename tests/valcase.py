"""Shared pieces of the validation-pass tests (tests/golden/userval_metrics.npz, tools/gen_golden_userval_metrics.py): the recorded
cases, the public models built from the recorded state dicts, random weights for the kernel-against-kernel checks."""
import os

import numpy as np
import torch

F = 32


def load(golden_dir):
    z = np.load(os.path.join(golden_dir, "userval_metrics.npz"))
    cases = []
    for ci in range(int(z["n_cases"])):
        pre = f"c{ci}_"
        U, I, Fv, E, kind = (int(v) for v in z[pre + "cfg"])
        c = dict(U=U, I=I, F=Fv, E=E, kind="dice" if kind else "pairwise", x=z[pre + "x"], y=z[pre + "y"], pred=z[pre + "pred"],
                 eval={"mae": float(z[pre + "eval"][0]), "mse": float(z[pre + "eval"][1])},
                 sd={k[len(pre) + 3:]: z[k] for k in z.files if k.startswith(pre + "sd_")})
        if ci in z["fit_cases"]:
            c["fit"] = dict(x=z[pre + "fit_x"], y=z[pre + "fit_y"], score=z[pre + "fit_score"], lr=float(z[pre + "fit_lr"]), logs=z[pre + "fit_logs"],
                            batch=int(z["fit_shape"][1]), epochs=int(z["fit_shape"][2]))
        cases.append(c)
    return cases


def columns(kind, U, I, E, Fv=F):
    from core.inputs import SparseFeatP
    from deepctr_torch.inputs import DenseFeat
    feat = lambda sfx: [SparseFeatP(f"feat{i}{sfx}", Fv, embedding_dim=E, embedding_name="feat", padding_idx=0) for i in range(4)]  # noqa: E731
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


def build_model(c, sd=None, metric_fun=None, lr=1e-3):
    """The public model of case c with the state dict sd (default: the recorded one), compiled with the case's loss."""
    from core.user_model_DICE import UserModel_DICE, loss_kuaishou_DICE
    from core.user_model_pairwise import UserModel_Pairwise, loss_kuaishou_IPS_pairwise
    xc, yc = columns(c["kind"], c["U"], c["I"], c["E"], c["F"])
    cls, loss = (UserModel_Pairwise, loss_kuaishou_IPS_pairwise) if c["kind"] == "pairwise" else (UserModel_DICE, loss_kuaishou_DICE)
    model = cls(xc, yc, "regression", 1, dnn_hidden_units=(64, 64), seed=2021, l2_reg_dnn=0.1, device="cpu")
    model.load_state_dict({k: torch.as_tensor(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in (sd or c["sd"]).items()})
    model.compile(torch.optim.Adam(model.parameters(), lr=lr), loss_func=loss, metric_fun=metric_fun)
    return model, xc, yc


def dataset(xc, yc, x, y, score=None):
    from core.static_dataset import StaticDataset
    ds = StaticDataset(xc, yc, num_workers=0)
    ds.compile_dataset(np.asarray(x), np.asarray(y), score)
    return ds


def random_state_dict(kind, U, I, E, seed, Fv=F):
    """Weights of order one in every tensor the forward reads, under the reference's state_dict names."""
    rng = np.random.RandomState(seed)
    n = lambda *s, std=0.3: rng.normal(0, std, s).astype(np.float32)     # noqa: E731
    if kind == "pairwise":
        sd = {"embedding_dict.user_id.weight": n(U, E), "embedding_dict.photo_id.weight": n(I, E), "embedding_dict.feat.weight": n(Fv, E),
              "linear.embedding_dict.user_id.weight": n(U, 1), "linear.embedding_dict.photo_id.weight": n(I, 1),
              "linear.embedding_dict.feat.weight": n(Fv, 1), "linear.weight": n(1, 1, std=0.02),
              "dnn.linears.0.weight": n(64, 6 * E + 1, std=0.1), "dnn.linears.0.bias": n(64, std=0.1), "dnn.linears.1.weight": n(64, 64, std=0.15),
              "dnn.linears.1.bias": n(64, std=0.1), "last.weight": n(1, 64), "out.bias": n(1, 1)}
        sd["embedding_dict.feat.weight"][0] = 0
        sd["dnn.linears.0.weight"][:, -1] *= 0.05      # the duration column: durations reach 60
        return sd
    from cirs_hip.dice_train import layout
    sd = {}
    for name, shape in layout(U, I, Fv, E):
        std = 0.1 if "linears.0.weight" in name else (0.15 if "linears.1.weight" in name else (0.02 if name == "linear_main.weight" else 0.3))
        sd[name] = n(*shape, std=std)
    sd["embedding_dict.feat.weight"][0] = 0
    sd["dnn_main.linears.0.weight"][:, -1] *= 0.05
    return sd


def random_rows(U, I, n, seed, same=False, Fv=F):
    """x [n,7], y [n,1]; same: every row a copy of the first."""
    rng = np.random.RandomState(seed)
    feats = np.where(np.arange(4)[None, :] < rng.randint(1, 5, n)[:, None], rng.randint(1, Fv, (n, 4)), 0)
    x = np.concatenate([rng.randint(0, U, (n, 1)), rng.randint(0, I, (n, 1)), feats, rng.uniform(2, 60, (n, 1))], axis=1).astype(np.float64)
    y = rng.uniform(0, 5, (n, 1))
    if same:
        x[:] = x[0]
    return x, y
