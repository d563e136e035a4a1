"""Helpers for the DICE baseline tests: the cases recorded from the reference (tools/gen_golden_usertrain_dice.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_RTOL = 3e-5          # the bar of the debias tests (tests/test_gpu_deepfm_debias.py)
L2 = dict(l2_embedding=1e-5, l2_linear=1e-5, l2_all=0.1)     # UserModel_DICE's defaults with the script's l2_reg_dnn

_cache = {}


def load():
    """-> dict(cases=[...], score=dict(photo, neg, score), forward=dict(x, y)); read once, shared, never modified by a test."""
    if "z" in _cache:
        return _cache["z"]
    z = np.load(os.path.join(GOLDEN, "usertrain_dice.npz"))
    cases = []
    for ci in range(int(z["n_cases"])):
        pre = f"c{ci}_"
        U, I, F, E, n, N, steps = (int(v) for v in z[pre + "cfg"])
        c = dict(U=U, I=I, F=F, E=E, n=n, N=N, steps=steps, x=z[pre + "x"], y=z[pre + "y"], score=z[pre + "score"], losses=z[pre + "losses"])
        for tag in ("init", "first", "final"):
            c[tag] = {k[len(pre + tag + "_"):]: z[k] for k in z.files if k.startswith(pre + tag + "_")}
        cases.append(c)
    out = dict(cases=cases, score=dict(photo=z["s0_photo"], neg=z["s0_neg"], score=z["s0_score"]), forward=dict(x=z["f0_x"], y=z["f0_y"]))
    _cache["z"] = out
    return out


def unused_names(params):
    """The base class's linear_model.* copy: no data gradient, moved by the regulariser alone."""
    return sorted(k for k in params if k.startswith("linear_model."))


def feature_columns(U, I, F, E):
    """The 16 input columns of load_dataset_kuaishou_DICE for the given vocabulary sizes."""
    from core.user_data import dice_feature_columns
    return dice_feature_columns(U, I, F, E, E)


def tight_share(got, want):
    """The smallest share, over the tensors of `want`, of entries inside the tight bar of traincase.compare_params, and the largest |diff|."""
    share = min(float((np.abs(np.asarray(got[k], np.float64).reshape(w.shape) - w) <= 2e-6 + 2e-5 * np.abs(w)).mean()) for k, w in want.items())
    worst = max(float(np.abs(np.asarray(got[k], np.float64).reshape(w.shape) - w).max()) for k, w in want.items())
    return share, worst
