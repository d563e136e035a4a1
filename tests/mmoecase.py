"""Helpers for the VirtualTaobao user-model training tests: the recorded cases of tests/golden/mmoetrain.npz (the reference's own
fit_data, tools/gen_golden_mmoetrain.py) and synthetic inputs of the same kind."""
import collections
import os

import numpy as np

L2_LINEAR, L2_ALL = 1e-5, 1e-2      # UserModel's l2_reg_linear default, UserModel_MMOE's l2_reg_dnn default


def load(golden_dir):
    z = np.load(os.path.join(golden_dir, "mmoetrain.npz"))
    cases = []
    for ci in range(int(z["n_cases"])):
        pre = f"c{ci}_"
        h1, h2, n, N, steps = (int(v) for v in z[pre + "cfg"])
        c = dict(dnn=(h1, h2), n=n, N=N, steps=steps, x=z[pre + "x"].astype(np.float64), y=z[pre + "y"], score=z[pre + "score"],
                 losses=z[pre + "losses"])
        for tag in ("init", "first", "final"):
            c[tag] = {k[len(pre + tag + "_"):]: z[k] for k in z.files if k.startswith(pre + tag + "_")}
        cases.append(c)
    expo = dict(timestamp=z["expo_timestamp"], action=z["expo_action"], taus=z["expo_taus"],
                out=[z[f"expo_out{i}"] for i in range(len(z["expo_taus"]))])
    return cases, expo


def columns():
    from deepctr_torch.inputs import DenseFeat
    return [DenseFeat("user_feat", 91), DenseFeat("feat_item", 27)], [DenseFeat("y", 1)]


def model(dnn, seed=2022):
    from core.user_model_mmoe import UserModel_MMOE
    xc, yc = columns()
    tasks = collections.OrderedDict({f.name: "regression" for f in yc})
    return UserModel_MMOE(xc, yc, len(tasks), tasks, {f.name: f.dimension for f in yc}, dnn_hidden_units=dnn, seed=seed, device="cpu")


def stressed_init(dnn, seed=3):
    """Initial weights at the scales of the recorded cases (the reference's own std 1e-4 leaves every gradient at round-off)."""
    import torch
    m = model(dnn)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("dnn.") and name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.15)
            elif name.endswith("weight") and "linear_model" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        m.tower_network[0].weight.mul_(0.05)
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def inputs(N, seed=1):
    """x [N, 118] (88 Bernoulli(0.15) columns, two uniform(0, 10), a turn counter, 27 actions uniform(-1, 1)), y integer 0..10,
    exposure gamma(1, 0.5): the kind of input the recorded cases use."""
    rng = np.random.RandomState(seed)
    user = np.concatenate([(rng.rand(N, 88) < 0.15).astype(float), rng.uniform(0, 10, (N, 2)), rng.randint(1, 30, (N, 1))], 1)
    x = np.concatenate([user, rng.uniform(-1, 1, (N, 27))], 1).astype(np.float32).astype(np.float64)
    return x, rng.randint(0, 11, (N, 1)).astype(float), rng.gamma(1.0, 0.5, (N, 1))
