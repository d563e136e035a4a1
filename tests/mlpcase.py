"""Helpers for the tests of the static baselines' training (csrc/mlp_train.hip): the recorded cases of tests/golden/mlptrain.npz (the
reference's own fit_data, tools/gen_golden_mlptrain.py) and synthetic inputs of the same kind."""
import os

import numpy as np

L2_LINEAR, L2_ALL = 1e-5, 1e-2      # UserModel's l2_reg_linear default, UserModel_MMOE's l2_reg_dnn default
CASES = [((128, 128), 4, 8, 64, 192), ((96,), 2, 5, 37, 100), ((40, 72, 24), 3, 6, 50, 150)]   # dnn, experts, expert_dim, batch, N

# ---- the device cases of tests/test_gpu_mlp_train.py against the torch restatement (tests/test_mlp_train_cpu.py checks the inputs of
# the first on the CPU): dnn, experts, expert_dim, batch, every click zero
GPU_STEPS = 8
GPU_CASES = {"script": ((256, 256), 4, 8, 100, False), "short": ((256, 256), 4, 8, 5, False), "tiny": ((5, 3), 2, 3, 37, False),
             "noclick": ((96,), 2, 5, 16, True)}


def load(golden_dir):
    z = np.load(os.path.join(golden_dir, "mlptrain.npz"))
    cases = []
    for ci in range(int(z["n_cases"])):
        pre = f"c{ci}_"
        cfg = [int(v) for v in z[pre + "cfg"]]
        n_dnn, experts, expert_dim, n, N, steps = cfg[3:]
        c = dict(dnn=tuple(cfg[:n_dnn]), experts=experts, expert_dim=expert_dim, n=n, N=N, steps=steps, x=z[pre + "x"].astype(np.float64),
                 y=z[pre + "y"].astype(np.float64), losses=z[pre + "losses"])
        for tag in ("init", "first", "final"):
            c[tag] = {k[len(pre + tag + "_"):]: z[k] for k in z.files if k.startswith(pre + tag + "_")}
        cases.append(c)
    return cases


def dnn_scale(dnn):
    """Standard deviation of the stressed hidden-layer weights: 0.15 up to width 64, shrinking with the square root of the width above
    (at 0.15 a 256-wide layer doubles the activations' scale per layer and the loss's round-off with it)."""
    return 0.15 * min(1.0, (64.0 / max(dnn)) ** 0.5)


def stressed_init(dnn, experts=4, expert_dim=8, seed=3, scale=None):
    """Initial weights at the scales of the recorded cases (the reference's own std 1e-4 leaves every gradient at round-off)."""
    import torch
    import vtbstaticcase
    m = vtbstaticcase.two_task_model(dnn, experts, expert_dim, stressed=True, seed=seed)
    if scale is not None:
        g = torch.Generator().manual_seed(seed + 100)
        with torch.no_grad():
            for lin in m.dnn.linears:
                lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * scale)
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def inputs(N, seed=1, no_click=False):
    """x [N, 91] (88 Bernoulli(0.15) columns, two integer columns 0..10, a turn counter), y [N, 28] (27 uniform(-1, 1) columns and a click
    column 0..10 with about 30 % of the rows zeroed): the kind of input the recorded cases use."""
    rng = np.random.RandomState(seed)
    x = np.concatenate([(rng.rand(N, 88) < 0.15).astype(float), rng.randint(0, 11, (N, 2)).astype(float), rng.randint(1, 30, (N, 1)).astype(float)], 1)
    click = rng.randint(0, 11, (N, 1)).astype(float)
    click[rng.rand(N) < 0.3] = 0.0
    if no_click:
        click[:] = 0.0
    y = np.concatenate([rng.uniform(-1, 1, (N, 27)).astype(np.float32).astype(np.float64), click], 1)
    return x, y


def gpu_case(name):
    """-> (init, x, y, batch) of a GPU_CASES entry: GPU_STEPS batches of fresh rows."""
    dnn, experts, expert_dim, batch, no_click = GPU_CASES[name]
    init = stressed_init(dnn, experts, expert_dim, scale=dnn_scale(dnn) if max(dnn) > 128 else None)
    x, y = inputs(batch * GPU_STEPS, seed=7, no_click=no_click)
    return init, x, y, batch


def tight_share(got, want):
    return min(float((np.abs(np.asarray(got[k], np.float64).reshape(w.shape) - w) <= 2e-6 + 2e-5 * np.abs(w)).mean()) for k, w in want.items())
