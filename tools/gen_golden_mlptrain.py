"""Generate tests/golden/mlptrain.npz by running the REFERENCE implementation (development machine only; no test calls this).

Run as `python tools/gen_golden_mlptrain.py` from the repository root.  Like tools/gen_golden_mmoetrain.py, through
oracle/ref_harness.py:

  train cases   the reference's UserModel_MMOE (all-dense, the two regression tasks feat_item (27) and y (1) of MLP-taobao.py) with its
                initial weights scaled up the way tests/vtbstaticcase.stress does (the reference initialises the DNN with std 1e-4,
                where every gradient is round-off), compiled with MLP-taobao.py's own `loss_taobao`; three optimiser steps through the
                reference's OWN fit_data (shuffle off), then the same statements one by one for the per-step {loss, reg}; both ends
                must agree bit for bit.
                Cases (dnn, experts x expert_dim, batch, N): (128, 128) 4 x 8 64 192; (96,) 2 x 5 37 100 (short third batch);
                (40, 72, 24) 3 x 6 50 150.
                Inputs: x = 88 Bernoulli(0.15) columns, two integer columns 0..10, a turn counter; y = 27 uniform(-1, 1) columns and
                a click column 0..10 with about 30 % of the rows zeroed (the mask of the action task switches real rows off).
  fp64 check    tests/traincase.compare_params lets 0.5 % of a tensor's entries miss its tight bar.  That cap is a condition on the
                inputs: the same three steps run in float64, the fp32 reference must pass compare_params against its own float64 run
                on every case, and the share of entries inside the tight bar must be at least 0.999 on every tensor.  Found when this
                fixture was written:
                    case 0 (128, 128)    share 1.0000, max |diff| 3.0e-07
                    case 1 (96,)         share 1.0000, max |diff| 3.0e-07
                    case 2 (40, 72, 24)  share 1.0000, max |diff| 2.5e-07

Only arrays are written."""
import collections
import copy
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

import ref_harness  # noqa: E402

ref_harness.install()

import pandas as pd  # noqa: E402
import torch  # noqa: E402

import traincase  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [((128, 128), 4, 8, 64, 192), ((96,), 2, 5, 37, 100), ((40, 72, 24), 3, 6, 50, 150)]   # dnn, experts, expert_dim, batch, N
STEPS = 3


def _script():
    spec = importlib.util.spec_from_file_location("mlp_taobao_script", os.path.join(ref_harness.REF_ROOT, "MLP-taobao.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def _build(dnn, experts, expert_dim):
    from core.user_model_mmoe import UserModel_MMOE
    from deepctr_torch.inputs import DenseFeat
    xc = [DenseFeat("feat_user", 91)]
    yc = [DenseFeat("feat_item", 27), DenseFeat("y", 1)]
    tasks = collections.OrderedDict({f.name: "regression" for f in yc})
    model = UserModel_MMOE(xc, yc, len(tasks), tasks, {f.name: f.dimension for f in yc}, num_experts=experts, expert_dim=expert_dim,
                           dnn_hidden_units=dnn, seed=2022, device="cpu")
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.startswith("dnn.") and name.endswith("weight"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.15)
            elif name.endswith("weight") and "linear_model" in name:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
            elif name.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
        for t in model.tower_network:
            t.weight.mul_(0.05)
    return model, xc, yc


def inputs(N, seed=1):
    """x [N, 91], y [N, 28]: the recipe tests/mlpcase.inputs repeats."""
    rng = np.random.RandomState(seed)
    x = np.concatenate([(rng.rand(N, 88) < 0.15).astype(float), rng.randint(0, 11, (N, 2)).astype(float), rng.randint(1, 30, (N, 1)).astype(float)], 1)
    click = rng.randint(0, 11, (N, 1)).astype(float)
    click[rng.rand(N) < 0.3] = 0.0
    y = np.concatenate([rng.uniform(-1, 1, (N, 27)).astype(np.float32).astype(np.float64), click], 1)   # fit_data trains on y.float(): stored as fp32
    return x, y


def _replay(model, x, y, sc, n, dtype):
    """fit_data's inner-loop statements one by one -> per-step [loss, reg], parameters after the first step and at the end."""
    losses, first = [], None
    for st in range(STEPS):
        xb, yb, sb = (torch.as_tensor(a[st * n:(st + 1) * n]).to(dtype) for a in (x, y, sc))
        loss = model.get_loss(xb, yb, sb).squeeze()
        model.optim.zero_grad()
        reg = model.get_regularization_loss()
        (loss + reg + model.aux_loss).backward()
        model.optim.step()
        losses.append([float(loss.detach()), float(reg.detach())])
        if st == 0:
            first = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    return np.array(losses), first, {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}


def main():
    from core.static_dataset import StaticDataset
    script = _script()
    out = {}
    for ci, (dnn, experts, expert_dim, n, N) in enumerate(CASES):
        model, xc, yc = _build(dnn, experts, expert_dim)
        x, y = inputs(N)
        sc = np.zeros((N, 1))
        model.compile(optimizer="adam", loss_func=script.loss_taobao, metrics=None)
        model_b = copy.deepcopy(model)
        model_b.compile(optimizer="adam", loss_func=script.loss_taobao, metrics=None)
        model64 = copy.deepcopy(model).double()
        model64.compile(optimizer="adam", loss_func=script.loss_taobao, metrics=None)
        init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
        ds = StaticDataset(xc, yc, num_workers=0)
        ds.compile_dataset(pd.DataFrame(x), pd.DataFrame(y))
        model.RL_eval_fun = None
        model.fit_data(ds, dataset_val=None, batch_size=n, epochs=1, shuffle=False, callbacks=[])     # (a) the reference's own loop
        final_a = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
        losses, first, final_b = _replay(model_b, x, y, sc, n, torch.float32)                         # (b) the same statements, step by step
        for k in final_a:
            assert np.array_equal(final_a[k], final_b[k]), k          # the step-by-step replay IS fit_data
        _, first64, final64 = _replay(model64, x, y, sc, n, torch.float64)                            # (c) the condition of compare_params' cap
        traincase.compare_params(first, first64, init, f"case {ci}: fp32 reference vs its float64 run, first step")
        traincase.compare_params(final_a, final64, init, f"case {ci}: fp32 reference vs its float64 run, final")
        share = min(float((np.abs(final_a[k] - final64[k]) <= 2e-6 + 2e-5 * np.abs(final64[k])).mean()) for k in final_a)
        worst = max(float(np.abs(final_a[k] - final64[k]).max()) for k in final_a)
        print(f"case {ci} {dnn} {experts}x{expert_dim} n={n} N={N}: losses {losses.tolist()}  tight share vs float64 {share:.4f}, max |diff| {worst:.2e}")
        assert share >= 0.999, f"case {ci}: the inputs leave the device no room (share {share:.4f})"
        assert (y[:, 27] == 0).mean() > 0.25 and (y[:n, 27] > 0).any()
        pre = f"c{ci}_"
        out[pre + "cfg"] = np.array(list(dnn) + [0] * (3 - len(dnn)) + [len(dnn), experts, expert_dim, n, N, STEPS], np.int64)
        out[pre + "x"] = x.astype(np.float32); out[pre + "y"] = y.astype(np.float32); out[pre + "losses"] = losses
        for tag, d in (("init", init), ("first", first), ("final", final_a)):
            for k, v in d.items():
                out[pre + tag + "_" + k] = v
    out["n_cases"] = len(CASES)
    path = os.path.join(GOLDEN, "mlptrain.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
