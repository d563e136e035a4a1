"""Generate tests/golden/mmoetrain.npz by running the REFERENCE implementation (development machine only; no test calls this).

Run as `python tools/gen_golden_mmoetrain.py` from the repository root.  Like oracle/gen_golden.py's `gen_usertrain`, through
oracle/ref_harness.py:

  train cases   the reference's UserModel_MMOE (all-dense, one regression task) with its initial weights scaled up the way
                tests' `_stressed_mmoe` does (the reference initialises the DNN with std 1e-4, where every gradient is round-off),
                compiled with the script's own `loss_taobao`; three optimiser steps through the reference's OWN fit_data
                (shuffle off), then the same statements one by one for the per-step {loss, reg}; both ends must agree bit for bit.
                Cases: (64, 64) at batch 100; (128, 128) at batch 64; (64, 64) at batch 37 with N = 100 (short third batch).
                Inputs: x = 88 Bernoulli(0.15) columns, two uniform(0, 10), a turn counter, 27 actions uniform(-1, 1); y integer
                0..10; exposure gamma(1, 0.5).
  fp64 check    tests/traincase.compare_params lets 0.5 % of a tensor's entries miss its tight bar.  That cap is a condition on the
                inputs: the same three steps run in float64, and the fp32 reference must pass compare_params against its own
                float64 run on every case.  Share of entries inside the tight bar found when this fixture was written: 1.0000 on
                every tensor of every case (largest |difference| 2.9e-7) -- the allowance is not needed by the reference here.
  exposure      a log of ~400 rows in 12 sessions of uneven length (one of length 1), tau in {0.01, 1.0, 0}: the script's
                compute_exposure_effect_virtualTaobao.

Only arrays are written."""
import collections
import copy
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import types  # noqa: E402


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
CASES = [((64, 64), 100, 300), ((128, 128), 64, 192), ((64, 64), 37, 100)]
STEPS = 3


def _script():
    spec = importlib.util.spec_from_file_location("cirs_usermodel_taobao_script", os.path.join(ref_harness.REF_ROOT, "CIRS-UserModel-taobao.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def _build(dnn):
    from core.user_model_mmoe import UserModel_MMOE
    from deepctr_torch.inputs import DenseFeat
    xc = [DenseFeat("user_feat", 91), DenseFeat("feat_item", 27)]
    yc = [DenseFeat("y", 1)]
    tasks = collections.OrderedDict({f.name: "regression" for f in yc})
    model = UserModel_MMOE(xc, yc, 1, tasks, {f.name: f.dimension for f in yc}, dnn_hidden_units=dnn, seed=2022, device="cpu")
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.startswith("dnn.") and name.endswith("weight"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.15)
            elif name.endswith("weight") and "linear_model" in name:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
            elif name.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
        model.tower_network[0].weight.mul_(0.05)
    return model, xc, yc


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
    for ci, (dnn, n, N) in enumerate(CASES):
        model, xc, yc = _build(dnn)
        rng = np.random.RandomState(1)
        user = np.concatenate([(rng.rand(N, 88) < 0.15).astype(float), rng.uniform(0, 10, (N, 2)), rng.randint(1, 30, (N, 1))], 1)
        x = np.concatenate([user, rng.uniform(-1, 1, (N, 27))], 1).astype(np.float32).astype(np.float64)   # fit_data trains on x.float(): stored as fp32
        y = rng.randint(0, 11, (N, 1)).astype(float)
        sc = rng.gamma(1.0, 0.5, (N, 1))
        model.compile(optimizer="adam", loss_func=script.loss_taobao, metrics=None)
        model_b = copy.deepcopy(model)
        model_b.compile(optimizer="adam", loss_func=script.loss_taobao, metrics=None)
        model64 = copy.deepcopy(model).double()
        model64.compile(optimizer="adam", loss_func=script.loss_taobao, metrics=None)
        init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
        ds = StaticDataset(xc, yc, num_workers=0)
        ds.compile_dataset(pd.DataFrame(x), pd.DataFrame(y), sc)
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
        print(f"case {ci} {dnn} n={n} N={N}: losses {losses.tolist()}  tight share vs float64 {share:.4f}, max |diff| {worst:.2e}")
        pre = f"c{ci}_"
        out[pre + "cfg"] = np.array([dnn[0], dnn[1], n, N, STEPS], np.int64)
        out[pre + "x"] = x.astype(np.float32); out[pre + "y"] = y; out[pre + "score"] = sc; out[pre + "losses"] = losses
        for tag, d in (("init", init), ("first", first), ("final", final_a)):
            for k, v in d.items():
                out[pre + tag + "_" + k] = v
    out["n_cases"] = len(CASES)

    # ---- exposure ---------------------------------------------------------------------------------------------------------------
    rng = np.random.RandomState(11)
    lens = [40, 1, 63, 17, 50, 2, 33, 71, 9, 48, 26, 40]
    ts = np.concatenate([np.arange(1, L + 1) for L in lens])
    act = rng.uniform(-1, 1, (len(ts), 27))
    act[5] = act[3]                                              # a repeated action: distance 0
    df = pd.DataFrame(np.concatenate([ts[:, None].astype(float), act], 1), columns=["feat90"] + [f"y{i}" for i in range(27)])
    taus = [0.01, 1.0, 0.0]
    out["expo_timestamp"] = ts.astype(np.int64); out["expo_action"] = act; out["expo_taus"] = np.array(taus)
    for ti, tau in enumerate(taus):
        out[f"expo_out{ti}"] = script.compute_exposure_effect_virtualTaobao(df, tau) if tau > 0 else np.zeros((len(ts), 1))
        print("exposure tau", tau, "max", float(out[f"expo_out{ti}"].max()), "nonzero", int((out[f"expo_out{ti}"] > 0).sum()))
    path = os.path.join(GOLDEN, "mmoetrain.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
