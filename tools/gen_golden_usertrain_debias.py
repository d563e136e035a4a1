"""Generate tests/golden/usertrain_debias.npz by running the REFERENCE implementation (development machine only; no test calls this).

Run as `python tools/gen_golden_usertrain_debias.py` from the repository root.  Like tools/gen_golden_mlptrain.py, through
oracle/ref_harness.py; the two script modules DeepFM-IPS-pairwise.py and PD-pairwise.py are imported as they are and supply the loss
functions and the score functions.

  score cases   compute_IPS_kuaishouRec and compute_popularity_kuaishouRec_pairwise (gamma 0.1 and 0.5, 5 bins) on three small logs:
                  s0  300 rows, 70 items, span 5000 s (interval exactly 1000): rows exactly on the interior bounds 1000 .. 4000, the row
                      at time_max, items drawn from a skewed distribution (repeats; most items absent from some bins)
                  s1  257 rows, 45 items, span 4999.7 s: rows placed on the bounds as the reference computes them
                      (`interval * i + time_min`), the row at time_max
                  s2  64 rows, 20 items, every timestamp equal (interval 0: the closed last bin takes every row)
  train cases   the reference's UserModel_Pairwise with ab_columns=None, its embedding tables scaled up the way oracle/gen_golden.py's
                gen_usertrain does, compiled with the loss function of the script itself; three optimiser steps through the reference's
                OWN fit_data (shuffle off), then the same statements one by one for the per-step {loss, reg}; both ends must agree bit
                for bit.  Cases (loss, U, I, E, batch, N): ips 50 80 8 37 100 (third batch short); ips 40 60 16 48 144;
                pd 50 80 8 37 100; pd 30 50 16 16 48.  The score column comes from the script's own score function over the case's
                positive item column (and timestamps drawn over 5000 s, gamma 0.1, for pd): IPS weights 1/1 .. 1/4 and the like.
  fp64 check    tests/traincase.compare_params lets 0.5 % of a tensor's entries miss its tight bar.  That cap is a condition on the
                inputs: the same three steps run in float64, the fp32 reference must pass compare_params against its own float64 run
                on every case, and the share of entries inside the tight bar must be at least 0.999 on every tensor.  Found when this
                fixture was written:
                    case 0 ips (50, 80, 8, 37, 100)    share 1.0000, max |diff| 8.2e-08
                    case 1 ips (40, 60, 16, 48, 144)   share 1.0000, max |diff| 6.6e-08
                    case 2 pd  (50, 80, 8, 37, 100)    share 1.0000, max |diff| 6.6e-08
                    case 3 pd  (30, 50, 16, 16, 48)    share 1.0000, max |diff| 6.6e-08

Only arrays are written."""
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
try:
    import tqdm  # noqa: F401
except ImportError:      # PD-pairwise.py wraps its bin loop in tqdm.tqdm
    sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, **kw: it)

import ref_harness  # noqa: E402

ref_harness.install()

import pandas as pd  # noqa: E402
import torch  # noqa: E402

import traincase  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TRAIN_CASES = [("ips", 50, 80, 8, 37, 100), ("ips", 40, 60, 16, 48, 144), ("pd", 50, 80, 8, 37, 100), ("pd", 30, 50, 16, 16, 48)]
KIND_ID = {"ips": 1, "pd": 2}
STEPS, F, NUM_BIN, T0 = 3, 32, 5, 1.6e9
GAMMAS = (0.1, 0.5)
TRAIN_GAMMA = 0.1


def _script(name):
    spec = importlib.util.spec_from_file_location(name.replace("-", "_").replace(".", "_"), os.path.join(ref_harness.REF_ROOT, name))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def score_logs():
    """[(photo [n] int64, timestamp [n] float64)] of the three score cases."""
    logs = []
    rng = np.random.RandomState(11)
    n, n_items = 300, 70
    photo = np.minimum(rng.zipf(1.4, n) - 1, n_items - 1).astype(np.int64)
    ts = T0 + rng.randint(1, 5000, n).astype(np.float64)
    ts[0], ts[-1] = T0, T0 + 5000.0
    for k, i in enumerate([7, 8, 50, 120, 121, 200, 250, 251]):      # exactly on the interior bounds
        ts[i] = T0 + 1000.0 * (1 + k % 4)
    logs.append((photo, ts))
    n, n_items = 257, 45
    photo = np.minimum(rng.zipf(1.3, n) - 1, n_items - 1).astype(np.int64)
    photo[5] = n_items - 1
    ts = T0 + 0.3 + np.round(rng.uniform(0.0, 4999.7, n), 1)
    ts[3], ts[100] = T0 + 0.3, T0 + 0.3 + 4999.7
    time_min, time_max = ts.min(), ts.max()
    interval = (time_max - time_min) / NUM_BIN
    for k, i in enumerate([10, 11, 60, 130, 131, 201, 240, 256]):    # on the bounds as the reference computes them
        ts[i] = interval * (1 + k % 4) + time_min
    assert ts.min() == time_min and ts.max() == time_max
    logs.append((photo, ts))
    logs.append((rng.randint(0, 20, 64).astype(np.int64), np.full(64, T0 + 17.0)))
    return logs


def ref_scores(ips_script, pd_script, photo, ts, gamma):
    df = pd.DataFrame({"photo_id": photo})
    ips = ips_script.compute_IPS_kuaishouRec(df, df) if gamma is None else None
    pop = None if gamma is None else pd_script.compute_popularity_kuaishouRec_pairwise(df, df, pd.Series(ts), gamma, num_bin=NUM_BIN)
    return ips if gamma is None else pop


def _build(U, I, E, ci):
    from core.inputs import SparseFeatP
    from core.user_model_pairwise import UserModel_Pairwise
    from deepctr_torch.inputs import DenseFeat
    x_columns = [SparseFeatP("user_id", U, embedding_dim=E), SparseFeatP("photo_id", I, embedding_dim=E)] + \
                [SparseFeatP(f"feat{i}", F, embedding_dim=E, embedding_name="feat", padding_idx=0) for i in range(4)] + [DenseFeat("photo_duration", 1)]
    y_columns = [DenseFeat("y", 1)]
    torch.manual_seed(31 + ci)
    model = UserModel_Pairwise(x_columns, y_columns, "regression", 1, dnn_hidden_units=(64, 64), seed=2021, l2_reg_dnn=0.1, device="cpu")
    rng = np.random.RandomState(100 + ci)
    with torch.no_grad():     # the reference initialises embeddings with std 1e-4: scale up so every term of the loss matters
        for name, prm in model.named_parameters():
            if "embedding_dict" in name:
                prm.copy_(torch.as_tensor(rng.normal(0, 0.3, prm.shape).astype(np.float32)))
                if name == "embedding_dict.feat.weight":
                    prm[0] = 0
    return model, x_columns, y_columns, rng


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
    ips_script, pd_script = _script("DeepFM-IPS-pairwise.py"), _script("PD-pairwise.py")
    loss_of = {"ips": ips_script.loss_kuaishou_IPS_pairwise, "pd": pd_script.loss_kuaishou_PD_pairwise}
    out = {}
    # ---- score cases ----------------------------------------------------------------------------------------------------------
    for si, (photo, ts) in enumerate(score_logs()):
        pre = f"s{si}_"
        out[pre + "photo"], out[pre + "timestamp"] = photo, ts
        out[pre + "ips"] = ref_scores(ips_script, pd_script, photo, ts, None)
        for gi, gamma in enumerate(GAMMAS):
            out[pre + f"pd{gi}"] = ref_scores(ips_script, pd_script, photo, ts, gamma)
        print(f"score case {si}: n={len(photo)} items={photo.max() + 1} ips values {np.unique(out[pre + 'ips']).size}, "
              f"pd zeros {(out[pre + 'pd0'] == 0).sum()}")
    out["n_score_cases"] = 3
    out["gammas"] = np.array(GAMMAS)
    out["num_bin"] = NUM_BIN
    # ---- train cases ----------------------------------------------------------------------------------------------------------
    for ci, (kind, U, I, E, n, N) in enumerate(TRAIN_CASES):
        model, xc, yc, rng = _build(U, I, E, ci)

        def col(v):
            return np.asarray(v, np.float64)[:, None]
        feats = lambda: np.where(np.arange(4)[None, :] < rng.randint(1, 5, N)[:, None], rng.randint(1, F, (N, 4)), 0)  # noqa: E731
        u = rng.randint(0, U, N)
        pos = rng.randint(0, I, N)
        x = np.concatenate([col(u), col(pos), feats(), col(rng.uniform(2, 60, N)), col(u), col(rng.randint(0, I, N)), feats(),
                            col(rng.uniform(2, 60, N))], axis=1)
        y = rng.uniform(0, 5, (N, 1))
        ts = T0 + rng.randint(0, 5000, N).astype(np.float64)
        sc = ref_scores(ips_script, pd_script, pos, ts, None if kind == "ips" else TRAIN_GAMMA)
        assert sc.shape == (N, 1) and (sc > 0).all()
        model.compile(optimizer="adam", loss_func=loss_of[kind], metric_fun={}, metrics=None)
        model_b = copy.deepcopy(model)
        model_b.compile(optimizer="adam", loss_func=loss_of[kind], metric_fun={}, metrics=None)
        model64 = copy.deepcopy(model).double()
        model64.compile(optimizer="adam", loss_func=loss_of[kind], metric_fun={}, metrics=None)
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
        print(f"case {ci} {kind} U={U} I={I} E={E} n={n} N={N}: losses {losses.tolist()}  tight share vs float64 {share:.4f}, max |diff| {worst:.2e}, "
              f"score values {np.unique(sc).size} in [{sc.min():.4f}, {sc.max():.4f}]")
        assert share >= 0.999, f"case {ci}: the inputs leave the device no room (share {share:.4f})"
        pre = f"c{ci}_"
        out[pre + "cfg"] = np.array([U, I, F, E, n, N, STEPS, KIND_ID[kind]], np.int64)
        out[pre + "x"] = x; out[pre + "y"] = y; out[pre + "score"] = sc; out[pre + "timestamp"] = ts; out[pre + "losses"] = losses
        for tag, d in (("init", init), ("first", first), ("final", final_a)):
            for k, v in d.items():
                out[pre + tag + "_" + k] = v
    out["n_cases"] = len(TRAIN_CASES)
    out["train_gamma"] = TRAIN_GAMMA
    path = os.path.join(GOLDEN, "usertrain_debias.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
