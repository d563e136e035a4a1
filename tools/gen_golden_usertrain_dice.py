"""Generate tests/golden/usertrain_dice.npz by running the REFERENCE implementation (development machine only; no test calls this).

Run as `python tools/gen_golden_usertrain_dice.py` from the repository root.  Built like tools/gen_golden_usertrain_debias.py, through
oracle/ref_harness.py; the script module DICE.py is imported as it is and supplies loss_kuaishou_DICE and
compute_popularity_kuaishouRec, core/user_model_DICE.py supplies UserModel_DICE.

  score case    compute_popularity_kuaishouRec + the sign rule of load_dataset_kuaishou_DICE (DICE.py:175-177) on one small log:
                  240 rows over 40 items drawn from a skewed distribution; the negatives include items that never occur in the log
                  (count 0 -> 1) and rows whose negative is as popular as the positive (ties -> -1), some of them the same item
  forward case  UserModel_DICE.forward of case 0's initial model on 50 seven-column rows [user, photo, feat0..3, duration]
  train cases   UserModel_DICE, its embedding tables scaled up the way gen_golden_usertrain_debias.py does, compiled with the script's
                loss function; three optimiser steps through the reference's OWN fit_data (shuffle off), then the same statements one
                by one for the per-step {loss, reg}; both ends must agree bit for bit.  Cases (U, I, E, batch, N):
                (50, 80, 8, 37, 100), the third batch short and the second batch all score +1 (bpr_int contributes nothing there);
                (40, 60, 16, 48, 144).  The con id columns are drawn independently of the int id columns, ids repeat inside a batch,
                some feat ids are 0, the scores are a mix of +1 and -1.
  fp64 check    tests/traincase.compare_params lets 0.5 % of a tensor's entries miss its tight bar.  That cap is a condition on the
                inputs: the same three steps run in float64, the fp32 reference must pass compare_params against its own float64 run
                on every case, and the share of entries inside the tight bar (tests/dicecase.tight_share) must be at least 0.999 on every tensor, after the first
                step and at the end.  Found when this
                fixture was written:
                    case 0 (50, 80, 8, 37, 100)    first step share 1.0000, max |diff| 6.3e-07; final share 1.0000, max |diff| 2.0e-07
                    case 1 (40, 60, 16, 48, 144)   first step share 0.9998, max |diff| 9.5e-06; final share 0.9998, max |diff| 7.7e-06

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
except ImportError:      # DICE.py imports tqdm
    sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, **kw: it)

import ref_harness  # noqa: E402

ref_harness.install()

import pandas as pd  # noqa: E402
import torch  # noqa: E402

import dicecase  # noqa: E402
import traincase  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TRAIN_CASES = [(50, 80, 8, 37, 100), (40, 60, 16, 48, 144)]
STEPS, F = 3, 32


def _script(name):
    spec = importlib.util.spec_from_file_location(name.replace("-", "_").replace(".", "_"), os.path.join(ref_harness.REF_ROOT, name))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def score_log():
    """(photo of the log [n], photo of the sampled negatives [n]) of the score case."""
    rng = np.random.RandomState(17)
    n, n_items = 240, 40
    photo = np.minimum(rng.zipf(1.4, n) - 1, n_items - 6).astype(np.int64)          # items n_items - 5 .. n_items - 1 never occur
    neg = rng.randint(0, n_items, n).astype(np.int64)
    neg[:6] = [n_items - 1, n_items - 2, n_items - 3, n_items - 1, n_items - 4, n_items - 5]   # absent from the log: count 0 -> 1
    neg[10:20] = photo[10:20]                                                        # ties with the same item
    count = np.bincount(photo, minlength=n_items)
    for i in range(20, 60):                                                          # ties with another item of the same count
        same = np.flatnonzero((count == count[photo[i]]) & (np.arange(n_items) != photo[i]))
        if same.size:
            neg[i] = same[0]
    return photo, neg


def ref_score(script, photo, neg):
    pop_pos, pop_neg = script.compute_popularity_kuaishouRec(pd.DataFrame({"photo_id": photo}), pd.DataFrame({"photo_id": neg}),
                                                             pd.DataFrame({"photo_id": photo}))
    s = (pop_pos > pop_neg).astype(int)
    s[s == 0] = -1
    return s, pop_pos, pop_neg


def _columns(U, I, E):
    from core.inputs import SparseFeatP
    from deepctr_torch.inputs import DenseFeat
    feat = lambda sfx: [SparseFeatP(f"feat{i}{sfx}", F, embedding_dim=E, embedding_name="feat", padding_idx=0) for i in range(4)]  # noqa: E731
    x_columns = [SparseFeatP("user_id_int", U, embedding_dim=E, embedding_name="user_int"),
                 SparseFeatP("user_id_con", U, embedding_dim=E, embedding_name="user_con"),
                 SparseFeatP("photo_id_int", I, embedding_dim=E, embedding_name="photo_int"),
                 SparseFeatP("photo_id_con", I, embedding_dim=E, embedding_name="photo_con")] + feat("") + [DenseFeat("photo_duration", 1)] + \
                [SparseFeatP("photo_id_int_neg", I, embedding_dim=E, embedding_name="photo_int"),
                 SparseFeatP("photo_id_con_neg", I, embedding_dim=E, embedding_name="photo_con")] + feat("_neg") + [DenseFeat("photo_duration_neg", 1)]
    return x_columns, [DenseFeat("y", 1)]


def _build(U, I, E, ci):
    from core.user_model_DICE import UserModel_DICE
    x_columns, y_columns = _columns(U, I, E)
    torch.manual_seed(41 + ci)
    model = UserModel_DICE(x_columns, y_columns, "regression", 1, dnn_hidden_units=(64, 64), seed=2021, l2_reg_dnn=0.1, device="cpu")
    rng = np.random.RandomState(200 + ci)
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
    script = _script("DICE.py")
    loss_fn = script.loss_kuaishou_DICE
    out = {}
    # ---- score case -----------------------------------------------------------------------------------------------------------
    photo, neg = score_log()
    s, pop_pos, pop_neg = ref_score(script, photo, neg)
    out["s0_photo"], out["s0_neg"], out["s0_score"] = photo, neg, s
    absent = int((np.bincount(photo, minlength=int(neg.max()) + 1)[neg] == 0).sum())
    print(f"score case: n={len(photo)} absent negatives {absent}, ties {(pop_pos == pop_neg).sum()}, +1 {(s > 0).sum()} -1 {(s < 0).sum()}")
    assert absent >= 5 and (pop_pos == pop_neg).sum() >= 10 and (s > 0).sum() > 20 and (s < 0).sum() > 20
    # ---- train cases ----------------------------------------------------------------------------------------------------------
    for ci, (U, I, E, n, N) in enumerate(TRAIN_CASES):
        model, xc, yc, rng = _build(U, I, E, ci)

        def col(v):
            return np.asarray(v, np.float64)[:, None]
        feats = lambda: np.where(np.arange(4)[None, :] < rng.randint(1, 5, N)[:, None], rng.randint(1, F, (N, 4)), 0)  # noqa: E731
        ids = lambda V: rng.randint(0, V // 2, N) * 2 % V      # noqa: E731   half the vocabulary: ids repeat inside a batch
        x = np.concatenate([col(ids(U)), col(rng.randint(0, U, N)), col(ids(I)), col(rng.randint(0, I, N)), feats(), col(rng.uniform(2, 60, N)),
                            col(ids(I)), col(rng.randint(0, I, N)), feats(), col(rng.uniform(2, 60, N))], axis=1)
        assert x.shape == (N, 16)
        assert (x[:, 0] != x[:, 1]).mean() > 0.9 and (x[:, 2] != x[:, 3]).mean() > 0.9 and (x[:, 9] != x[:, 10]).mean() > 0.9
        assert (x[:, 4:8] == 0).any() and (x[:, 11:15] == 0).any()
        y = rng.uniform(0, 5, (N, 1))
        sc = np.where(rng.uniform(size=(N, 1)) < 0.5, 1, -1).astype(np.int64)
        if ci == 0:
            sc[n:2 * n] = 1                                     # the second batch: bpr_int contributes nothing
        assert (sc > 0).sum() > N // 4 and (sc < 0).sum() > N // 4
        if ci == 0:     # forward case on the initial model
            fr = np.random.RandomState(7)
            xf = np.concatenate([col(fr.randint(0, U, 50)), col(fr.randint(0, I, 50)),
                                 np.where(np.arange(4)[None, :] < fr.randint(1, 5, 50)[:, None], fr.randint(1, F, (50, 4)), 0),
                                 col(fr.uniform(2, 60, 50))], axis=1)
            with torch.no_grad():
                out["f0_x"], out["f0_y"] = xf, model.forward(torch.as_tensor(xf, dtype=torch.float32)).numpy()
        model.compile(optimizer="adam", loss_func=loss_fn, metric_fun={}, metrics=None)
        model_b = copy.deepcopy(model)
        model_b.compile(optimizer="adam", loss_func=loss_fn, metric_fun={}, metrics=None)
        model64 = copy.deepcopy(model).double()
        model64.compile(optimizer="adam", loss_func=loss_fn, metric_fun={}, metrics=None)
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
        (share1, worst1), (share, worst) = dicecase.tight_share(first, first64), dicecase.tight_share(final_a, final64)
        print(f"case {ci} U={U} I={I} E={E} n={n} N={N}: losses {losses.tolist()}  tight share vs float64: first step {share1:.4f} "
              f"(max |diff| {worst1:.2e}), final {share:.4f} (max |diff| {worst:.2e})")
        assert min(share1, share) >= 0.999, f"case {ci}: the inputs leave the device no room (shares {share1:.4f}, {share:.4f})"
        pre = f"c{ci}_"
        out[pre + "cfg"] = np.array([U, I, F, E, n, N, STEPS], np.int64)
        out[pre + "x"] = x; out[pre + "y"] = y; out[pre + "score"] = sc; out[pre + "losses"] = losses
        for tag, d in (("init", init), ("first", first), ("final", final_a)):
            for k, v in d.items():
                out[pre + tag + "_" + k] = v
    out["n_cases"] = len(TRAIN_CASES)
    path = os.path.join(GOLDEN, "usertrain_dice.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
