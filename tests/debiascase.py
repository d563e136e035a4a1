"""Helpers for the tests of the two debiasing baselines: the cases of tests/golden/usertrain_debias.npz (recorded from the reference's
fit_data and score functions by tools/gen_golden_usertrain_debias.py)."""
import os

import numpy as np

KIND_NAME = {0: "pairwise", 1: "ips", 2: "pd"}


def load_train(golden_dir):
    z = np.load(os.path.join(golden_dir, "usertrain_debias.npz"))
    cases = []
    for ci in range(int(z["n_cases"])):
        pre = f"c{ci}_"
        U, I, F, E, n, N, steps, kind = (int(v) for v in z[pre + "cfg"])
        c = dict(U=U, I=I, F=F, E=E, n=n, N=N, steps=steps, kind=KIND_NAME[kind], x=z[pre + "x"], y=z[pre + "y"], score=z[pre + "score"],
                 losses=z[pre + "losses"])
        for tag in ("init", "first", "final"):
            c[tag] = {k[len(pre + tag + "_"):]: z[k] for k in z.files if k.startswith(pre + tag + "_")}
        cases.append(c)
    return cases


def load_scores(golden_dir):
    z = np.load(os.path.join(golden_dir, "usertrain_debias.npz"))
    gammas = [float(g) for g in z["gammas"]]
    return [dict(photo=z[f"s{si}_photo"], timestamp=z[f"s{si}_timestamp"], ips=z[f"s{si}_ips"], num_bin=int(z["num_bin"]),
                 pd={g: z[f"s{si}_pd{gi}"] for gi, g in enumerate(gammas)}) for si in range(int(z["n_score_cases"]))]


def host_bins(ts, bounds):
    """The bin of every row by the reference's rule (PD-pairwise.py:93-96) in numpy; -1 when no bin takes the row."""
    num_bin = len(bounds) - 1
    bins = np.full(len(ts), -1, np.int32)
    for b in range(num_bin):
        index = (bounds[b] <= ts) & ((ts < bounds[b + 1]) if b < num_bin - 1 else (ts <= bounds[b + 1]))
        bins[index] = b
    return bins


def host_counts(photo, bins, num_bin, n_items):
    return np.stack([np.bincount(photo[bins == b], minlength=n_items) for b in range(num_bin)]).astype(np.int32)
