"""The LinUCB fixture (tests/golden/linucb.npz, written by tools/gen_golden_linucb.py), the error protocol of its comparisons and the
synthetic logs that the fixture generator and the GPU tests share.

Error protocol.  inv(A) is ill-conditioned on this workload (cond_2 up to 1e12: within an arm only the user id varies), so neither the
reference nor the device reproduces the other bit for bit, and a fixed rtol would be wrong in either direction.  The fixture therefore
records, next to the reference's float64 results, the EXACT results (Gauss-Jordan over fractions.Fraction on the recorded A and b,
rounded to float64 once), and for every case, recorded epoch and quantity the reference's own error
    E_ref = max |reference - exact| / max |exact|         over all entries of the quantity.
A result under test gets E_dev the same way, against the same exact values, and passes when E_dev <= FACTOR * E_ref: no worse than the
reference in effect (the convention of tests/test_gpu_head_precision.py)."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linucb.npz")
FACTOR = 4.0
QUANTITIES = ("theta", "mean", "var", "ucb", "y_predict")
N_FEAT_VALUES = 32


def rel_err(got, exact, scale=None):
    """max |got - exact| / max |exact|; scale: the array whose largest magnitude is the denominator when `exact` is only a part of it."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    return float(np.abs(got - exact).max() / np.abs(exact if scale is None else scale).max())


def within(E_dev, E_ref):
    return E_dev <= FACTOR * E_ref


def check(what, got, exact, E_ref, scale=None):
    """Assert `got` inside the bar; prints the figures first.  At shapes the fixture does not hold, the host restatement's values take
    the place of the exact ones and E_ref is case 1's."""
    E_dev = rel_err(got, exact, scale)
    print(f"{what}: E_dev {E_dev:.3e}  E_ref {E_ref:.3e}  ratio {E_dev / E_ref if E_ref else float('inf'):.3g}")
    assert within(E_dev, E_ref), f"{what}: E_dev {E_dev:.3e} > {FACTOR:g} x E_ref {E_ref:.3e}"
    return E_dev


def load():
    z = np.load(GOLDEN)
    cases = []
    for ci in range(int(z["n_cases"])):
        pre = f"c{ci}_"
        c = SimpleNamespace(index=ci, **{k[len(pre):]: z[k] for k in z.files if k.startswith(pre) and not k[len(pre):].startswith("e")})
        c.K, c.d, c.alpha = int(len(c.classes)), int(c.x.shape[1]), float(c.alpha)
        c.epochs = [int(e) for e in z[pre + "epochs"]]
        c.full = [int(e) for e in c.full]                                   # the epochs with the solve-dependent recordings
        c.rec = {}
        for e in c.epochs:
            epre = f"{pre}e{e}_"
            r = SimpleNamespace(**{k[len(epre):]: z[k] for k in z.files if k.startswith(epre)})
            for k in [k for k in vars(r) if k.endswith("_dref")]:         # stored as the difference to the exact values: exact sum
                setattr(r, k[:-5] + "_ref", getattr(r, k[:-5] + "_exact") + getattr(r, k))
            if e in c.full:
                r.eref = {q: float(z[pre + "eref_" + q][c.full.index(e)]) for q in QUANTITIES}
            c.rec[e] = r
        cases.append(c)
    return cases


# ---- synthetic logs ----------------------------------------------------------------------------------------------------------------
def make_item_feats(rng, K, d):
    """[K, d - 2]: category-like integer columns and, last, a fractional duration (df_photo_env: feat0.. , photo_duration)."""
    w = d - 2
    feats = np.zeros((K, w))
    if w > 1:
        feats[:, :w - 1] = rng.randint(0, N_FEAT_VALUES, (K, w - 1))
    if w > 0:
        feats[:, w - 1] = rng.uniform(2.0, 60.0, K)
    return feats


def skewed_counts(rng, K, n, heavy=None):
    """Rows per arm, n in all: arm order random, sizes falling like a power law; `heavy`: the largest arm gets exactly that many."""
    w = 1.0 / np.arange(1, K + 1) ** 1.1
    w = w[rng.permutation(K)]
    if heavy is not None and K > 1:
        top = int(np.argmax(w))
        rest = np.delete(np.arange(K), top)
        cnt = np.zeros(K, np.int64)
        cnt[top] = heavy
        cnt[rest] = rng.multinomial(n - heavy, w[rest] / w[rest].sum())
        return cnt
    return rng.multinomial(n, w / w.sum()).astype(np.int64)


def make_log(rng, classes, item_feats, user_ids, counts, n_outside=0, raw_space=None):
    """A log x [n, d] = [user id, RAW photo id, the photo's feature columns], y [n]: counts[a] rows of arm a and n_outside rows whose
    raw id is not in `classes`, in random order (the rows of an arm interleave with the others')."""
    classes = np.asarray(classes, np.int64)
    K, w = len(classes), item_feats.shape[1]
    arms = np.repeat(np.arange(K), counts)
    raw = classes[arms].astype(np.float64)
    feats = item_feats[arms]
    if n_outside:
        free = np.setdiff1d(np.arange(raw_space if raw_space else int(classes.max()) + 2 + n_outside), classes)
        raw = np.r_[raw, rng.choice(free, n_outside).astype(np.float64)]
        feats = np.r_[feats, make_item_feats(rng, n_outside, w + 2)]
    n = len(raw)
    x = np.concatenate([rng.choice(user_ids, n).astype(np.float64)[:, None], raw[:, None], feats], axis=1)
    y = rng.uniform(0.0, 2.0, n)
    perm = rng.permutation(n)
    return np.ascontiguousarray(x[perm]), np.ascontiguousarray(y[perm])


CASE1_USER_SPACE, CASE1_ITEM_SPACE = 7176, 10728      # user ids up to 7175, raw photo ids up to 10727


def synthetic_problem(seed, K, d, n_rows, heavy=None, n_outside=0, every_arm=False):
    """A log at case 1's id ranges -> (classes [K], item_feats [K, d - 2], x, y, user_ids).  every_arm: every arm has at least one row,
    as in case 1 (n_rows grows by the rows that adds)."""
    rng = np.random.RandomState(seed)
    classes = np.sort(rng.choice(CASE1_ITEM_SPACE, K, replace=False)).astype(np.int64)
    item_feats = make_item_feats(rng, K, d)
    user_ids = rng.choice(CASE1_USER_SPACE, min(CASE1_USER_SPACE, 400), replace=False)
    counts = skewed_counts(rng, K, n_rows, heavy=heavy)
    if every_arm:
        counts = np.maximum(counts, 1)
    x, y = make_log(rng, classes, item_feats, user_ids, counts, n_outside=n_outside, raw_space=CASE1_ITEM_SPACE)
    return classes, item_feats, x, y, user_ids
