"""Shared cases of the convolutional window state-tracker tests (a helper, not a test).  Inputs, buffer rows, the bars and the
float32-restatement rule are the GRU tracker's (grucase); the parameters are grucase's O(1) tensors without the gru.* entries plus the filter
banks, the vertical filter and fc at 1 / sqrt(fan_in).  Biases are +-(0.05 .. 0.15) with both signs: relu(bias) of an all-zero patch sometimes
wins the max, and no pre-activation of an all-zero window sits at a ReLU's kink.

Max-pool and ReLU make the gradient discontinuous, so the inputs must be ones where float64 itself is unambiguous (the near-tie condition of
tests/test_caser_host_cpu.py).  SEEDS holds, per case, the first parameter seed, searched upwards from 3 on the CPU, that meets it with four
times the test's factor -- the third case meets it 19-fold at seed 3 and 32-fold at no seed below 60, so it keeps seed 3."""
import math

import torch

import grucase
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of, teacher_inputs  # noqa: F401

# (U, I, B, T, W, heights, S, hot): users, items, envs, max_turn, window, filter heights, dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, 4, (2, 3, 4), 20, 0.0),          # the window slides; W = the tallest filter: height 4 pools over a single position
         (30, 40, 5, 100, 10, (2, 3, 4), 20, 0.0),        # max_len 101: the default shape
         (120, 200, 33, 30, 16, (1, 2, 3, 4), 20, 0.0),   # W at its cap, all four banks; B no multiple of any env grouping
         (30, 40, 6, 7, 8, (3,), 32, 0.0),                # W > T: zero rows in every window; one bank; every decoder lane live
         (8, 9, 1, 3, 4, (4,), 20, 0.0),                  # one env; the history is shorter than the filter
         (8, 90, 48, 30, 10, (2, 3, 4), 20, 0.6)]         # one hot item: long segments in the ordered scatter
SEEDS = [3, 3, 3, 3, 3, 21]
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-W{c[4]}-h{''.join(map(str, c[5]))}-S{c[6]}" + ("-hot" if c[7] else "") for c in CASES]
NUM_FILTERS = 16


def caser_param_dict(U, I, seed, W, heights, D=32, S=20, emb_scale=0.5):
    """grucase.gru_param_dict's tensors (same seed -> same tensors) minus the gru.* entries, then the Caser tensors from a generator of their
    own; keyed and ordered like cirs_hip.caser_tracker.caser_param_shapes."""
    base = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=1, emb_scale=emb_scale)
    g = torch.Generator().manual_seed(seed + 7919)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def bias(n):
        sign = (torch.rand(n, generator=g) < 0.5).float() * 2 - 1
        return sign * (0.05 + 0.1 * torch.rand(n, generator=g))

    F = NUM_FILTERS
    p = {k: v for k, v in base.items() if not k.startswith("gru.") and not k.startswith("decoder.")}
    for i, h in enumerate(heights):
        p[f"horizontal_cnn.{i}.weight"] = rn(F, 1, h, D, scale=1 / math.sqrt(h * D))
        p[f"horizontal_cnn.{i}.bias"] = bias(F)
    p["vertical_cnn.weight"] = rn(1, 1, W, 1, scale=1 / math.sqrt(W))
    p["vertical_cnn.bias"] = bias(1)
    KC = F * len(heights) + D
    p["fc.weight"] = rn(D, KC, scale=1 / math.sqrt(KC))
    p["fc.bias"] = bias(D)
    p["decoder.weight"], p["decoder.bias"] = base["decoder.weight"], base["decoder.bias"]
    return p


def case_params(ci):
    U, I, B, T, W, heights, S, hot = CASES[ci]
    return caser_param_dict(U, I, SEEDS[ci], W, heights, S=S)


def device_caser_trainable(p, U, I, B, T, W, heights, S):
    from cirs_hip.caser_tracker import DeviceCaserTracker, caser_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(caser_param_shapes(U, I, 32, S, W, heights), init=p)
    trk = DeviceCaserTracker(dict(views), U, I, B, T, dim_state=S, window_size=W, filter_sizes=heights)
    trk.enable_training(flat)
    return trk, views


def near_tie_margins(p, users, acts, rews, lens, W):
    """{quantity: (min |q| in float64, max |q32 - q64|)} over the live rows (env b, position < lens[b]) for the four quantities at which the
    model is not smooth: the gap between the pooled maximum and the best runner-up whose patch is not identical to the arg-max's (identical
    patches -- all-zero ones -- give the same gradients whichever is taken), the pooled maximum (its ReLU), every vertical and every fc
    pre-activation (their ReLUs).  The float32 run is measured at float64's arg-max and runner-up."""
    import numpy as np
    from cirs_hip import caser_host
    q = {}
    for dtype in (torch.float64, torch.float32):
        pd = caser_host.cast_params(p, dtype)
        X = caser_host.input_slots(pd, users, acts, rews)
        B, L, D = X.shape
        live = (np.arange(L)[None, :] < np.asarray(lens)[:, None]).reshape(-1)
        win = caser_host.windows(X, W).reshape(B * L, W, D)[torch.as_tensor(live)]
        cs, vpre = caser_host.pre_activations(pd, win)
        q[dtype] = dict(win=win.numpy(), cs=[c.numpy() for c in cs], vpre=vpre.numpy(), zpre=caser_host.features(pd, win)[1].numpy())
    a, b = q[torch.float64], q[torch.float32]
    out = {"vertical": (np.abs(a["vpre"]).min(), np.abs(b["vpre"] - a["vpre"]).max()), "fc": (np.abs(a["zpre"]).min(), np.abs(b["zpre"] - a["zpre"]).max())}
    gaps, gap_err, tops, top_err = [], [], [], []
    for i, h in enumerate(caser_host.heights_of(p)):
        c64, c32 = a["cs"][i], b["cs"][i].astype(np.float64)          # [N, F, nT]
        N, F, nT = c64.shape
        patches = np.stack([a["win"][:, t:t + h].reshape(N, -1) for t in range(nT)], 1)                 # [N, nT, h D]
        same = (patches[:, :, None, :] == patches[:, None, :, :]).all(-1)                               # [N, nT, nT]
        arg = c64.argmax(-1)                                                                            # first maximal t
        rival = ~np.take_along_axis(same, arg[:, :, None].repeat(nT, 2), 1) if nT > 1 else np.zeros((N, F, nT), bool)
        top64, top32 = np.take_along_axis(c64, arg[..., None], -1)[..., 0], np.take_along_axis(c32, arg[..., None], -1)[..., 0]
        run = np.where(rival, c64, -np.inf)
        ra = run.argmax(-1)
        run64, run32 = np.take_along_axis(run, ra[..., None], -1)[..., 0], np.take_along_axis(c32, ra[..., None], -1)[..., 0]
        has = rival.any(-1)
        tops.append(np.abs(top64).min()); top_err.append(np.abs(top32 - top64).max())
        if has.any():
            gaps.append((top64 - run64)[has].min()); gap_err.append(np.abs((top32 - run32) - (top64 - run64))[has].max())
    out["pooled maximum"] = (min(tops), max(top_err))
    out["gap to the runner-up"] = (min(gaps), max(gap_err)) if gaps else (np.inf, 0.0)
    return out
