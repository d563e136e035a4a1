"""Shared cases of the dilated-convolution state-tracker tests and the tracker's record for the slot-tracker checks (a helper, not a test).
Inputs, buffer rows, the bars and the float32-restatement rule are the GRU tracker's (grucase); the parameters are grucase's O(1) tensors
without the gru.* entries plus, per block, the conv weight at 1 / sqrt(fan_in = 96), the LayerNorm weight around 1, and biases +-(0.05 .. 0.15)
with both signs.

ReLU makes the gradient discontinuous, and there are 32 of them per (block, position), so the inputs must be ones where float64 itself is
unambiguous: for every block and every live item position |n^l_t| in float64 is at least 8 x the float32 restatement's own maximum error on
n^l (the near-tie condition of tests/test_nextitnet_host_cpu.py; the factor and its reason are DESIGN.md 7.5's).  SEEDS holds, per case, the
first parameter seed, searched upwards from 3 on the CPU, that meets it with four times that factor (32); a case with no such seed below 200
takes the first seed that meets the plain factor.  RATIOS records what the chosen seed measured (min |n| / error, the smallest over the blocks)."""
import math

import numpy as np
import torch

import grucase
import slotcase
from cirs_hip import nextitnet_host
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of, teacher_inputs  # noqa: F401

# (U, I, B, T, dilations, S, hot): users, items, envs, max_turn, the blocks' dilations, dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, (1, 2), 20, 0.0),              # R = 7 < T: histories shorter than, equal to and longer than the receptive field
         (30, 40, 3, 100, (1, 2, 4), 20, 0.0),          # the default dilations at max_len 101
         (120, 200, 33, 20, (1, 2, 1, 2), 20, 0.0),     # four blocks, a repeated dilation; B no multiple of any env grouping
         (30, 40, 6, 7, (1, 2, 4), 32, 0.0),            # R = 15 > T: every cone reaches before the first item at every layer; every decoder lane live
         (8, 9, 1, 3, (4,), 20, 0.0),                   # one env, one block, the largest dilation: every tap but the last reads padding
         (8, 90, 48, 30, (1, 2, 4), 20, 0.6)]           # one hot item: long segments in the ordered scatter
SEEDS = [3, 3, 13, 3, 3, 3]      # the third case: 27.8 at seed 3, first 32-fold at 13
RATIOS = [1207.2, 41.5, 134.4, 471.4, 257367.2, 68.1]
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-d{''.join(map(str, c[4]))}-S{c[5]}" + ("-hot" if c[6] else "") for c in CASES]
FACTOR = 8


def nextitnet_param_dict(U, I, seed, dilations, D=32, S=20, emb_scale=0.5):
    """grucase.gru_param_dict's tensors (same seed -> same tensors) minus the gru.* entries, then the blocks' tensors from a generator of their
    own; keyed and ordered like cirs_hip.nextitnet_tracker.nextitnet_param_shapes."""
    base = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=1, emb_scale=emb_scale)
    g = torch.Generator().manual_seed(seed + 7907)

    def bias(n):
        sign = (torch.rand(n, generator=g) < 0.5).float() * 2 - 1
        return sign * (0.05 + 0.1 * torch.rand(n, generator=g))

    p = {k: v for k, v in base.items() if not k.startswith("gru.") and not k.startswith("decoder.")}
    for l in range(len(dilations)):
        p[f"blocks.{l}.conv.weight"] = torch.randn(D, D, 3, generator=g) / math.sqrt(3 * D)
        p[f"blocks.{l}.conv.bias"] = bias(D)
        p[f"blocks.{l}.ln.weight"] = 1.0 + 0.1 * torch.randn(D, generator=g)
        p[f"blocks.{l}.ln.bias"] = bias(D)
    p["decoder.weight"], p["decoder.bias"] = base["decoder.weight"], base["decoder.bias"]
    return p


def case_params(ci, seed=None):
    U, I, B, T, dilations, S, hot = CASES[ci]
    return nextitnet_param_dict(U, I, SEEDS[ci] if seed is None else seed, dilations, S=S)


def device_nextitnet_trainable(p, U, I, B, T, dilations, S):
    from cirs_hip.nextitnet_tracker import DeviceNextItNetTracker, nextitnet_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(nextitnet_param_shapes(U, I, 32, S, dilations), init=p)
    trk = DeviceNextItNetTracker(dict(views), U, I, B, T, dim_state=S, dilations=dilations)
    trk.enable_training(flat)
    return trk, views


def near_tie_margins(p, users, acts, rews, lens, dilations):
    """{block: (min |n^l_t| in float64, max |n32 - n64|)} over the live item positions (env b, 1 <= t < lens[b]): the LayerNorm outputs, whose
    signs the ReLUs read.  The blocks are causal: n^l_t is the same number in every row whose cone holds t."""
    n = {}
    for dtype in (torch.float64, torch.float32):
        pd = nextitnet_host.cast_params(p, dtype)
        X = nextitnet_host.input_slots(pd, users, acts, rews)
        keep = []
        nextitnet_host.blocks(pd, X[:, 1:], dilations, keep)
        n[dtype] = [k[2].numpy().astype(np.float64) for k in keep]
    T = n[torch.float64][0].shape[1]
    live = np.arange(1, T + 1)[None, :] < np.asarray(lens)[:, None]      # [B, T]: item slot t = column t - 1
    return {f"block {l}": (np.abs(a[live]).min(), np.abs(b[live] - a[live]).max()) for l, (a, b) in enumerate(zip(n[torch.float64], n[torch.float32]))}


def near_tie_ratio(p, users, acts, rews, lens, dilations):
    """the smallest margin / error over the blocks"""
    return min(m / max(e, 1e-300) for m, e in near_tie_margins(p, users, acts, rews, lens, dilations).values())


class NextItNet(slotcase.Slot):
    name, display, entry, host = "nextitnet", "NextItNet", "cirs_nextitnet_tracker", nextitnet_host
    # more than 4 x workgroups-per-CU x CUs envs on a 256-CU part.  The step kernel keeps 73 984 bytes of LDS per workgroup (50 KB of conv weights,
    # the decoder, the slot's matrix, four 24-row tiles): two workgroups fit in a CU's 160 KB, four envs (one per wavefront) each: 4 x 2 x 256 =
    # 2048, so 2056 envs make every workgroup walk a second group of four, the last one ragged.  T = 4 with dilations (1, 2), R = 7: every cone
    # starts in the padding.  States only: they are continuous at every ReLU, so the near-tie condition of the gradient tests is not needed
    walk = ((2056, 4, (1, 2), 5),)
    rollout_model, rollout_seed = (1, 2), 6      # T = 8, R = 7: the cone starts inside the padding and slides off it
    plugin_model, plugin_seed = (1, 2), 3
    example_model = (2, 1)
    state_names = ("blocks.0.conv.weight", "blocks.0.conv.bias", "blocks.0.ln.weight", "blocks.1.ln.bias", "embedding_dict.feat_item.weight",
                   "decoder.bias")

    @property
    def case(self):
        import nextitnetcase
        return nextitnetcase

    def params(self, ci):
        return case_params(ci)      # the per-case SEEDS: the near-tie condition depends on them

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return nextitnet_param_dict(Uc, Ic, seed, model, S=Sc)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.nextitnet_tracker import nextitnet_param_shapes
        return nextitnet_param_shapes(Uc, Ic, 32, Sc, model)

    def n_grad_tensors(self, model):
        return 8 + 4 * len(model)

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return device_nextitnet_trainable(p, Uc, Ic, B, Tc, model, Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.nextitnet_tracker import DeviceNextItNetTracker
        return DeviceNextItNetTracker(params, Uc, Ic, B, Tc, dim_state=Sc, dilations=model)

    def flags(self, model):
        return ["--dilations", ",".join(map(str, model))]

    def plugin_kw(self, model):
        return {"dilations": tuple(model)}

    def engine_refusals(self, params):
        return [(ValueError, "dilations", lambda: self.engine(params, slotcase.U, slotcase.I, 6, slotcase.T, slotcase.S, (4, 4)))]      # sum 8

    def check_unambiguous(self, p, users, acts, rews, lens, model):
        for what, (margin, e32) in near_tie_margins(p, users, np.maximum(acts, 0), rews, lens, model).items():
            assert margin >= FACTOR * e32, f"the rollout's inputs sit near a ReLU's kink ({what}): choose another parameter seed"


SLOT = NextItNet()
