"""Shared cases of the filter-MLP state-tracker tests and the tracker's record for the slot-tracker checks (a helper, not a test).
Inputs, buffer rows, the bars and the float32-restatement rule are the GRU tracker's (grucase); the parameters are grucase's O(1) tensors
without the gru.* entries plus the nine tensors of every layer from a generator of their own: complex_weight at 0.5 N(0, 1), the dense weights
at 1 / sqrt(fan_in), the dense and LayerNorm biases at 0.1 N(0, 1), the LayerNorm weights at 1 + 0.1 N(0, 1).  At these scales every tensor
receives a gradient of size >= 0.5 in every case and the float32 restatement's own error stays at a few 1e-7.

`model` is (W, L): the window and the layer count.  The model is smooth (LayerNorm, the erf GELU; no max, no ReLU): the gradient tests need
no near-tie condition, and no case and no element is skipped or masked."""
import math

import torch

import grucase
import slotcase
from cirs_hip import fmlp_host
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of, teacher_inputs  # noqa: F401

# (U, I, B, T, (W, L), S, hot): users, items, envs, max_turn, (window, layers), dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, (3, 2), 20, 0.0),         # odd W < T, not a power of two; tile rows 3 .. 15 are don't-cares that layer 1 must not read
         (30, 40, 3, 100, (10, 2), 20, 0.0),       # the default at max_len 101
         (120, 200, 33, 20, (16, 2), 20, 0.0),     # the full tile and its Nyquist bin; B is no multiple of any grouping
         (30, 40, 6, 7, (16, 1), 32, 0.0),         # W > T: padded rows at every position; one layer; every decoder lane live
         (8, 9, 1, 3, (1, 2), 20, 0.0),            # W = 1: the DC bin only
         (8, 9, 2, 4, (2, 2), 20, 0.0),            # W = 2: DC + Nyquist only, every imaginary gradient zero
         (20, 30, 5, 9, (5, 2), 20, 0.0),          # odd W, no Nyquist bin
         (8, 90, 48, 30, (10, 2), 20, 0.6)]        # one hot item: long segments in the ordered scatter
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-W{c[4][0]}-L{c[4][1]}-S{c[5]}" + ("-hot" if c[6] else "") for c in CASES]
SEED = 3      # the parameter seed of every case

LAYER = ("filter.complex_weight", "filter.ln.weight", "filter.ln.bias", "ffn.dense_1.weight", "ffn.dense_1.bias", "ffn.dense_2.weight",
         "ffn.dense_2.bias", "ffn.ln.weight", "ffn.ln.bias")


def new_names(L):
    return tuple(f"layers.{l}.{k}" for l in range(L) for k in LAYER)


def fmlp_param_dict(U, I, seed, W, L, D=32, S=20, emb_scale=0.5):
    """grucase.gru_param_dict's tensors (same seed -> same tensors) minus the gru.* entries, then the layers' tensors from a generator of
    their own; keyed and ordered like cirs_hip.fmlp_tracker.fmlp_param_shapes."""
    from cirs_hip.fmlp_tracker import fmlp_param_shapes
    base = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=1, emb_scale=emb_scale)
    g = torch.Generator().manual_seed(seed + 7919)
    shapes = fmlp_param_shapes(U, I, D, S, W, L)
    p = {k: v for k, v in base.items() if not k.startswith("gru.") and not k.startswith("decoder.")}
    for k in new_names(L):
        sh = shapes[k]
        if k.endswith("complex_weight"):
            p[k] = 0.5 * torch.randn(*sh, generator=g)
        elif k.endswith("ln.weight"):
            p[k] = 1.0 + 0.1 * torch.randn(*sh, generator=g)
        elif k.endswith(".weight"):
            p[k] = torch.randn(*sh, generator=g) / math.sqrt(sh[1])
        else:
            p[k] = 0.1 * torch.randn(*sh, generator=g)
    p["decoder.weight"], p["decoder.bias"] = base["decoder.weight"], base["decoder.bias"]
    assert list(p) == list(shapes)
    return p


def device_fmlp_trainable(p, U, I, B, T, W, L, S):
    from cirs_hip.fmlp_tracker import DeviceFmlpTracker, fmlp_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(fmlp_param_shapes(U, I, 32, S, W, L), init=p)
    trk = DeviceFmlpTracker(dict(views), U, I, B, T, dim_state=S, window_size=W, nlayers=L)
    trk.enable_training(flat)
    return trk, views


class Fmlp(slotcase.Slot):
    name, display, entry, host = "fmlp", "FMLP", "cirs_fmlp_tracker", fmlp_host
    # more than (envs per workgroup) x (workgroups per CU) x CUs envs on a 256-CU part.  The step kernel keeps 131 328 bytes of LDS per workgroup (both
    # layers' dense_1 and dense_2 as the MFMA's operands: 70 656; complex_weight and the taps; the decoder and the slot's matrix; four 16-row tiles
    # and four 16 x 128 hidden tiles: 43 008): one workgroup fits in a CU's 160 KB, four envs (one per wavefront) each: 4 x 1 x 256 = 1024, so 1030 envs make every workgroup
    # walk a second group of four, the last one ragged (two envs).  T = 4 with W = 3: tiles with two, one and no padded rows, and at position 4 a
    # live older slot that the tile must not hold
    walk = ((1030, 4, (3, 2), 5),)
    rollout_model, rollout_seed, plugin_model, plugin_seed = (3, 2), 2, (3, 2), 4      # T = 8: the tile slides from position 4 on
    example_model = (2, 1)
    state_names = new_names(1) + ("embedding_dict.feat_item.weight", "decoder.bias")

    @property
    def case(self):
        import fmlpcase
        return fmlpcase

    def host_arg(self, model):
        return model[0]      # the restatement reads the layer count off the parameters

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return fmlp_param_dict(Uc, Ic, seed, model[0], model[1], S=Sc)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.fmlp_tracker import fmlp_param_shapes
        return fmlp_param_shapes(Uc, Ic, 32, Sc, model[0], model[1])

    def n_grad_tensors(self, model):
        return 8 + 9 * model[1]

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return device_fmlp_trainable(p, Uc, Ic, B, Tc, model[0], model[1], Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.fmlp_tracker import DeviceFmlpTracker
        return DeviceFmlpTracker(params, Uc, Ic, B, Tc, dim_state=Sc, window_size=model[0], nlayers=model[1])

    def flags(self, model):
        return ["--window-size", str(model[0]), "--fmlp-layers", str(model[1])]

    def plugin_kw(self, model):
        return {"window_size": model[0], "nlayers": model[1]}

    def engine_refusals(self, params):
        U, I, T, S = slotcase.U, slotcase.I, slotcase.T, slotcase.S
        return [(ValueError, "window_size", lambda: self.engine(params, U, I, 6, T, S, (0, 2))),
                (ValueError, "window_size", lambda: self.engine(params, U, I, 6, T, S, (17, 2))),
                (ValueError, "nlayers", lambda: self.engine(params, U, I, 6, T, S, (3, 3)))]


SLOT = Fmlp()
