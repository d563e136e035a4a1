"""Shared cases of the attention-pool state-tracker tests and the tracker's record for the slot-tracker checks (a helper, not a test).
Inputs, buffer rows, the bars and the float32-restatement rule are the GRU tracker's (grucase); the parameters are grucase's O(1) tensors
without the gru.* entries plus the nine tensors of the attention and the read-out from a generator of their own: the five square weights and
attn.w0 at 1 / sqrt(32), the three biases at 0.1 N(0, 1).

The model is smooth (sigmoid, tanh; no max, no ReLU): the gradient tests need no near-tie condition, and no case and no element is skipped or
masked."""
import math

import torch

import grucase
import slotcase
from cirs_hip import stamp_host
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of, teacher_inputs  # noqa: F401

# (U, I, B, T, W, S, hot): users, items, envs, max_turn, window, dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, 3, 20, 0.0),          # W < T: the window grows, fills and slides; tile rows beyond the window are live older slots
         (30, 40, 3, 100, 10, 20, 0.0),        # the default window at max_len 101
         (120, 200, 33, 20, 16, 20, 0.0),      # the full 16-row tile; B is no multiple of any env grouping
         (30, 40, 6, 7, 16, 32, 0.0),          # W > T: the window is never full; every decoder lane is live
         (8, 9, 1, 3, 1, 20, 0.0),             # one env, W = 1: m_s = m_t, one attention term
         (8, 90, 48, 30, 10, 20, 0.6)]         # one hot item: long segments in the ordered scatter
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-W{c[4]}-S{c[5]}" + ("-hot" if c[6] else "") for c in CASES]
SEED = 3      # the parameter seed of every case

SQUARE = ("attn.w1.weight", "attn.w2.weight", "attn.w3.weight", "mlp_a.weight", "mlp_b.weight")
NEW = ("attn.bias", "attn.w1.weight", "attn.w2.weight", "attn.w3.weight", "attn.w0.weight", "mlp_a.weight", "mlp_a.bias", "mlp_b.weight", "mlp_b.bias")


def stamp_param_dict(U, I, seed, D=32, S=20, emb_scale=0.5):
    """grucase.gru_param_dict's tensors (same seed -> same tensors) minus the gru.* entries, then the attention's and the read-out's tensors
    from a generator of their own; keyed and ordered like cirs_hip.stamp_tracker.stamp_param_shapes."""
    base = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=1, emb_scale=emb_scale)
    g = torch.Generator().manual_seed(seed + 7919)
    p = {k: v for k, v in base.items() if not k.startswith("gru.") and not k.startswith("decoder.")}
    for k in NEW:
        if k in SQUARE:
            p[k] = torch.randn(D, D, generator=g) / math.sqrt(D)
        elif k == "attn.w0.weight":
            p[k] = torch.randn(1, D, generator=g) / math.sqrt(D)
        else:
            p[k] = 0.1 * torch.randn(D, generator=g)
    p["decoder.weight"], p["decoder.bias"] = base["decoder.weight"], base["decoder.bias"]
    return p


def device_stamp_trainable(p, U, I, B, T, W, S):
    from cirs_hip.stamp_tracker import DeviceStampTracker, stamp_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(stamp_param_shapes(U, I, 32, S), init=p)
    trk = DeviceStampTracker(dict(views), U, I, B, T, dim_state=S, window_size=W)
    trk.enable_training(flat)
    return trk, views


class Stamp(slotcase.Slot):
    name, display, entry, host = "stamp", "STAMP", "cirs_stamp_tracker", stamp_host
    # more than 4 x workgroups-per-CU x CUs envs on a 256-CU part.  The step kernel keeps 40 448 bytes of LDS per workgroup (W1 as the MFMA's
    # operand, W2, W3, A, B, the decoder and the slot's matrix, four 16-row tiles, four sets of vectors): four workgroups fit in a CU's 160 KB,
    # four envs (one per wavefront) each: 4 x 4 x 256 = 4096, so 4102 envs make every workgroup walk a second group of four, the last one
    # ragged (two envs).  T = 4 with W = 3: windows of one, two and three slots, and at position 4 a live older slot in front of the window
    walk = ((4102, 4, 3, 5),)
    rollout_model, rollout_seed, plugin_model, plugin_seed = 3, 2, 3, 4      # T = 8: the window slides from position 4 on
    example_model = 2
    state_names = NEW + ("embedding_dict.feat_item.weight", "decoder.bias")

    @property
    def case(self):
        import stampcase
        return stampcase

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return stamp_param_dict(Uc, Ic, seed, S=Sc)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.stamp_tracker import stamp_param_shapes
        return stamp_param_shapes(Uc, Ic, 32, Sc)

    def n_grad_tensors(self, model):
        return 17

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return device_stamp_trainable(p, Uc, Ic, B, Tc, model, Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.stamp_tracker import DeviceStampTracker
        return DeviceStampTracker(params, Uc, Ic, B, Tc, dim_state=Sc, window_size=model)

    def flags(self, model):
        return ["--window-size", str(model)]

    def plugin_kw(self, model):
        return {"window_size": model}

    def engine_refusals(self, params):
        return [(ValueError, "window_size", lambda: self.engine(params, slotcase.U, slotcase.I, 6, slotcase.T, slotcase.S, 0)),
                (ValueError, "window_size", lambda: self.engine(params, slotcase.U, slotcase.I, 6, slotcase.T, slotcase.S, 17))]


SLOT = Stamp()
