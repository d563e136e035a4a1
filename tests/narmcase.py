"""Shared cases of the GRU-with-attention state-tracker tests and the tracker's record for the slot-tracker checks (a helper, not a test).
Buffer rows, the bars and the float32-restatement rule are the GRU tracker's (grucase); the inputs are grucase's with the first env's
length pinned to T and, where there is a second env, its length to T - 1, so that the longest session of a case is certain and not drawn.
The parameters are grucase's O(1) tensors at one layer plus the four tensors of the attention and the read-out from a generator of their
own: attn.a1, attn.a2 and attn.v at 1 / sqrt(32), bilinear at 1 / sqrt(64).

The model is smooth (sigmoid, tanh; no max, no ReLU): the gradient tests need no near-tie condition, and no case and no element is skipped or
masked."""
import math

import torch

import grucase
import slotcase
from cirs_hip import narm_host
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of  # noqa: F401

# (U, I, B, T, L, S, hot): users, items, envs, max_turn, encoder layers (1), dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, 1, 20, 0.0),          # the plain case; ragged lengths
         (30, 40, 3, 100, 1, 20, 0.0),         # a session of 100 positions: the j-walk over many batches of passes, the largest unnormalised c_p
         (20, 30, 2, 65, 1, 20, 0.0),          # lengths exactly 65 and 64: one position past a wavefront's width, and exactly at it
         (120, 200, 33, 20, 1, 20, 0.0),       # B is no multiple of any env grouping
         (30, 40, 6, 7, 1, 32, 0.0),           # every decoder lane is live
         (8, 9, 1, 3, 1, 20, 0.0),             # one env, one workgroup; position 0's single attention term c_0 = alpha_{0,0} h_0
         (8, 90, 48, 30, 1, 20, 0.6)]          # one hot item: long segments in the ordered embedding scatter
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-L{c[4]}-S{c[5]}" + ("-hot" if c[6] else "") for c in CASES]

NEW = ("attn.a1.weight", "attn.a2.weight", "attn.v.weight", "bilinear.weight")


def teacher_inputs(U, I, B, T, hot=0.0):
    """grucase.teacher_inputs (same draws) with lens[0] = T and, where B >= 2, lens[1] = T - 1."""
    users, acts, rews, lens, rng = grucase.teacher_inputs(U, I, B, T, hot)
    lens = lens.copy()
    lens[0] = T
    if B >= 2:
        lens[1] = T - 1
    return users, acts, rews, lens, rng


def narm_param_dict(U, I, seed, D=32, S=20, emb_scale=0.5):
    """grucase.gru_param_dict's tensors at one layer (same seed -> same tensors), then the attention's and the read-out's tensors from a
    generator of their own; keyed and ordered like cirs_hip.narm_tracker.narm_param_shapes."""
    base = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=1, emb_scale=emb_scale)
    g = torch.Generator().manual_seed(seed + 104729)
    p = {k: v for k, v in base.items() if not k.startswith("decoder.")}
    p["attn.a1.weight"] = torch.randn(D, D, generator=g) / math.sqrt(D)
    p["attn.a2.weight"] = torch.randn(D, D, generator=g) / math.sqrt(D)
    p["attn.v.weight"] = torch.randn(1, D, generator=g) / math.sqrt(D)
    p["bilinear.weight"] = torch.randn(D, 2 * D, generator=g) / math.sqrt(2 * D)
    p["decoder.weight"], p["decoder.bias"] = base["decoder.weight"], base["decoder.bias"]
    return p


def device_narm_trainable(p, U, I, B, T, S):
    from cirs_hip.narm_tracker import DeviceNarmTracker, narm_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(narm_param_shapes(U, I, 32, S), init=p)
    trk = DeviceNarmTracker(dict(views), U, I, B, T, dim_state=S)
    trk.enable_training(flat)
    return trk, views


class Narm(slotcase.Slot):
    name, display, entry, host = "narm", "NARM", "cirs_narm_tracker", narm_host
    # two more envs than 4 x workgroups-per-CU x CUs on a 256-CU part.  The step kernel keeps 43 392 bytes of LDS per workgroup (the cell's two
    # matrices and biases 25 600, A1 and A2 8 448, Bw 8 320, four wavefronts' vectors 1 024): three workgroups fit in a CU's 160 KB (a fourth
    # would need 173 568 bytes), four envs (one per wavefront) each: 4 x 3 x 256 = 3072, so 3074 envs make every workgroup walk a second group
    # of four, the last one ragged (two envs).  T = 3: attention over one, two and three hidden states
    walk = ((3074, 3, 1, 5),)
    rollout_model, rollout_seed, example_model, plugin_model, plugin_seed = 1, 2, 1, 1, 4
    state_names = NEW + ("gru.weight_ih_l0", "gru.weight_hh_l0", "embedding_dict.feat_item.weight", "decoder.bias")

    @property
    def case(self):
        import narmcase
        return narmcase

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return narm_param_dict(Uc, Ic, seed, S=Sc)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.narm_tracker import narm_param_shapes
        return narm_param_shapes(Uc, Ic, 32, Sc)

    def n_grad_tensors(self, model):
        return 16

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return device_narm_trainable(p, Uc, Ic, B, Tc, Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.narm_tracker import DeviceNarmTracker
        return DeviceNarmTracker(params, Uc, Ic, B, Tc, dim_state=Sc, nlayers=model)

    def engine_refusals(self, params):
        return [(ValueError, "nlayers", lambda: self.engine(params, slotcase.U, slotcase.I, 6, slotcase.T, slotcase.S, 2))]


SLOT = Narm()
