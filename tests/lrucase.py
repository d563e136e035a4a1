"""Shared cases of the linear-recurrence state-tracker tests and the tracker's record for the slot-tracker checks (a helper, not a test).
Buffer rows, the bars and the float32-restatement rule are the GRU tracker's (grucase); the inputs are narmcase.teacher_inputs (grucase's
with the first env's length pinned to T and, where there is a second env, its length to T - 1, so that the longest session of a case is
certain and not drawn).  The parameters are grucase's O(1) tensors at one layer without the gru.* entries plus the fifteen tensors of the
recurrence and the feed-forward block from a generator of their own: |lambda| uniform in [0.30, 0.98] and the phase uniform in
[0.05, 2 pi - 0.05] (as nu_log and theta_log), gamma_log = 1/2 log(1 - |lambda|^2), in_proj and dense_1 at 1 / sqrt(32), out_proj at
1 / sqrt(64), dense_2 at 1 / sqrt(128), every bias at 0.1 N(0, 1), the LayerNorm weights at 1 + 0.1 N(0, 1).

The model is smooth (a linear recurrence, LayerNorm, the erf GELU; no max, no ReLU): the gradient tests need no near-tie condition, and no
case and no element is skipped or masked."""
import math

import torch

import grucase
import slotcase
from cirs_hip import lru_host
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of  # noqa: F401
from narmcase import teacher_inputs  # noqa: F401

SCAN = 8      # lScan of csrc/lru_tracker.hip: the positions of a scan whose row loads are issued together

# (U, I, B, T, L, S, hot): users, items, envs, max_turn, recurrence layers (1), dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, 1, 20, 0.0),          # the plain case; ragged lengths
         (30, 40, 3, 100, 1, 20, 0.0),         # a session of 100 positions: twelve and a half load batches of the scans, the largest powers of lambda
         (20, 30, 2, 65, 1, 20, 0.0),          # lengths exactly 65 and 64: one position past eight full batches, and exactly eight
         (120, 200, 33, 20, 1, 20, 0.0),       # B is no multiple of any env grouping
         (30, 40, 6, 7, 1, 32, 0.0),           # every decoder lane is live; every session shorter than one batch
         (8, 9, 1, 3, 1, 20, 0.0),             # one env, one workgroup; position 0 alone is h_0 = u_0
         (8, 90, 48, 30, 1, 20, 0.6),          # one hot item: long segments in the ordered embedding scatter
         # T = SCAN + 1: the first env has SCAN + 1 positions -- one full batch of the scans and a batch that holds a single live position, whose
         # seven other loads are clamped to a live row and whose arithmetic must stop after one step (in the adjoint scan that lone position is
         # position 0, the one without a previous hidden state); the second env has exactly SCAN positions, one full batch and no tail
         (20, 30, 4, SCAN + 1, 1, 20, 0.0)]
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-L{c[4]}-S{c[5]}" + ("-hot" if c[6] else "") for c in CASES]

NEW = ("lru.nu_log", "lru.theta_log", "lru.gamma_log", "lru.in_proj.weight", "lru.in_proj.bias", "lru.out_proj.weight", "lru.out_proj.bias",
       "lru.ln.weight", "lru.ln.bias", "ffn.dense_1.weight", "ffn.dense_1.bias", "ffn.dense_2.weight", "ffn.dense_2.bias", "ffn.ln.weight",
       "ffn.ln.bias")


def lru_param_dict(U, I, seed, D=32, S=20, emb_scale=0.5):
    """grucase.gru_param_dict's tensors at one layer (same seed -> same tensors) minus the gru.* entries, then the recurrence's and the
    feed-forward block's tensors from a generator of their own; keyed and ordered like cirs_hip.lru_tracker.lru_param_shapes."""
    from cirs_hip.lru_tracker import lru_param_shapes
    base = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=1, emb_scale=emb_scale)
    g = torch.Generator().manual_seed(seed + 15485863)
    shapes = lru_param_shapes(U, I, D, S)
    p = {k: v for k, v in base.items() if not k.startswith("gru.") and not k.startswith("decoder.")}
    mod = 0.30 + 0.68 * torch.rand(D, generator=g)
    phi = 0.05 + (2 * math.pi - 0.10) * torch.rand(D, generator=g)
    p["lru.nu_log"] = torch.log(-torch.log(mod))
    p["lru.theta_log"] = torch.log(phi)
    p["lru.gamma_log"] = 0.5 * torch.log(1 - mod * mod)
    for k in NEW[3:]:
        sh = shapes[k]
        if k.endswith("ln.weight"):
            p[k] = 1.0 + 0.1 * torch.randn(*sh, generator=g)
        elif k.endswith(".weight"):
            p[k] = torch.randn(*sh, generator=g) / math.sqrt(sh[1])
        else:
            p[k] = 0.1 * torch.randn(*sh, generator=g)
    p["decoder.weight"], p["decoder.bias"] = base["decoder.weight"], base["decoder.bias"]
    assert list(p) == list(shapes)
    return p


def device_lru_trainable(p, U, I, B, T, S):
    from cirs_hip.lru_tracker import DeviceLruTracker, lru_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(lru_param_shapes(U, I, 32, S), init=p)
    trk = DeviceLruTracker(dict(views), U, I, B, T, dim_state=S)
    trk.enable_training(flat)
    return trk, views


class Lru(slotcase.Slot):
    name, display, entry, host = "lru", "LRU", "cirs_lru_tracker", lru_host
    # two more envs than 4 x workgroups-per-CU x CUs on a 256-CU part.  The step kernel keeps 63 104 bytes of LDS per workgroup (in_proj [64][33]
    # 8 448, out_proj [32][65] 8 320, dense_1 [128][33] 16 896, dense_2 [32][129] 16 512, the decoder and the slot's matrix [32][33] 4 224 each,
    # lambda and gamma 384, four wavefronts' vectors 4 096): two workgroups fit in a CU's 160 KB (a third would need 189 312 bytes), four envs (one
    # per wavefront) each: 4 x 2 x 256 = 2048, so 2050 envs make every workgroup walk a second group of four, the last one ragged (two envs).
    # T = 3: the recurrence over one, two and three positions
    walk = ((2050, 3, 1, 5),)
    rollout_model, rollout_seed, example_model, plugin_model, plugin_seed = 1, 2, 1, 1, 4
    state_names = NEW + ("embedding_dict.feat_item.weight", "decoder.bias")

    @property
    def case(self):
        import lrucase
        return lrucase

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return lru_param_dict(Uc, Ic, seed, S=Sc)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.lru_tracker import lru_param_shapes
        return lru_param_shapes(Uc, Ic, 32, Sc)

    def n_grad_tensors(self, model):
        return 23

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return device_lru_trainable(p, Uc, Ic, B, Tc, Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.lru_tracker import DeviceLruTracker
        return DeviceLruTracker(params, Uc, Ic, B, Tc, dim_state=Sc, nlayers=model)

    def engine_refusals(self, params):
        return [(ValueError, "nlayers", lambda: self.engine(params, slotcase.U, slotcase.I, 6, slotcase.T, slotcase.S, 2))]


SLOT = Lru()
