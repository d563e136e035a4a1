"""Shared cases of the pooled-window state-tracker tests (a helper, not a test).  Inputs, buffer rows, the bars and the float32-restatement
rule are the GRU tracker's (grucase); the parameters are grucase's O(1) tensors without the gru.* entries.  emb_scale = 0.5: a window that is
off by one slot moves a state by about 0.1 of its scale, four orders above the bar."""
import grucase
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of, teacher_inputs  # noqa: F401

# (U, I, B, T, W, S, hot): users, items, envs, max_turn, window, dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, 3, 20, 0.0),        # the window slides
         (30, 40, 5, 100, 10, 20, 0.0),      # max_len 101
         (300, 500, 70, 30, 1, 20, 0.0),     # W = 1
         (30, 40, 6, 7, 7, 32, 0.0),         # W = T: never slides; every decoder lane live
         (30, 40, 6, 7, 64, 32, 0.0),        # W beyond the history
         (8, 9, 1, 3, 2, 20, 0.0),           # one env
         (8, 90, 48, 30, 30, 20, 0.6)]       # one hot item: long segments in the ordered scatter
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-W{c[4]}-S{c[5]}" + ("-hot" if c[6] else "") for c in CASES]


def avg_param_dict(U, I, seed, D=32, S=20, emb_scale=0.5):
    """grucase.gru_param_dict's tensors (same seed -> same tensors) minus the gru.* entries; keyed and ordered like
    cirs_hip.avg_tracker.avg_param_shapes."""
    p = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=1, emb_scale=emb_scale)
    return {k: v for k, v in p.items() if not k.startswith("gru.")}


def device_avg_trainable(p, U, I, B, T, W, S):
    from cirs_hip.avg_tracker import DeviceAvgTracker, avg_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(avg_param_shapes(U, I, 32, S), init=p)
    trk = DeviceAvgTracker(dict(views), U, I, B, T, dim_state=S, window_size=W)
    trk.enable_training(flat)
    return trk, views
