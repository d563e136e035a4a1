"""Shared cases of the LSTM state-tracker tests (a helper, not a test).  Inputs, buffer rows, the bars and the float32-restatement rule are
the GRU tracker's (grucase); the parameters are grucase's shared tensors around O(1) LSTM tensors.

With exactly these parameters and inputs the float32 restatement's own error (cirs_hip/lstm_host.py at float32 against float64, on a CPU)
is at most 2.8e-7 on the states and 1.1e-6 on the gradients, relative to max-abs: bar_for stays at the fixed bars in every case."""
import torch

import grucase
from grucase import GRAD_BAR, STATE_BAR, bar_for, rows_of, teacher_inputs  # noqa: F401

# (U, I, B, T, L, S, hot): users, items, envs, max_turn, LSTM layers, dim_state, share of the actions that are ONE item -- the smallest
# shapes at which each part can go wrong
CASES = [(8, 9, 1, 3, 1, 20, 0.0),          # one env: three of a workgroup's four wavefronts idle
         (50, 80, 9, 12, 1, 20, 0.0),       # a ragged last workgroup
         (30, 40, 5, 100, 2, 20, 0.0),      # the longest chain through c, two layers
         (30, 40, 6, 7, 2, 32, 0.0),        # every decoder lane live
         (300, 500, 70, 30, 1, 20, 0.0),    # many workgroups
         (8, 90, 48, 30, 1, 20, 0.6)]       # long segments in the ordered scatter
IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-L{c[4]}-S{c[5]}" + ("-hot" if c[6] else "") for c in CASES]


def lstm_param_dict(U, I, seed, D=32, S=20, nlayers=1):
    """grucase.gru_param_dict's shared tensors (same seed -> same tensors), lstm.* weights ~ 0.18 N(0, 1) and biases ~ 0.1 N(0, 1) from a
    generator of their own; keyed and ordered like cirs_hip.lstm_tracker.lstm_param_shapes."""
    p = grucase.gru_param_dict(U, I, seed, D=D, S=S, nlayers=nlayers)
    g = torch.Generator().manual_seed(seed + 1000)
    q = {k: v for k, v in p.items() if not k.startswith("gru.") and not k.startswith("decoder.")}
    for l in range(nlayers):
        q[f"lstm.weight_ih_l{l}"] = torch.randn(4 * D, D, generator=g) * 0.18; q[f"lstm.weight_hh_l{l}"] = torch.randn(4 * D, D, generator=g) * 0.18
        q[f"lstm.bias_ih_l{l}"] = torch.randn(4 * D, generator=g) * 0.1; q[f"lstm.bias_hh_l{l}"] = torch.randn(4 * D, generator=g) * 0.1
    q["decoder.weight"], q["decoder.bias"] = p["decoder.weight"], p["decoder.bias"]
    return q


def device_lstm_trainable(p, U, I, B, T, nlayers, S):
    from cirs_hip.lstm_tracker import DeviceLstmTracker, lstm_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(lstm_param_shapes(U, I, 32, S, nlayers), init=p)
    trk = DeviceLstmTracker(dict(views), U, I, B, T, dim_state=S, nlayers=nlayers)
    trk.enable_training(flat)
    return trk, views
