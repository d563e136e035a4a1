"""Host restatement of the LSTM state tracker (csrc/lstm_tracker.hip) in plain torch at a chosen dtype: the checker of every device
number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format itself
costs.  Nothing here imports the device path.

The model (there is no reference text: the reference declares StateTrackerLSTM and leaves it empty, core/state_tracker.py:282-289):
  slots       the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  cell        i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)   f = sigmoid(W_if x + b_if + W_hf h + b_hf)
              g = tanh(W_ig x + b_ig + W_hg h + b_hg)      o = sigmoid(W_io x + b_io + W_ho h + b_ho)
              c' = f * c + i * g                           h' = o * tanh(c')                  (torch.nn.LSTM, h_{-1} = c_{-1} = 0)
  state       s_t = decoder(h_t of the top layer)
"""
from typing import Dict

import numpy as np
import torch

from .gru_host import cast_params, input_slots, upstream  # noqa: F401  (the slots and the helpers are the GRU tracker's)


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """(h', c') of one cell."""
    D = h.shape[-1]
    a = x @ w_ih.T + b_ih + h @ w_hh.T + b_hh
    i, f, g, o = torch.sigmoid(a[..., :D]), torch.sigmoid(a[..., D:2 * D]), torch.tanh(a[..., 2 * D:3 * D]), torch.sigmoid(a[..., 3 * D:])
    c2 = f * c + i * g
    return o * torch.tanh(c2), c2


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, nlayers: int, carried=None) -> torch.Tensor:
    """The equations written out: states [B, T+1, S] of every position.  carried: a dict that receives "h" and "c" [nlayers, B, T+1, D],
    what every layer carries after every position."""
    B, L, D = X.shape
    h = [torch.zeros(B, D, dtype=X.dtype) for _ in range(nlayers)]
    c = [torch.zeros(B, D, dtype=X.dtype) for _ in range(nlayers)]
    out, hs, cs = [], [], []
    for t in range(L):
        x = X[:, t]
        for l in range(nlayers):
            h[l], c[l] = lstm_cell(x, h[l], c[l], p[f"lstm.weight_ih_l{l}"], p[f"lstm.weight_hh_l{l}"], p[f"lstm.bias_ih_l{l}"],
                                   p[f"lstm.bias_hh_l{l}"])
            x = h[l]
        out.append(x @ p["decoder.weight"].T + p["decoder.bias"])
        hs.append(torch.stack(h)); cs.append(torch.stack(c))
    if carried is not None:
        carried["h"], carried["c"] = torch.stack(hs, 2), torch.stack(cs, 2)
    return torch.stack(out, 1)


def states(p, users, acts, rews, nlayers, carried=None) -> torch.Tensor:
    return states_from_slots(p, input_slots(p, users, acts, rews), nlayers, carried)


def build_modules(p: Dict[str, torch.Tensor], nlayers: int):
    """(torch.nn.LSTM, torch.nn.Linear decoder) loaded BY NAME from the parameter dict, at the dict's dtype."""
    D, S = p["decoder.weight"].shape[1], p["decoder.weight"].shape[0]
    dtype = p["decoder.weight"].dtype
    lstm = torch.nn.LSTM(D, D, nlayers).to(dtype)
    lstm.load_state_dict({k[len("lstm."):]: v.detach() for k, v in p.items() if k.startswith("lstm.")}, strict=True)
    dec = torch.nn.Linear(D, S).to(dtype)
    dec.load_state_dict({"weight": p["decoder.weight"].detach(), "bias": p["decoder.bias"].detach()}, strict=True)
    return lstm, dec


def module_states(lstm, dec, X: torch.Tensor) -> torch.Tensor:
    """states [B, T+1, S] through the torch modules (nn.LSTM is time-major)."""
    out, _ = lstm(X.transpose(0, 1))
    return dec(out).transpose(0, 1)


def grads(params, users, acts, rews, lens, G, nlayers, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """d sum(states * G over the live rows) / d every parameter, by autograd at `dtype`."""
    p = cast_params(params, dtype, requires_grad=True)
    s = states(p, users, acts, rews, nlayers)
    (s * upstream(G, lens, s.shape[0], s.shape[1], dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}
