"""Host restatement of the pooled-window state tracker (csrc/avg_tracker.hip) in plain torch at a chosen dtype: the checker of every
device number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format
itself costs.  Nothing here imports the device path.

The model (the reference has no counterpart; include/cirs_hip.h and DESIGN.md 7.4 define it):
  slots       the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  pooling     n_p = min(W, p);  m_0 = 0,  m_p = (x_{p-n_p+1} + ... + x_p) / n_p  (ascending k, one division);  h_p = x_0 + m_p
  state       s_p = decoder(h_p)
"""
from typing import Dict

import numpy as np
import torch

from .gru_host import cast_params, input_slots, upstream  # noqa: F401  (the slots and the helpers are the GRU tracker's)


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, window: int) -> torch.Tensor:
    """The equations written out: states [B, T+1, S] of every position, the window summed anew at every position."""
    B, L, D = X.shape
    assert int(window) >= 1
    out = []
    for t in range(L):
        h = X[:, 0]
        if t > 0:
            n = min(int(window), t)
            m = X[:, t - n + 1]
            for k in range(t - n + 2, t + 1):
                m = m + X[:, k]
            h = h + m / float(n)
        out.append(h @ p["decoder.weight"].T + p["decoder.bias"])
    return torch.stack(out, 1)


def states(p, users, acts, rews, window) -> torch.Tensor:
    return states_from_slots(p, input_slots(p, users, acts, rews), window)


def grads(params, users, acts, rews, lens, G, window, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """d sum(states * G over the live rows) / d every parameter, by autograd at `dtype`."""
    p = cast_params(params, dtype, requires_grad=True)
    s = states(p, users, acts, rews, window)
    (s * upstream(G, lens, s.shape[0], s.shape[1], dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}
