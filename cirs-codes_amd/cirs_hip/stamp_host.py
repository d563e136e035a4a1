"""Host restatement of the attention-pool state tracker (csrc/stamp_tracker.hip) in plain torch at a chosen dtype: the checker of every
device number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format
itself costs.  Nothing here imports the device path.

The model (the reference has no counterpart; include/cirs_hip.h and DESIGN.md 7.7 define it; STAMP, Liu et al., KDD 2018):
  slots       the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  window      n_p = min(W, p), k = p - n_p + 1 .. p;  m_s = (x_{p-n_p+1} + ... + x_p) / n_p  (ascending k, one division);  m_t = x_p
  attention   c = W2 m_t + W3 m_s + b_a;  e_k = w0 . sigmoid(W1 x_k + c)  (no softmax);  m_a = sum_k e_k x_k  (ascending k)
  read-out    h_s = tanh(A m_a + b_A),  h_t = tanh(B m_t + b_B);  h_p = x_0 + h_s * h_t,  h_0 = x_0
  state       s_p = decoder(h_p)
"""
from typing import Dict

import numpy as np
import torch

from .gru_host import cast_params, input_slots, upstream  # noqa: F401  (the slots and the helpers are the GRU tracker's)

MAX_WINDOW = 16


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, window: int) -> torch.Tensor:
    """The equations written out: states [B, T+1, S] of every position, the window read anew at every position."""
    B, L, D = X.shape
    assert 1 <= int(window) <= MAX_WINDOW
    W1, W2, W3, b_a, w0 = p["attn.w1.weight"], p["attn.w2.weight"], p["attn.w3.weight"], p["attn.bias"], p["attn.w0.weight"]
    out = []
    for t in range(L):
        h = X[:, 0]
        if t > 0:
            n = min(int(window), t)
            m_s = X[:, t - n + 1]
            for k in range(t - n + 2, t + 1):
                m_s = m_s + X[:, k]
            m_s = m_s / float(n)
            m_t = X[:, t]
            c = m_t @ W2.T + m_s @ W3.T + b_a
            m_a = None
            for k in range(t - n + 1, t + 1):
                e = torch.sigmoid(X[:, k] @ W1.T + c) @ w0.T          # [B, 1]
                m_a = e * X[:, k] if m_a is None else m_a + e * X[:, k]
            h_s = torch.tanh(m_a @ p["mlp_a.weight"].T + p["mlp_a.bias"])
            h_t = torch.tanh(m_t @ p["mlp_b.weight"].T + p["mlp_b.bias"])
            h = h + h_s * h_t
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
