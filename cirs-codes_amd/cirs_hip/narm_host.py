"""Host restatement of the GRU-with-attention state tracker (csrc/narm_tracker.hip) in plain torch at a chosen dtype: the checker of every
device number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format
itself costs.  Nothing here imports the device path.

The model (the reference has no counterpart; include/cirs_hip.h and DESIGN.md 7.9 define it; NARM, Li et al., CIKM 2017):
  slots       the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  encoder     h_p = GRU cell(x_p, h_{p-1}), h_{-1} = 0  (gru_host.gru_cell: torch.nn.GRU(32, 32, 1), gate order r, z, n, both bias vectors)
  attention   for position p over j = 0 .. p:  q_j = A2 h_j,  a_p = A1 h_p,  alpha_{p,j} = v . sigmoid(a_p + q_j)  (no softmax)
              c_p = sum_j alpha_{p,j} h_j  (ascending j)
  read-out    m_p = Bw [h_p ; c_p]
  state       s_p = decoder(m_p)
"""
from typing import Dict

import numpy as np
import torch

from .gru_host import cast_params, gru_cell, input_slots, upstream  # noqa: F401  (the slots, the cell and the helpers are the GRU tracker's)


def hidden_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor) -> torch.Tensor:
    """The encoder: h [B, T+1, D] of every position."""
    B, L, D = X.shape
    h = torch.zeros(B, D, dtype=X.dtype)
    out = []
    for t in range(L):
        h = gru_cell(X[:, t], h, p["gru.weight_ih_l0"], p["gru.weight_hh_l0"], p["gru.bias_ih_l0"], p["gru.bias_hh_l0"])
        out.append(h)
    return torch.stack(out, 1)


def states_from_hidden(p: Dict[str, torch.Tensor], H: torch.Tensor, carried=None) -> torch.Tensor:
    """The attention, the read-out and the decoder over the hidden states H [B, T+1, D]: states [B, T+1, S] of every position."""
    A1, A2, v, Bw = p["attn.a1.weight"], p["attn.a2.weight"], p["attn.v.weight"], p["bilinear.weight"]
    Q = H @ A2.T
    if carried is not None:
        carried["h"], carried["q"] = H.detach(), Q.detach()
    out = []
    for t in range(H.shape[1]):
        a = H[:, t] @ A1.T
        alpha = torch.sigmoid(a.unsqueeze(1) + Q[:, :t + 1]) @ v.T          # [B, t+1, 1]
        c = alpha[:, 0] * H[:, 0]
        for j in range(1, t + 1):
            c = c + alpha[:, j] * H[:, j]
        m = torch.cat([H[:, t], c], -1) @ Bw.T
        out.append(m @ p["decoder.weight"].T + p["decoder.bias"])
    return torch.stack(out, 1)


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, nlayers: int = 1, carried=None) -> torch.Tensor:
    """The equations written out: states [B, T+1, S] of every position.  `carried` (a dict) receives the hidden states "h" and their
    projections "q" = A2 h, [B, T+1, D] each."""
    assert int(nlayers) == 1, "one encoder layer"
    return states_from_hidden(p, hidden_from_slots(p, X), carried)


def states(p, users, acts, rews, nlayers=1, carried=None) -> torch.Tensor:
    return states_from_slots(p, input_slots(p, users, acts, rews), nlayers, carried)


def grads(params, users, acts, rews, lens, G, nlayers=1, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """d sum(states * G over the live rows) / d every parameter, by autograd at `dtype`."""
    p = cast_params(params, dtype, requires_grad=True)
    s = states(p, users, acts, rews, nlayers)
    (s * upstream(G, lens, s.shape[0], s.shape[1], dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}
