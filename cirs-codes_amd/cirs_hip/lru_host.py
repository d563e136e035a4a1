"""Host restatement of the linear-recurrence state tracker (csrc/lru_tracker.hip) in plain torch at a chosen dtype, in real arithmetic: the
checker of every device number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number
format itself costs.  Nothing here imports the device path.

The model (the reference has no counterpart; include/cirs_hip.h and DESIGN.md 7.11 define it; the recurrence of LRU, Orvieto et al., ICML
2023, as LRURec, Yue et al., 2023, uses it; a complex number is a (re, im) pair):
  slots       the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  lambda      = exp(-exp(nu_log)) (cos phi, sin phi), phi = exp(theta_log);  gamma = exp(gamma_log)
  input       v_p = W_in x_p + b_in  (rows 0..31 the real part, 32..63 the imaginary part);  u_p = gamma * v_p (both parts)
  recurrence  h_re' = lr h_re - li h_im + u_re,  h_im' = lr h_im + li h_re + u_im,  h_{-1} = 0
  read-out    y_p = W_out [h_re ; h_im] + b_out;  z_p = LayerNorm(y_p + x_p)  (lru.ln)
  block       m_p = LayerNorm(z_p + W2 gelu(W1 z_p + b1) + b2)  (ffn.ln, the exact GELU)
  state       s_p = decoder(m_p)
"""
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from .fmlp_host import EPS
from .gru_host import cast_params, input_slots, upstream  # noqa: F401  (the slots and the helpers are the GRU tracker's)

HIDDEN = 128


def eigenvalues(p: Dict[str, torch.Tensor]):
    """(lambda_re, lambda_im, gamma), [D] each, from the three log vectors"""
    mod, phi = torch.exp(-torch.exp(p["lru.nu_log"])), torch.exp(p["lru.theta_log"])
    return mod * torch.cos(phi), mod * torch.sin(phi), torch.exp(p["lru.gamma_log"])


def hidden_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor):
    """The recurrence: (h_re, h_im), [B, T+1, D] each, of every position."""
    B, L, D = X.shape
    lr, li, ga = eigenvalues(p)
    V = X @ p["lru.in_proj.weight"].T + p["lru.in_proj.bias"]
    u_re, u_im = ga * V[..., :D], ga * V[..., D:]
    h_re, h_im = torch.zeros(B, D, dtype=X.dtype), torch.zeros(B, D, dtype=X.dtype)
    re, im = [], []
    for t in range(L):
        h_re, h_im = lr * h_re - li * h_im + u_re[:, t], lr * h_im + li * h_re + u_im[:, t]
        re.append(h_re); im.append(h_im)
    return torch.stack(re, 1), torch.stack(im, 1)


def states_from_hidden(p: Dict[str, torch.Tensor], X: torch.Tensor, h_re: torch.Tensor, h_im: torch.Tensor) -> torch.Tensor:
    """The read-out, the two LayerNorms, the feed-forward block and the decoder over every position at once."""
    D = X.shape[-1]
    Y = torch.cat([h_re, h_im], -1) @ p["lru.out_proj.weight"].T + p["lru.out_proj.bias"]
    Z = F.layer_norm(Y + X, (D,), p["lru.ln.weight"], p["lru.ln.bias"], EPS)
    U = Z @ p["ffn.dense_1.weight"].T + p["ffn.dense_1.bias"]
    Fo = F.gelu(U) @ p["ffn.dense_2.weight"].T + p["ffn.dense_2.bias"]
    M = F.layer_norm(Z + Fo, (D,), p["ffn.ln.weight"], p["ffn.ln.bias"], EPS)
    return M @ p["decoder.weight"].T + p["decoder.bias"]


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, nlayers: int = 1, kept=None) -> torch.Tensor:
    """The equations written out: states [B, T+1, S] of every position.  `kept` (a dict) receives the hidden state of every (env, position):
    "h_re" and "h_im", [B, T+1, D] each."""
    assert int(nlayers) == 1, "one recurrence layer"
    h_re, h_im = hidden_from_slots(p, X)
    if kept is not None:
        kept["h_re"], kept["h_im"] = h_re.detach(), h_im.detach()
    return states_from_hidden(p, X, h_re, h_im)


def states(p, users, acts, rews, nlayers=1, kept=None) -> torch.Tensor:
    return states_from_slots(p, input_slots(p, users, acts, rews), nlayers, kept)


def grads(params, users, acts, rews, lens, G, nlayers=1, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """d sum(states * G over the live rows) / d every parameter, by autograd at `dtype`."""
    p = cast_params(params, dtype, requires_grad=True)
    s = states(p, users, acts, rews, nlayers)
    (s * upstream(G, lens, s.shape[0], s.shape[1], dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}
