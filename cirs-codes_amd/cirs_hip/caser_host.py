"""Host restatement of the convolutional window state tracker (csrc/caser_tracker.hip) in plain torch at a chosen dtype: the checker of every
device number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format itself
costs.  Nothing here imports the device path.

The model (the reference has no counterpart; include/cirs_hip.h and DESIGN.md 7.5 define it), W = window, h_i = the heights:
  slots       the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  window      win_p[j] = x_{p-W+1+j} if p-W+1+j >= 1, else the zero row   (j = 0..W-1; x_0 is never in it; position 0: all zero rows)
  banks       c_{i,f,t} = bh_i[f] + sum_{j<h_i} sum_d Wh_i[f,j,d] win_p[t+j,d]  (t = 0..W-h_i);  o_{i,f} = relu(max_t c_{i,f,t})
  vertical    v_d = relu(bv + sum_j wv[j] win_p[j,d])
  fc, state   z = relu(fc([o_0 | o_1 | ... | v]));  h_p = x_0 + z;  s_p = decoder(h_p)
"""
from typing import Dict, Sequence

import numpy as np
import torch

from .gru_host import cast_params, input_slots, upstream  # noqa: F401  (the slots and the helpers are the GRU tracker's)


def heights_of(p: Dict[str, torch.Tensor]) -> Sequence[int]:
    """The banks' heights, read off the parameter shapes."""
    n = sum(1 for k in p if k.startswith("horizontal_cnn.") and k.endswith(".weight"))
    return [int(p[f"horizontal_cnn.{i}.weight"].shape[2]) for i in range(n)]


def windows(X: torch.Tensor, window: int) -> torch.Tensor:
    """[B, L, W, D]: the window of every position -- the last W item slots (x_0 excluded), zero rows in front."""
    B, L, D = X.shape
    W = int(window)
    padded = torch.cat([torch.zeros(B, W, D, dtype=X.dtype), X[:, 1:]], 1)      # index W - 1 + k holds x_k (k >= 1)
    return torch.stack([padded[:, p:p + W] for p in range(L)], 1)              # win_p[j] = padded[p + j] = x_{p-W+1+j}


def pre_activations(p: Dict[str, torch.Tensor], win: torch.Tensor):
    """The equations written out on windows [N, W, D]: (c: per bank [N, F, W-h+1], vertical pre-activation [N, D])."""
    N, W, D = win.shape
    cs = []
    for i, h in enumerate(heights_of(p)):
        wh, bh = p[f"horizontal_cnn.{i}.weight"][:, 0], p[f"horizontal_cnn.{i}.bias"]          # [F, h, D], [F]
        cs.append(torch.stack([torch.einsum("njd,fjd->nf", win[:, t:t + h], wh) + bh for t in range(W - h + 1)], -1))
    vpre = torch.einsum("j,njd->nd", p["vertical_cnn.weight"].reshape(-1), win) + p["vertical_cnn.bias"]
    return cs, vpre


def features(p: Dict[str, torch.Tensor], win: torch.Tensor):
    """(concatenation [N, F n_h + D], fc pre-activation [N, D]) of windows [N, W, D]"""
    cs, vpre = pre_activations(p, win)
    cat = torch.cat([torch.relu(c.max(-1).values) for c in cs] + [torch.relu(vpre)], -1)
    return cat, cat @ p["fc.weight"].T + p["fc.bias"]


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, window: int) -> torch.Tensor:
    """states [B, T+1, S] of every position."""
    B, L, D = X.shape
    win = windows(X, window).reshape(B * L, int(window), D)
    z = torch.relu(features(p, win)[1]).reshape(B, L, D)
    h = X[:, :1] + z
    return h @ p["decoder.weight"].T + p["decoder.bias"]


def states(p, users, acts, rews, window) -> torch.Tensor:
    return states_from_slots(p, input_slots(p, users, acts, rews), window)


def grads(params, users, acts, rews, lens, G, window, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """d sum(states * G over the live rows) / d every parameter, by autograd at `dtype`."""
    p = cast_params(params, dtype, requires_grad=True)
    s = states(p, users, acts, rews, window)
    (s * upstream(G, lens, s.shape[0], s.shape[1], dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}
