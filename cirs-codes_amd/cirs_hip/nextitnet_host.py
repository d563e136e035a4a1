"""Host restatement of the dilated-convolution state tracker (csrc/nextitnet_tracker.hip) in plain torch at a chosen dtype: the checker of
every device number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format
itself costs.  Nothing here imports the device path.

It is written as the full-sequence definition -- F.pad + F.conv1d(dilation=) over the whole history, every position at once -- while the device
computes every position from the cone of its last R = 1 + 2 sum(dilations) item slots: two formulations, forward and backward.

The model (the reference has no counterpart; include/cirs_hip.h and DESIGN.md 7.6 define it), d_l = the dilations, kernel width 3:
  slots       the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  blocks      y^{-1}_t = x_t (t >= 1);  c^l_t = b_l + sum_{j<3} W_l[:,:,j] y^{l-1}_{t-(2-j) d_l} with y^{l-1}_s = 0 for s < 1;
              n^l_t = LayerNorm_l(c^l_t) (eps 1e-5, biased variance);  y^l_t = y^{l-1}_t + relu(n^l_t)
  state       h_p = x_0 + y^{n-1}_p (p >= 1), h_0 = x_0;  s_p = decoder(h_p)
"""
from typing import Dict, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .gru_host import cast_params, input_slots, upstream  # noqa: F401  (the slots and the helpers are the GRU tracker's)

KERNEL_SIZE = 3
EPS = 1e-5


def receptive_field(dilations: Sequence[int]) -> int:
    """item slots that reach a position: 1 + 2 sum(d_l)"""
    return 1 + (KERNEL_SIZE - 1) * sum(int(d) for d in dilations)


def blocks(p: Dict[str, torch.Tensor], items: torch.Tensor, dilations: Sequence[int], keep=None) -> torch.Tensor:
    """The stack over item slots [N, T, D] -> y^{n-1} [N, T, D], every position at once.  `keep`: a list that receives every block's
    (input y^{l-1}, pre-LayerNorm c, LayerNorm output n), [N, T, D] each."""
    y = items
    for l, d in enumerate(dilations):
        d = int(d)
        c = F.conv1d(F.pad(y.transpose(1, 2), ((KERNEL_SIZE - 1) * d, 0)), p[f"blocks.{l}.conv.weight"], p[f"blocks.{l}.conv.bias"], dilation=d)
        c = c.transpose(1, 2)
        n = F.layer_norm(c, (c.shape[-1],), p[f"blocks.{l}.ln.weight"], p[f"blocks.{l}.ln.bias"], EPS)
        if keep is not None:
            keep.append((y, c, n))
        y = y + torch.relu(n)
    return y


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, dilations: Sequence[int]) -> torch.Tensor:
    """states [B, T+1, S] of every position from the slots [B, T+1, D]."""
    y = blocks(p, X[:, 1:], dilations) if X.shape[1] > 1 else X[:, 1:]
    h = X[:, :1] + torch.cat([torch.zeros_like(X[:, :1]), y], 1)
    return h @ p["decoder.weight"].T + p["decoder.bias"]


def states(p, users, acts, rews, dilations) -> torch.Tensor:
    return states_from_slots(p, input_slots(p, users, acts, rews), dilations)


def grads(params, users, acts, rews, lens, G, dilations, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """d sum(states * G over the live rows) / d every parameter, by autograd at `dtype`."""
    p = cast_params(params, dtype, requires_grad=True)
    s = states(p, users, acts, rews, dilations)
    (s * upstream(G, lens, s.shape[0], s.shape[1], dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}
