"""Host restatement of the filter-MLP state tracker (csrc/fmlp_tracker.hip) in plain torch at a chosen dtype: the checker of every device
number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format itself costs.
Nothing here imports the device path.  The filter is written in the frequency domain (torch.fft.rfft / irfft over the tile's rows), the
device works in the time domain (a circular convolution with h = irfft(w, n=W)): every device check is between two formulations.

The model (the reference has no counterpart; include/cirs_hip.h and DESIGN.md 7.10 define it; FMLP-Rec, Zhou et al., WWW 2022):
  slots     the GRU tracker's (gru_host.input_slots): x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
  tile      Y[i] = x_{p-W+1+i} if p-W+1+i >= 1 else 0, i = 0 .. W-1   (left zero padding at the input of layer 0 only)
  layer l   w = view_as_complex(layers.l.filter.complex_weight);  F = irfft(rfft(Y, dim=rows, norm="ortho") * w, n=W, dim=rows, norm="ortho")
            A = LayerNorm(Y + F) (layers.l.filter.ln);  M = dense_2(gelu(dense_1(A))) (erf GELU);  Y = LayerNorm(A + M) (layers.l.ffn.ln)
  state     h_p = x_0 + Y[W-1] (p >= 1), h_0 = x_0;  s_p = decoder(h_p)
"""
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from .gru_host import cast_params, input_slots, upstream  # noqa: F401  (the slots and the helpers are the GRU tracker's)

MAX_WINDOW, MAX_LAYERS, HIDDEN, EPS = 16, 2, 128, 1e-5


def n_layers(p) -> int:
    return sum(1 for k in p if k.endswith(".filter.complex_weight"))


def layer(p: Dict[str, torch.Tensor], l: int, Y: torch.Tensor) -> torch.Tensor:
    """One filter + feed-forward layer over tiles Y [..., W, D] (the rows are dim -2)."""
    W, D = Y.shape[-2], Y.shape[-1]
    pre = f"layers.{l}."
    w = torch.view_as_complex(p[pre + "filter.complex_weight"])                       # [W//2+1, D]
    Fq = torch.fft.irfft(torch.fft.rfft(Y, dim=-2, norm="ortho") * w, n=W, dim=-2, norm="ortho")
    A = F.layer_norm(Y + Fq, (D,), p[pre + "filter.ln.weight"], p[pre + "filter.ln.bias"], EPS)
    U = A @ p[pre + "ffn.dense_1.weight"].T + p[pre + "ffn.dense_1.bias"]
    M = F.gelu(U) @ p[pre + "ffn.dense_2.weight"].T + p[pre + "ffn.dense_2.bias"]
    return F.layer_norm(A + M, (D,), p[pre + "ffn.ln.weight"], p[pre + "ffn.ln.bias"], EPS)


def tile_of(X: torch.Tensor, t: int, window: int) -> torch.Tensor:
    """The tile of position t >= 1 from slots X [B, L, D]: rows x_{t-W+1} .. x_t, zero rows where the slot index is < 1."""
    B, _, D = X.shape
    first = t - window + 1
    rows = X[:, max(first, 1):t + 1]
    if first < 1:
        rows = torch.cat([torch.zeros((B, 1 - first, D), dtype=X.dtype), rows], 1)
    return rows


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, window: int) -> torch.Tensor:
    """The equations written out: states [B, T+1, S] of every position, the tile read anew at every position."""
    B, L, D = X.shape
    W, nl = int(window), n_layers(p)
    assert 1 <= W <= MAX_WINDOW and 1 <= nl <= MAX_LAYERS
    out = []
    for t in range(L):
        h = X[:, 0]
        if t > 0:
            Y = tile_of(X, t, W)
            for l in range(nl):
                Y = layer(p, l, Y)
            h = h + Y[:, W - 1]
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
