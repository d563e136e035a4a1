"""Host restatement of the GRU state tracker (csrc/gru_tracker.hip) in plain torch at a chosen dtype: the checker of every device
number.  float64 + autograd is the reference of the tests; the float32 run of the same code measures what the number format itself
costs.  Nothing here imports the device path.

The model (there is no reference text: the reference declares StateTrackerGRU and leaves it empty, core/state_tracker.py:282-289):
  slot 0      x_0 = ffn_user(Emb_user[u])
  slot k >= 1 x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k,  a_k = Emb_item[item_k],  r_k = float32(reward_k)
  cell        r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)     z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
              n = tanh(W_in x + b_in + r * (W_hn h + b_hn))  h' = (1 - z) * n + z * h          (torch.nn.GRU, h_{-1} = 0)
  state       s_t = decoder(h_t of the top layer)
"""
from typing import Dict

import numpy as np
import torch


def cast_params(params: Dict[str, torch.Tensor], dtype=torch.float64, requires_grad=False) -> Dict[str, torch.Tensor]:
    out = {k: v.detach().to("cpu", dtype).clone() for k, v in params.items()}
    if requires_grad:
        for v in out.values():
            v.requires_grad_(True)
    return out


def input_slots(p: Dict[str, torch.Tensor], users, acts, rews) -> torch.Tensor:
    """X [B, T+1, D] from users [B], acts [B, T] (ids < 0 are read as item 0: the caller ignores those positions) and rews [B, T]
    (float64 of the env, cast to float32 first like the device does)."""
    dtype = p["ffn_user.weight"].dtype
    users = torch.as_tensor(np.asarray(users)).long()
    acts = torch.as_tensor(np.asarray(acts)).long().clamp(min=0)
    r = torch.as_tensor(np.asarray(rews, dtype=np.float64)).float().to(dtype)
    x0 = p["embedding_dict.feat_user.weight"][users] @ p["ffn_user.weight"].T + p["ffn_user.bias"]
    a = p["embedding_dict.feat_item.weight"][acts]                                   # [B, T, D]
    g = torch.sigmoid(torch.cat([r.unsqueeze(-1), a], -1) @ p["fnn_gate.weight"].T + p["fnn_gate.bias"])
    return torch.cat([x0.unsqueeze(1), g * a], 1)


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh):
    D = h.shape[-1]
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = torch.sigmoid(gi[..., :D] + gh[..., :D])
    z = torch.sigmoid(gi[..., D:2 * D] + gh[..., D:2 * D])
    n = torch.tanh(gi[..., 2 * D:] + r * gh[..., 2 * D:])
    return (1 - z) * n + z * h


def states_from_slots(p: Dict[str, torch.Tensor], X: torch.Tensor, nlayers: int) -> torch.Tensor:
    """The equations written out: states [B, T+1, S] of every position."""
    B, L, D = X.shape
    h = [torch.zeros(B, D, dtype=X.dtype) for _ in range(nlayers)]
    out = []
    for t in range(L):
        x = X[:, t]
        for l in range(nlayers):
            h[l] = gru_cell(x, h[l], p[f"gru.weight_ih_l{l}"], p[f"gru.weight_hh_l{l}"], p[f"gru.bias_ih_l{l}"], p[f"gru.bias_hh_l{l}"])
            x = h[l]
        out.append(x @ p["decoder.weight"].T + p["decoder.bias"])
    return torch.stack(out, 1)


def states(p, users, acts, rews, nlayers) -> torch.Tensor:
    return states_from_slots(p, input_slots(p, users, acts, rews), nlayers)


def build_modules(p: Dict[str, torch.Tensor], nlayers: int):
    """(torch.nn.GRU, torch.nn.Linear decoder) loaded BY NAME from the parameter dict, at the dict's dtype."""
    D, S = p["decoder.weight"].shape[1], p["decoder.weight"].shape[0]
    dtype = p["decoder.weight"].dtype
    gru = torch.nn.GRU(D, D, nlayers).to(dtype)
    gru.load_state_dict({k[len("gru."):]: v.detach() for k, v in p.items() if k.startswith("gru.")}, strict=True)
    dec = torch.nn.Linear(D, S).to(dtype)
    dec.load_state_dict({"weight": p["decoder.weight"].detach(), "bias": p["decoder.bias"].detach()}, strict=True)
    return gru, dec


def module_states(gru, dec, X: torch.Tensor) -> torch.Tensor:
    """states [B, T+1, S] through the torch modules (nn.GRU is time-major)."""
    out, _ = gru(X.transpose(0, 1))
    return dec(out).transpose(0, 1)


def upstream(G, lens, B, L, dtype) -> torch.Tensor:
    """G [T+1, B, S] restricted to the live rows (env b, position p < lens[b]) as [B, T+1, S]."""
    up = torch.zeros(B, L, G.shape[-1], dtype=dtype)
    for b in range(B):
        up[b, :lens[b]] = torch.as_tensor(np.asarray(G[:lens[b], b])).to(dtype)
    return up


def grads(params, users, acts, rews, lens, G, nlayers, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """d sum(states * G over the live rows) / d every parameter, by autograd at `dtype`."""
    p = cast_params(params, dtype, requires_grad=True)
    s = states(p, users, acts, rews, nlayers)
    (s * upstream(G, lens, s.shape[0], s.shape[1], dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}
