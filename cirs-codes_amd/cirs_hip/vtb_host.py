"""Host restatements for the device VirtualTaobao rollout (csrc/vtb_rollout.hip); imports without libcirs_hip.so.

tracker_states    one teacher-forced causal pass of HostStateTracker (core/host_rl.py) over a whole recorded collect, in torch with
                  autograd: the input slots are recomputed from the recorded user features, rewards and actions, so the gradient
                  reaches ffn_user and fnn_gate as well as the encoder.  A functional restatement of the post-norm
                  TransformerEncoderLayer that takes the rollout's dropout masks as given tensors (nn.Dropout cannot).  With
                  position-keyed masks one pass equals the T per-step calls of build_state.
redraw_states     the same states under the exact-redraw dropout (dropout_redraw=True): one causal pass per call c with that call's masks
                  over positions 0..c, position c kept, every call's graph retained -- what the reference's tracker in train() does.
gauss_noise       the rollout's Gaussian draw z (Box-Muller on Philox), restated in numpy bit for bit.
policy_rows       the policy of CIRS-RL-taobao.py over given states as plain tensor algebra in the dtype of its arguments (the tianshou
                  modules cast their input to float32): Net trunk, ActorProb's (mu, sigma), Independent(Normal)'s log-probability and
                  entropy, the Critic's last layer.  hidden_preactivations returns the trunk's pre-activations.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

DROP_POS, DROP_ATTN, DROP_RES1, DROP_FF, DROP_RES2 = range(5)
ACTION_DIM, USER_DIM = 27, 88


# ---- tracker ---------------------------------------------------------------------------------------------------------------
def input_slots(tracker, user, rew, act):
    """[T+1, B, D] slots: x_0 = ffn_user(user [B, 88]); x_{t+1} = sigmoid(fnn_gate([r_t, a_t])) * a_t, rew [T, B], act [T, B, 27]."""
    first = tracker.ffn_user(user).unsqueeze(0)
    if rew.shape[0] == 0:
        return first
    gate = torch.sigmoid(tracker.fnn_gate(torch.cat((rew.unsqueeze(-1), act), -1)))
    return torch.cat((first, gate * act), 0)


def _layer(lyr, h, causal, masks, nhead):
    """One post-norm TransformerEncoderLayer over h [T, B, D] with given dropout scales (None = no dropout)."""
    T, B, D = h.shape
    hd = D // nhead
    qkv = F.linear(h, lyr.self_attn.in_proj_weight, lyr.self_attn.in_proj_bias)
    q, k, v = (u.reshape(T, B, nhead, hd).permute(1, 2, 0, 3) for u in qkv.split(D, -1))      # [B, H, T, hd]
    scores = torch.matmul(q * (1.0 / math.sqrt(hd)), k.transpose(-1, -2)) + causal
    prob = torch.softmax(scores, -1)
    if masks is not None:      # ATTN element = key_pos * nhead + head -> [B, H, Tq, Tk]
        prob = prob * masks[DROP_ATTN].reshape(B, T, T, nhead).permute(0, 3, 1, 2)
    att = torch.matmul(prob, v).permute(2, 0, 1, 3).reshape(T, B, D)
    sa = lyr.self_attn.out_proj(att)
    if masks is not None:
        sa = sa * masks[DROP_RES1].transpose(0, 1)
    h1 = F.layer_norm(h + sa, (D,), lyr.norm1.weight, lyr.norm1.bias, lyr.norm1.eps)
    ff = F.relu(lyr.linear1(h1))
    if masks is not None:
        ff = ff * masks[DROP_FF].transpose(0, 1)
    ff = lyr.linear2(ff)
    if masks is not None:
        ff = ff * masks[DROP_RES2].transpose(0, 1)
    return F.layer_norm(h1 + ff, (D,), lyr.norm2.weight, lyr.norm2.bias, lyr.norm2.eps)


def states_from_slots(tracker, slots, masks=None):
    """The tracker's state at every position of slots [T, B, D] (causal): [T, B, dim_state].  masks: None (no dropout) or the scaled
    keep masks as cirs_vtb_rollout_masks returns them, env-major: {"pos": [B, T, D], (layer, site): [B, T, n_elem]} (ATTN: n_elem =
    T * nhead, element key_pos * nhead + head)."""
    T, B, D = slots.shape
    layers = tracker.transformer_encoder.layers
    nhead = layers[0].self_attn.num_heads
    h = slots * math.sqrt(tracker.dim_model) + tracker.pos_encoder.pe[:T]
    if masks is not None:
        h = h * masks["pos"].transpose(0, 1)
    causal = torch.triu(torch.full((T, T), float("-inf")), diagonal=1)
    for l, lyr in enumerate(layers):
        h = _layer(lyr, h, causal, None if masks is None else {s: masks[(l, s)] for s in (DROP_ATTN, DROP_RES1, DROP_FF, DROP_RES2)}, nhead)
    return tracker.decoder(h)


def tracker_states(tracker, user, rew, act, masks=None):
    """States [T+1, B, dim_state] of a recorded collect, with autograd: user [B, 88], rew [T, B], act [T, B, 27] (fp32)."""
    return states_from_slots(tracker, input_slots(tracker, user, rew, act), masks)


def _pad_masks(masks, n):
    """Masks of positions 0..c (states_from_slots' layout) as masks of n >= c + 1 positions: ones at the added positions and keys."""
    out = {}
    for key, m in masks.items():
        B, c1, n_elem = m.shape
        if key != "pos" and key[1] == DROP_ATTN:
            nhead = n_elem // c1
            full = torch.ones(B, n, n, nhead, dtype=m.dtype)
            full[:, :c1, :c1] = m.reshape(B, c1, c1, nhead)
            out[key] = full.reshape(B, n, n * nhead)
        else:
            out[key] = torch.cat((m, torch.ones(B, n - c1, n_elem, dtype=m.dtype)), 1)
    return out


def redraw_states(tracker, user, rew, act, masks_of_call=None):
    """States [T+1, B, dim_state] where state c is position c of a causal pass of its own with the masks masks_of_call(c) (the layout
    states_from_slots takes, positions 0..c; None = no dropout), with autograd through every call's pass.  Every pass runs over all
    T + 1 slots: position c sees positions 0..c only, so that is call c's prefix pass, and passes of one length round alike (torch
    blocks its sums by shape), which makes the result independent of the call when the masks are."""
    slots = input_slots(tracker, user, rew, act)
    n = slots.shape[0]
    return torch.stack([states_from_slots(tracker, slots, None if masks_of_call is None else _pad_masks(masks_of_call(c), n))[c]
                        for c in range(n)])


# ---- policy rows -------------------------------------------------------------------------------------------------------------
SIGMA_MIN, SIGMA_MAX = -20.0, 2.0      # ActorProb's clamp of a conditioned sigma head
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def hidden_preactivations(p, states):
    """The Net trunk's pre-activations [n, width] per hidden layer over states [n, dim_state]; p: {name: tensor} with the names of
    vtb_model.policy_tensors (trunk{i}_w / _b, torch's [out][in] layout), in the dtype of the tensors."""
    out, h = [], states
    i = 0
    while f"trunk{i}_w" in p:
        out.append(h @ p[f"trunk{i}_w"].T + p[f"trunk{i}_b"])
        h = torch.relu(out[-1])
        i += 1
    return out


def policy_rows(p, states, act, max_action=1.0, unbounded=False):
    """Per row of states [n, dim_state] and stored raw actions act [n, 27]: dict(mu, sigma [n, 27], logp, ent, value [n], pre = the trunk's
    pre-activations, sigma_pre = the sigma head's output [n, 27] or None with the free sigma_param).  ActorProb.forward, Independent(Normal)
    .log_prob / .entropy and Critic.forward as tensor algebra, in the dtype of the arguments."""
    pre = hidden_preactivations(p, states)
    h = torch.relu(pre[-1])
    mu = h @ p["mu_w"].T + p["mu_b"]
    if not unbounded:
        mu = max_action * torch.tanh(mu)
    if "sigma_w" in p:
        sigma_pre = h @ p["sigma_w"].T + p["sigma_b"]
        log_sigma = torch.clamp(sigma_pre, min=SIGMA_MIN, max=SIGMA_MAX)
    else:
        sigma_pre = None
        log_sigma = p["sigma_param"].reshape(1, -1) + torch.zeros_like(mu)
    sigma = log_sigma.exp()
    logp = (-((act - mu) ** 2) / (2.0 * sigma ** 2) - log_sigma - HALF_LOG_2PI).sum(-1)
    ent = (0.5 + HALF_LOG_2PI + log_sigma).sum(-1)
    value = (h @ p["critic_w"].T + p["critic_b"]).reshape(-1)
    return dict(mu=mu, sigma=sigma, logp=logp, ent=ent, value=value, pre=pre, sigma_pre=sigma_pre)


# ---- Gaussian noise -----------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_F = np.float32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(x, np.uint64) & _M32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & _M32, np.uint64(k1) & _M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def fmaf(a, b, c):
    """Single-rounding float32 fused multiply-add: the float64 sum of the exact product and c, corrected where its rounding to float32
    would be a double rounding (a float32 midpoint reached inexactly)."""
    a, b, c = (np.asarray(x, _F) for x in np.broadcast_arrays(a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)          # exact (24 + 24 bits)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)                           # s + err == p + c exactly
    r = s.astype(_F)
    diff = s - r.astype(np.float64)
    with np.errstate(invalid="ignore"):
        nb = np.nextafter(r, np.where(diff > 0, _F(np.inf), _F(-np.inf)).astype(_F))
        mid = (r.astype(np.float64) + nb.astype(np.float64)) * 0.5
        fix = (diff != 0) & (s == mid) & (err != 0) & (np.sign(err) == np.sign(diff))
    return np.where(fix, nb, r).astype(_F)


def u01_from_bits(x):
    return ((np.asarray(x, np.uint64) >> np.uint64(9)).astype(_F) + _F(0.5)) * _F(1.1920928955078125e-7)


def det_logf(x):
    """csrc/rng.h det_logf."""
    x = np.asarray(x, _F)
    bits = x.view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int32) - 127
    m = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(_F)
    big = m > _F(1.41421356237)
    m = np.where(big, m * _F(0.5), m).astype(_F)
    e = e + big.astype(np.int32)
    f = m - _F(1.0)
    z = f * f
    p = _F(7.0376836292e-2)
    for coef in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1,
                 -2.4999993993e-1, 3.3333331174e-1):
        p = fmaf(p, f, _F(coef))
    y = (f * z) * p
    fe = e.astype(_F)
    y = fmaf(fe, _F(-2.12194440e-4), y)
    y = fmaf(_F(-0.5), z, y)
    r = f + y
    return fmaf(fe, _F(0.693359375), r)


def _poly(z, coefs):
    p = _F(coefs[0])
    for c in coefs[1:]:
        p = fmaf(p, z, _F(c))
    return p


def gauss_noise(seed, collect_id, env_ids, ts, dims=ACTION_DIM):
    """z [n, dims] float32 of (env_ids[j], ts[j]): what cirs_vtb_rollout_noise returns (include/cirs_hip.h)."""
    env = np.asarray(env_ids, np.uint64).reshape(-1, 1)
    t = np.asarray(ts, np.uint64).reshape(-1, 1)
    dim = np.arange(dims, dtype=np.uint64).reshape(1, -1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10(dim >> np.uint64(2), env, t, np.uint64(int(collect_id) & 0xFFFFFFFF), (seed & 0xFFFFFFFF) ^ 0x47415553, seed >> 32)
    hi = (dim & np.uint64(2)) != 0
    u1 = u01_from_bits(np.where(hi, r[2], r[0]))
    u2 = u01_from_bits(np.where(hi, r[3], r[1]))
    rad = np.sqrt(_F(-2.0) * det_logf(u1)).astype(_F)
    v = u2 * _F(4.0)
    q = v.astype(np.int32)
    x = (v - q.astype(_F)) * _F(1.5707963267948966)
    z2 = x * x
    s = x * _poly(z2, (-2.5052108385e-8, 2.7557319224e-6, -1.9841269841e-4, 8.3333333333e-3, -1.6666666667e-1, 1.0))
    c = _poly(z2, (2.0876756988e-9, -2.7557319224e-7, 2.4801587302e-5, -1.3888888889e-3, 4.1666666667e-2, -0.5, 1.0))
    cs = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    sn = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    return (rad * np.where((dim & np.uint64(1)) != 0, sn, cs)).astype(_F)

