"""Shared cases of the GRU state-tracker tests: O(1) parameters (states and gradients are then O(1) too), teacher-forced inputs with
per-env lengths, the buffer-row description, and the float32-restatement rule for a bar."""
import numpy as np
import torch

# (U, I, B, T, L, S, hot): users, items, envs, max_turn, GRU layers, dim_state, share of the actions that are ONE item
CASES = [(50, 80, 9, 12, 1, 20, 0.0), (30, 40, 5, 100, 2, 20, 0.0), (300, 500, 70, 30, 1, 20, 0.0), (30, 40, 6, 7, 2, 32, 0.0),
         (8, 9, 1, 3, 1, 20, 0.0), (8, 90, 48, 30, 1, 20, 0.6)]
STATE_BAR = 1e-5      # states, relative to their max-abs: the README's bar for the Transformer tracker's states
GRAD_BAR = 2e-4       # gradients, per tensor, relative to max|want|: the bar of tests/test_gpu_tracker_bwd.py


def gru_param_dict(U, I, seed, D=32, S=20, nlayers=1, emb_scale=0.5):
    """Embeddings ~ 0.5 N(0, 1), dense weights ~ 1 / sqrt(fan_in) (rolloutcase.tracker_param_dict's scales), keyed and ordered like
    cirs_hip.gru_tracker.gru_param_shapes."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    p = {"embedding_dict.feat_user.weight": rn(U, D, scale=emb_scale), "embedding_dict.feat_item.weight": rn(I, D, scale=emb_scale),
         "ffn_user.weight": rn(D, D, scale=0.25), "ffn_user.bias": rn(D, scale=0.1),
         "fnn_gate.weight": rn(D, D + 1, scale=0.25), "fnn_gate.bias": rn(D, scale=0.1)}
    for l in range(nlayers):
        p[f"gru.weight_ih_l{l}"] = rn(3 * D, D, scale=0.18); p[f"gru.weight_hh_l{l}"] = rn(3 * D, D, scale=0.18)
        p[f"gru.bias_ih_l{l}"] = rn(3 * D, scale=0.1); p[f"gru.bias_hh_l{l}"] = rn(3 * D, scale=0.1)
    p["decoder.weight"] = rn(S, D, scale=0.25); p["decoder.bias"] = rn(S, scale=0.1)
    return p


def teacher_inputs(U, I, B, T, hot=0.0):
    """users [B], acts [B, T], rews [B, T], lens [B] in 2 .. T (rows p < lens[b] are live; position p reads action p - 1)."""
    rng = np.random.RandomState(B * T)
    lens = rng.randint(2, T + 1, size=B)
    users = rng.randint(0, U, B); acts = rng.randint(0, I, (B, T)); rews = rng.uniform(0, 1, (B, T))
    acts[:, ::5] = acts[:, :1]      # repeated items: several rows hit the same embedding row
    if hot > 0:                     # a concentrated policy: one item owns most rows -> long segments in the ordered scatter
        acts[rng.uniform(size=acts.shape) < hot] = 7
    return users, acts, rews, lens, rng


def rows_of(lens):
    B = len(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    row_env = np.repeat(np.arange(B), lens).astype(np.int32)
    row_t = np.concatenate([np.arange(l) for l in lens]).astype(np.int32)
    return offsets, row_env, row_t


def bar_for(fixed, err32):
    """The rule of tests/test_gpu_head_precision.py: the project's bar, unless the float32 restatement itself misses it -- then
    4 x the float32 restatement's own error (computed in the test, never a constant chosen after seeing the device)."""
    return fixed if err32 <= fixed else 4.0 * err32


def device_gru_trainable(p, U, I, B, T, nlayers, S):
    from cirs_hip.gru_tracker import DeviceGruTracker, gru_param_shapes
    from cirs_hip.tracker import flat_tracker_params
    flat, views = flat_tracker_params(gru_param_shapes(U, I, 32, S, nlayers), init=p)
    trk = DeviceGruTracker(dict(views), U, I, B, T, dim_state=S, nlayers=nlayers)
    trk.enable_training(flat)
    return trk, views
