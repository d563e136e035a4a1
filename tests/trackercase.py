"""Shared cases of the Transformer state tracker's float64 tests (tests/test_tracker_case_cpu.py, tests/test_gpu_tracker_f64.py): the shapes at
which csrc/tracker.hip and csrc/tracker_bwd.hip take another path, the float64 reference (oracle/nn_oracle.py run on float64 parameters), the
conditions every case has to meet, and the bar.

Lengths are ROW counts: env b owns the rows (positions) 0 .. lens[b] - 1 of its episode, position 0 is the user's slot and position p >= 1 reads
(action, reward) of step p - 1.  lens[b] = 0 is an env without rows, lens[b] = T + 1 = max_len a full episode."""
import contextlib
import functools

import numpy as np
import torch

import nn_oracle
import rolloutcase
from grucase import rows_of  # noqa: F401  (the buffer-row description: the same function as tests/test_gpu_tracker_bwd.rows_of, importable without a GPU)

RELU_MARGIN = 1e-5      # no linear1 pre-activation of a live row comes this close to 0 in float64: 5 to 10 x what float32 loses on these O(1) sums of 32 products
FLOOR = 3e-6            # tests/vtbppogradcase.py's floor of a relative bar
GOLDEN_BAR = 1e-5       # tests/test_gpu_tracker.py::test_tracker_matches_reference_golden
DROP_SEED, DROP_TAG, DROP_ENV_BASE = 99, 17, 1000
PE = "pos_encoder.pe"


def bar_for(e32):
    """err(device, float64) <= max(4 x err(float32 restatement, float64), 3e-6): the factor of grucase.bar_for, the floor of vtbppogradcase."""
    return max(4.0 * e32, FLOOR)


# ---- which kernels a shape takes (csrc/tracker_bwd.hip: tracker_rows_impl) -----------------------------------------------------------
# The per-episode attention kernels run when  max_len <= 64  and  4 * EpGeo<NH>::bwd_floats(max_len) <= 64 KB = 16384 floats, where
#   NW = min(NH, 4), HPL = NH / NW, strip(L) = (HPL * L) | 1,
#   bwd_floats(L) = 128 L + NW (L + 1) strip(L) + 2 NH L + 2 NH L          (Q/K/V/dATT rows + the score strips + statistics + keep bits).
#   NH = 1: 128 L + (L + 1)(L | 1) + 4 L      L = 64: 12673 (fits; 65 fails the max_len <= 64 clause)                 -> 64
#   NH = 2: 128 L + 2 (L + 1)(L | 1) + 8 L    L = 62: 7936 + 7938 + 496 = 16370,  L = 63: 8064 + 8064 + 504 = 16632    -> 62
#   NH = 4: 128 L + 4 (L + 1)(L | 1) + 16 L   L = 47: 6016 + 9024 + 752 = 15792,  L = 48: 6144 + 9604 + 768 = 16516    -> 47
#   NH = 8: 128 L + 4 (L + 1)(2L | 1) + 32 L  L = 35: 4480 + 10224 + 1120 = 15824, L = 36: 4608 + 10804 + 1152 = 16564 -> 35
EP_LIMIT = {1: 64, 2: 62, 4: 47, 8: 35}
PREFIX_ONE_LAUNCH_MAX_LEN = 32      # cirs_tracker_prefix_states: one launch (prefix_env_kernel) up to here, the multi-launch pass beyond


def ep_bwd_floats(nhead, L):
    nw = min(nhead, 4)
    hpl = nhead // nw
    return 128 * L + nw * (L + 1) * ((hpl * L) | 1) + 2 * nhead * L + 2 * nhead * L


def takes_episode_kernels(nhead, max_len):
    return max_len <= 64 and 4 * ep_bwd_floats(nhead, max_len) <= 64 * 1024


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _case(U, I, T, lens, *, nhead=4, nlayers=2, S=20, seed=3, hot=0.0, p=0.0, paths=("fused",), special=False, modes=False, pad=0, nudges=(), claims=None):
    """lens: rows per env.  seed: the FINAL seed (the first of seed0 + 1000 k that meets the ReLU condition).  nudges: (layer, unit, delta) added to
    linear1.bias where a case has too many rows for a clean seed.  paths: "fused" = the default dispatch, "rows" = CIRS_TRACKER_ATTN_ROWS=1.
    special: also backward(last_rows_only=True) and prefix_states.  modes: also the skip / item -1 replays.  pad: spare columns of the state buffer.
    claims: the property the case's name promises (test_tracker_case_cpu.py asserts it)."""
    return dict(U=U, I=I, T=T, lens=np.asarray(lens, dtype=np.int64), nhead=nhead, nlayers=nlayers, S=S, seed=seed, hot=hot, p=p, paths=tuple(paths),
                special=special, modes=modes, pad=pad, nudges=tuple(nudges), claims=dict(claims or {}))


def _hot_lens():
    return np.random.RandomState(48 * 30).randint(2, 31, size=48)      # the lengths of test_gpu_tracker_bwd's (8, 90, 48, 30, 4, 0.6)


BOTH = ("fused", "rows")
CASES = {
    # 1. smallest: the user slot alone (no action is read), then one action
    "R1": _case(30, 40, 1, [1], claims=dict(R=1, B=1, max_len=2)),
    "R2": _case(30, 40, 1, [2], claims=dict(R=2, B=1, max_len=2, full=True)),
    # 2. row-count edges of the 32-row tiles and of the per-row attention's 4 rows per workgroup
    "R31": _case(50, 80, 12, [13, 5, 12, 1], paths=BOTH, claims=dict(R=31)),
    "R32": _case(50, 80, 12, [13, 6, 12, 1], paths=BOTH, claims=dict(R=32)),
    "R33": _case(50, 80, 12, [13, 7, 12, 1], paths=BOTH, modes=True, claims=dict(R=33, min_len=1)),
    # 3. episode-length edges: the per-episode kernels' first 32 rows and their paired queries; an env without rows
    "len-edges": _case(60, 90, 36, [0, 1, 2, 31, 32, 33, 36, 37], paths=BOTH, special=True,
                       claims=dict(has=(0, 1, 2, 31, 32, 33, 36, 37), min_max_len=34, full=True, ep=True)),
    # 4. the per-episode limit of every head count, and one past it
    "ep-nh1-L64": _case(40, 60, 63, [64, 30, 3, 41], nhead=1, paths=BOTH, special=True, claims=dict(max_len=64, ep=True, full=True)),
    "ep-nh1-L65": _case(40, 60, 64, [65, 30, 3, 41], nhead=1, claims=dict(max_len=65, ep=False, full=True)),
    "ep-nh2-L62": _case(40, 60, 61, [62, 30, 3, 41], nhead=2, seed=1003, paths=BOTH, special=True, claims=dict(max_len=62, ep=True, full=True)),
    "ep-nh2-L63": _case(40, 60, 62, [63, 30, 3, 41], nhead=2, seed=1003, claims=dict(max_len=63, ep=False, full=True)),
    "ep-nh4-L47": _case(40, 60, 46, [47, 23, 3, 30], nhead=4, paths=BOTH, special=True, modes=True, claims=dict(max_len=47, ep=True, full=True, min_len=1)),
    "ep-nh4-L48": _case(40, 60, 47, [48, 23, 3, 30], nhead=4, claims=dict(max_len=48, ep=False, full=True)),
    "ep-nh8-L35": _case(40, 60, 34, [35, 17, 3, 22], nhead=8, paths=BOTH, special=True, claims=dict(max_len=35, ep=True, full=True)),
    "ep-nh8-L36": _case(40, 60, 35, [36, 17, 3, 22], nhead=8, claims=dict(max_len=36, ep=False, full=True)),
    # 5. layer counts other than 2 through the general backward (and, with 3, the two special passes)
    "layers1": _case(40, 60, 14, [15, 3, 14, 9, 11, 8], nlayers=1, claims=dict(nlayers=1, R=60)),
    "layers3": _case(40, 60, 14, [15, 3, 14, 9, 0, 11, 8], nlayers=3, special=True, claims=dict(nlayers=3, R=60, has=(0,))),
    # 6. state widths other than 20, written at out_stride = dim_state + 3
    "S1": _case(30, 40, 9, [10, 4, 1, 7, 9], S=1, pad=3, claims=dict(S=1, pad=3)),
    "S7": _case(30, 40, 9, [10, 4, 1, 7, 9], S=7, pad=3, claims=dict(S=7, pad=3)),
    "S32": _case(30, 40, 9, [10, 4, 1, 7, 9], S=32, pad=3, claims=dict(S=32, pad=3)),
    # 9. dropout: one ragged row count, one per-episode limit
    "R33-p0.3": _case(50, 80, 12, [13, 7, 12, 1], p=0.3, paths=BOTH, claims=dict(R=33, p=0.3)),
    "ep-nh4-L47-p0.1": _case(40, 60, 46, [47, 23, 3, 30], nhead=4, p=0.1, seed=1003, paths=BOTH, special=True, claims=dict(max_len=47, ep=True, full=True, p=0.1)),
    # 10. a concentrated policy: embedding-gradient segments that span several 64-row sub-runs of the sorted scatter
    "hot": _case(8, 90, 30, _hot_lens(), hot=0.6, paths=BOTH, claims=dict(min_R=700, hot_rows=200)),
    # 11. prefix_states' own switch (one launch up to max_len 32)
    "prefix-L32": _case(40, 60, 31, [32, 0, 5, 1, 31, 17], special=True, claims=dict(max_len=32, full=True, has=(0,))),
    "prefix-L33": _case(40, 60, 32, [33, 0, 5, 1, 32, 17], special=True, claims=dict(max_len=33, full=True, has=(0,))),
}
MODE_CASES = [k for k, c in CASES.items() if c["modes"]]
SPECIAL_CASES = [k for k, c in CASES.items() if c["special"]]
BACKWARD_RUNS = [(k, path) for k, c in CASES.items() for path in c["paths"]]


def inputs(c):
    """Parameters (float32, the values the device holds), users [B], acts [B, T], rews [B, T] (float64: the device casts to float32, as
    nn_oracle.tracker_inputs does), the upstream gradients G [T + 1, B, S] and g_last [B, S]."""
    U, I, T, S, B = c["U"], c["I"], c["T"], c["S"], len(c["lens"])
    p = rolloutcase.tracker_param_dict(U, I, T, seed=c["seed"], S=S, nlayers=c["nlayers"])
    for layer, unit, delta in c["nudges"]:
        p[f"transformer_encoder.layers.{layer}.linear1.bias"][unit] += delta
    rng = np.random.RandomState(c["seed"] + 7)
    users = rng.randint(0, U, B); acts = rng.randint(0, I, (B, T)); rews = rng.uniform(0, 1, (B, T))
    acts[:, ::5] = acts[:, :1]      # repeated items: several rows hit the same embedding row
    if c["hot"] > 0:
        acts[rng.uniform(size=acts.shape) < c["hot"]] = 7
    G = rng.normal(size=(T + 1, B, S)).astype(np.float32)
    g_last = rng.normal(size=(B, S)).astype(np.float32)
    return p, users, acts, rews, G, g_last


def dropout_of(c):
    if c["p"] == 0:
        return None
    return dict(p=c["p"], key=nn_oracle.dropout_key(DROP_SEED, DROP_TAG), envs=np.arange(len(c["lens"])) + DROP_ENV_BASE)


@contextlib.contextmanager
def relu_inputs():
    """Records what nn_oracle.tracker_forward_all hands to torch.relu: the linear1 pre-activations [B, L, d_hid], one entry per layer."""
    seen, orig = [], torch.relu

    def spy(x):
        seen.append(x.detach().double())
        return orig(x)
    torch.relu = spy
    try:
        yield seen
    finally:
        torch.relu = orig


def live_mask(lens, T):
    return np.arange(T + 1)[None, :] < np.asarray(lens)[:, None]


def restatement(c, p, users, acts, rews, G, g_last, dtype, want_grads=True):
    """nn_oracle's forward on parameters cast to `dtype` -> states [B, T + 1, S] (numpy float64), the gradient of (states * up).sum() per tensor for
    up = G on the live rows, the same for up = g_last on every env's last row (special cases), the smallest |linear1 pre-activation| of a live row."""
    lens, T, B = c["lens"], c["T"], len(c["lens"])
    q = {k: v.to(dtype).clone() for k, v in p.items()}
    names = [k for k in q if k != PE]
    for k in names:
        q[k].requires_grad_(want_grads)
    with relu_inputs() as pre:
        st = nn_oracle.tracker_forward_all(q, nn_oracle.tracker_inputs(q, users, acts, rews), c["nhead"], c["nlayers"], dropout=dropout_of(c))
    assert st.dtype == dtype and len(pre) == c["nlayers"]
    live = torch.as_tensor(live_mask(lens, T))
    out = dict(states=st.detach().double().numpy(), margin=min(float(x[live].abs().min()) for x in pre))
    if not want_grads:
        return out
    up, up_last = torch.zeros_like(st), torch.zeros_like(st)
    for b in range(B):
        up[b, :lens[b]] = torch.as_tensor(G[:lens[b], b]).to(dtype)
        if lens[b] > 0:
            up_last[b, lens[b] - 1] = torch.as_tensor(g_last[b]).to(dtype)
    g = torch.autograd.grad((st * up).sum(), [q[k] for k in names], retain_graph=c["special"])
    out["grads"] = {k: v.double().numpy() for k, v in zip(names, g)}
    if c["special"]:
        g = torch.autograd.grad((st * up_last).sum(), [q[k] for k in names])
        out["grads_last"] = {k: v.double().numpy() for k, v in zip(names, g)}
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per case and shared, never modified: inputs, the float64 states / gradients, and e32 = the float32 restatement's own distance
    from them (states: relative to the largest live state; gradients: per tensor, relative to max|want|)."""
    c = CASES[name]
    p, users, acts, rews, G, g_last = inputs(c)
    r64 = restatement(c, p, users, acts, rews, G, g_last, torch.float64)
    r32 = restatement(c, p, users, acts, rews, G, g_last, torch.float32)
    live = live_mask(c["lens"], c["T"])
    ref = dict(case=c, name=name, p=p, users=users, acts=acts, rews=rews, G=G, g_last=g_last, lens=c["lens"], live=live, s64=r64["states"],
               margin=r64["margin"], s_scale=float(np.abs(r64["states"][live]).max()), g64=r64["grads"],
               e32={k: _rel(r32["grads"][k], r64["grads"][k]) for k in r64["grads"]})
    ref["s_e32"] = float(np.abs(r32["states"][live] - r64["states"][live]).max() / ref["s_scale"])
    if c["special"]:
        ref["g64_last"] = r64["grads_last"]
        ref["e32_last"] = {k: _rel(r32["grads_last"][k], r64["grads_last"][k]) for k in r64["grads_last"]}
    return ref


def touched(ref):
    """Embedding rows that occur in a live row: users of envs with a row, items read by positions 1 .. lens - 1."""
    lens, acts = ref["lens"], ref["acts"]
    items = [acts[b, :lens[b] - 1] for b in range(len(lens)) if lens[b] > 1]
    return np.unique(ref["users"][lens > 0]), np.unique(np.concatenate(items)) if items else np.zeros(0, np.int64)


# ---- the device side -----------------------------------------------------------------------------------------------------------------
def device_tracker(c, p):
    """test_gpu_tracker_bwd.device_tracker_trainable at any dim_state / layer count, with the case's dropout key."""
    from cirs_hip.tracker import DeviceTracker, flat_tracker_params, tracker_param_shapes
    U, I, T, S, nl, B = c["U"], c["I"], c["T"], c["S"], c["nlayers"], len(c["lens"])
    flat, views = flat_tracker_params(tracker_param_shapes(U, I, dim_state=S, nlayers=nl), init=p)
    trk = DeviceTracker({**views, PE: p[PE].float().cuda().contiguous()}, U, I, B, T, dim_state=S, nhead=c["nhead"], nlayers=nl)
    trk.enable_training(flat)
    if c["p"] > 0:
        trk.set_dropout(c["p"])
        trk.set_dropout_key(DROP_SEED, DROP_TAG, DROP_ENV_BASE)
    return trk


def replay(trk, users, acts, rews, lens, mode, pad=0):
    """slotcase.replay in this tracker's terms (an env may have no row at all; the state buffer may have spare columns): reset / init /
    step, teacher-forced, env b gets positions 0 .. lens[b] - 1.  Finished envs are dropped through env_ids (the live ones only, in descending order)
    or stay in the batch and are marked (skip on even steps, item -1 on odd ones).  Every call writes into a NaN-filled buffer of S + pad columns:
    rows of finished envs and the spare columns must keep the NaN.  Returns states [B, T + 1, S], NaN where no state was produced."""
    B, T = acts.shape
    S = trk.dim_state
    lens = np.asarray(lens)
    out = np.full((B, T + 1, S), np.nan, np.float32)
    dev = lambda ids: torch.as_tensor(ids.astype(np.int32)).cuda()  # noqa: E731
    new = lambda n: torch.full((n, S + pad), float("nan"), device="cuda")  # noqa: E731
    trk.reset()
    started = np.where(lens > 0)[0]
    assert mode == "env_ids" or len(started) == B, "the skip / item -1 forms keep every env in the batch: every env needs a row"
    ids = started[::-1].copy() if mode == "env_ids" else started
    buf = new(len(ids))
    trk.init(torch.as_tensor(users[ids]), env_ids=dev(ids) if mode == "env_ids" else None, out=buf, out_stride=S + pad)
    got = buf.cpu().numpy()
    assert np.isnan(got[:, S:]).all(), "init wrote a spare column of state_out"
    out[ids, 0] = got[:, :S]
    for t in range(T):
        live = np.where(lens > t + 1)[0]
        if len(live) == 0:
            break
        if mode == "env_ids":
            ids = live[::-1].copy()
            buf = new(len(ids))
            trk.step(torch.as_tensor(acts[ids, t]), torch.as_tensor(rews[ids, t]), env_ids=dev(ids), out=buf, out_stride=S + pad)
            got = buf.cpu().numpy()
            out[ids, t + 1] = got[:, :S]
        else:
            dead = lens <= t + 1
            buf = new(B)
            if t % 2 == 0:
                trk.step(torch.as_tensor(acts[:, t]), torch.as_tensor(rews[:, t]), skip=torch.as_tensor(dead.astype(np.uint8)).cuda(), out=buf,
                         out_stride=S + pad)
            else:
                trk.step(torch.as_tensor(np.where(dead, -1, acts[:, t])), torch.as_tensor(rews[:, t]), out=buf, out_stride=S + pad)
            got = buf.cpu().numpy()
            assert np.isnan(got[dead]).all(), "a finished env's row of state_out was written"
            out[:, t + 1] = got[:, :S]
        assert np.isnan(got[:, S:]).all(), "step wrote a spare column of state_out"
    return out


def backward_args(ref):
    """(users, traj, row_env, row_t, offsets, lens, n_rows) of DeviceTracker.backward for the case's rows."""
    from cirs_hip.rollout import Trajectory
    c, lens, acts = ref["case"], ref["lens"], ref["acts"]
    B, T = acts.shape
    traj = Trajectory(B, T, c["S"], "cuda")
    a = np.where(np.arange(T)[None, :] < lens[:, None] - 1, acts, -1)      # position p reads action p - 1: lens - 1 actions per env
    traj.act.copy_(torch.as_tensor(a.T.copy())); traj.rew.copy_(torch.as_tensor(ref["rews"].T.copy()))
    offsets, row_env, row_t = rows_of(lens)
    d = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    return torch.as_tensor(ref["users"]), traj, d(row_env), d(row_t), d(offsets), d(lens.astype(np.int32)), int(lens.sum())
