"""Shared cases and the float64 reference of the VirtualTaobao PPO update's gradient tests (tests/test_gpu_vtb_ppo_grads.py,
tests/test_vtb_ppo_gradcase_cpu.py): csrc/vtb_learn.hip from vtb_learn_forward_kernel to vtb_learn_tracker_adam_kernel, driven through
cirs_hip.vtb_learn.DeviceVtbLearner on a fabricated trajectory.

A case is a model (tracker, ActorProb / Critic over one Net), a trajectory [T, B] with ragged episode lengths (NaN in every float column behind
an episode's end, so a read past it shows), a list of buffer rows, the four per-row columns the returns stage would have produced (v_s, adv,
returns, logp_old: the test overwrites the device's with them) and one row permutation per pass.  The columns place rows on every branch of the
row objective: logp_old is the current policy's log-probability shifted by the logarithm of a chosen ratio, v_s the current value shifted by a
chosen amount.  The builder keeps every row and position KINK away from every branch point, by a deterministic adjustment (a hidden unit's bias
for a ReLU, + 0.01 on logp_old / v_s for the objective), never by leaving a row out.

The reference: vtb_host.tracker_states / redraw_states on a copy of the tracker in the evaluation's dtype, vtb_host.policy_rows, ppo_terms below
(test_vtb_ppo_gradcase_cpu.py holds it to core.host_rl.ppo_objective, which rounds the ratio to float32 and so cannot serve itself).  Cases come
from fixed seeds (no golden file)."""
import copy
import functools
import types

import numpy as np
import torch

from cirs_hip import vtb_host
from cirs_hip.vtb_host import ACTION_DIM, USER_DIM

KINK = 1e-4            # the least distance of any row / position from any branch point (float64)
MIN_CLASS_ROWS = 2
HALF_ULP = 2.0 ** -24
SCRIPT = dict(discount_factor=0.95, eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, reward_normalization=1, advantage_normalization=1,
              recompute_advantage=0, value_clip=1, gae_lambda=0.95, dual_clip=None)      # CIRS-RL-taobao.py's (tests/test_gpu_vtb_learn.py SCRIPT)
PLAIN = dict(ent_coef=0.01, value_clip=0, advantage_normalization=0)
DUAL = dict(dual_clip=2.0)
DROP_SEED, DROP_BASE = 0x5EED0123456789, 1000
ADAM_K, ADAM_KT = 7, 5      # step counts before the Adam run: heads 7 (trunk 14), tracker 5

SMALL = (1, 4, 2)           # B = 3, T = 4: one step, a full unfinished episode, a short one
# lens of B = 5, T = 30 whose sums sit on the minibatch kernel's 64 rows per workgroup (4 waves, one row per wave at a time)
WG = {63: (30, 1, 17, 2, 13), 64: (30, 30, 1, 1, 2), 65: (30, 5, 28, 1, 1), 129: (30, 30, 30, 30, 9)}


def _case(lens, T, seed, unfinished=(), n_draw=None, batch_size=None, repeat=1, dropout=0.0, redraw=False, adam=False, hyper=None, nhead=3,
          d_hid=128, nlayers=2, dim_state=20, hidden=(64, 64), conditioned_sigma=False, unbounded=False, classes="all"):
    return dict(lens=tuple(lens), T=T, seed=seed, unfinished=tuple(unfinished), n_draw=n_draw, batch_size=batch_size, repeat=repeat,
                dropout=dropout, redraw=redraw, adam=adam, hyper=dict(SCRIPT, **(hyper or {})), nhead=nhead, d_hid=d_hid, nlayers=nlayers,
                dim_state=dim_state, hidden=tuple(hidden), conditioned_sigma=conditioned_sigma, unbounded=unbounded, classes=classes)


def _ragged(B, T, seed):
    r = np.random.RandomState(seed)
    lens = r.randint(1, T + 1, B)
    lens[:3] = (1, T, T)      # the shortest episode, a full unfinished one, a full finished one
    return tuple(int(x) for x in lens)


# classes: which branch classes the builder must find MIN_CLASS_ROWS rows of: "all" = both sides of the ratio clip with both signs of the
# advantage, ties, and (value clip) both binding sides and the free error winning, (dual clip) the floor winning on a negative advantage;
# "few" (7 rows): ties, rows outside the clip on its gradient-blocking side and on its passing side.  (a seed is a plain number unless the case it gives misses a class count or a
# margin no adjustment reaches; then it is the next of seed + 1000 k that meets them)
CASES = {
    "one-row": _case((1,), 1, 11, hyper=dict(advantage_normalization=0), classes=None),      # the std of one row is NaN on both sides
    "ragged-small": _case(SMALL, 4, 12, unfinished=(1,), adam=True, classes="few"),
    "rows63": _case(WG[63], 30, 13, unfinished=(0,)),                                       # one workgroup, its last wave turn short
    "rows64-plain": _case(WG[64], 30, 14, unfinished=(0,), hyper=PLAIN),                    # exactly one workgroup
    "rows65-dual": _case(WG[65], 30, 15, unfinished=(0,), hyper=DUAL, adam=True),           # a second workgroup of one row
    "rows129-drop": _case(WG[129], 30, 16, unfinished=(0, 2), dropout=0.1),                 # three workgroups, the last of one row
    "rows129-split": _case(WG[129], 30, 17, unfinished=(1,), batch_size=64, repeat=2, hyper=dict(DUAL, ent_coef=0.01)),      # 64 + 65 rows, twice
    "dup70-of-40": _case((10, 3, 10, 1, 16), 16, 18, unfinished=(4,), n_draw=70, dropout=0.1, adam=True),
    "csigma-h128-S7": _case(SMALL, 4, 2019, unfinished=(1,), conditioned_sigma=True, hidden=(128,), dim_state=7, nlayers=1, nhead=1, d_hid=5,
                            hyper=dict(ent_coef=0.01), classes="few"),
    "unbounded-h3-S128": _case(SMALL, 4, 20, unfinished=(1,), unbounded=True, hidden=(24, 40, 8), dim_state=128, nlayers=4, nhead=9, d_hid=130,
                               hyper=DUAL, classes="few"),
    "nhead27-drop": _case(SMALL, 4, 1021, unfinished=(1,), nhead=27, dropout=0.1, hyper=PLAIN, classes="few"),
    "redraw-small": _case(SMALL, 4, 22, unfinished=(1,), dropout=0.1, redraw=True, classes="few"),
    "redraw-B130": _case(_ragged(130, 2, 23), 2, 23, unfinished=(1,), dropout=0.1, redraw=True, batch_size=64, repeat=2),      # 7 workgroups per env
    "redraw-B200": _case(_ragged(200, 6, 24), 6, 24, unfinished=(1,), dropout=0.1, redraw=True, hyper=DUAL),      # 5 per env: two calls in some
}
ADAM_CASES = tuple(k for k, c in CASES.items() if c["adam"])


def hyper_of(kw):
    """PpoHyper of HostPPOPolicy's keywords (its constructor's mapping; the GPU test compares with the policy's own)."""
    from core.host_rl import PpoHyper
    return PpoHyper(clip=kw["eps_clip"], dual=kw["dual_clip"], clip_value=bool(kw["value_clip"]), whiten_adv=bool(kw["advantage_normalization"]),
                    refresh_adv=bool(kw["recompute_advantage"]), c_value=kw["vf_coef"], c_entropy=kw["ent_coef"], max_norm=None,
                    lam=kw["gae_lambda"], discount=kw["discount_factor"], scale_returns=bool(kw["reward_normalization"]))


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def make_modules(c):
    """(tracker, actor, critic) on the CPU in fp32: torch's initialisation from the case's seed, then every bias and LayerNorm weight
    moved off its constant (a gradient through a bias of 0 or a weight of 1 hides a wrong factor there)."""
    from core.inputs import get_dataset_columns
    from core.state_tracker import StateTrackerTransformer
    from tianshou.utils.net.common import Net
    from tianshou.utils.net.continuous import ActorProb, Critic
    torch.manual_seed(c["seed"])
    uc, ac, fc, hu, ha, hf = get_dataset_columns(ACTION_DIM, envname="VirtualTB-v0")
    tracker = StateTrackerTransformer(uc, ac, fc, dim_model=ACTION_DIM, dim_state=c["dim_state"], dim_max_batch=len(c["lens"]),
                                      dataset="VirtualTB-v0", has_user_embedding=hu, has_action_embedding=ha, has_feedback_embedding=hf,
                                      nhead=c["nhead"], d_hid=c["d_hid"], nlayers=c["nlayers"], dropout=c["dropout"], device="cpu",
                                      seed=c["seed"], MAX_TURN=c["T"])
    net = Net(c["dim_state"], hidden_sizes=list(c["hidden"]), device="cpu")
    actor = ActorProb(net, (ACTION_DIM,), max_action=1.0, device="cpu", unbounded=c["unbounded"], conditioned_sigma=c["conditioned_sigma"])
    critic = Critic(net, device="cpu")
    g = torch.Generator().manual_seed(c["seed"] + 1)
    with torch.no_grad():
        for mod in (tracker, actor, critic):
            for name, p in mod.named_parameters():
                if "norm" in name and name.endswith("weight"):
                    p.add_(0.2 * torch.randn(p.shape, generator=g))
                elif name.endswith("bias"):
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        tracker.decoder.weight.mul_(4.0)      # states of O(1): the trunk sees what a trained tracker gives it
        if c["conditioned_sigma"]:
            _wide_sigma_head(actor, g)
        else:
            actor.sigma_param.copy_(-0.5 + 0.3 * torch.randn(actor.sigma_param.shape, generator=g))
    return tracker, actor, critic


WIDE_DIMS = (5, 20)      # conditioned sigma: the action dims whose sigma pre-activation spreads past both ends of ActorProb's clamp [-20, 2]


def _wide_sigma_head(actor, g):
    """Sigma pre-activations around -1 +- 0.3, except WIDE_DIMS: there they spread over [-40, 20], and mu is exactly 0 (a zero row of
    the mu head), so that a stored action sigma^2 u next to it keeps (act - mu) / sigma^2 of O(1) and fp32-exact at sigma = e^-20."""
    lin_s, lin_m = actor.sigma.model[0], actor.mu.model[0]
    lin_s.weight.mul_(0.3)
    lin_s.bias.copy_(-1.0 + 0.1 * torch.randn(lin_s.bias.shape, generator=g))
    for d in WIDE_DIMS:
        lin_s.weight[d].copy_(6.0 * torch.randn(lin_s.weight[d].shape, generator=g))
        lin_s.bias[d] = -9.0
        lin_m.weight[d].zero_()
        lin_m.bias[d] = 0.0


def images(tracker, actor, critic):
    """({name: parameter} of the tracker image, of the policy image) in image order (vtb_model)."""
    from cirs_hip.vtb_model import policy_tensors, tracker_tensors
    return dict(tracker_tensors(tracker)), dict(policy_tensors(actor, critic))


def n_trunk_floats(pimg):
    return sum(v.numel() for k, v in pimg.items() if k.startswith("trunk"))


# ---- the trajectory -----------------------------------------------------------------------------------------------------------------
def _trajectory(c, rng):
    """Host arrays of a collect: every float an fp32 value (the kernels read obs0 / obs / rew as (float)), finite everywhere here; to_device
    puts NaN behind the episode ends."""
    B, T = len(c["lens"]), c["T"]
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)      # noqa: E731
    obs0 = f((rng.uniform(0, 1, (B, USER_DIM + 3)) < 0.25) + 0.05 * rng.standard_normal((B, USER_DIM + 3)))
    obs = f(rng.uniform(-1, 1, (T, B, ACTION_DIM + 3)))
    rew = f(rng.randint(0, 4, (T, B)) + 0.25 * rng.randint(0, 4, (T, B)))
    lens = np.asarray(c["lens"], np.int64)
    done = np.zeros((T, B), np.uint8)
    for e, n in enumerate(lens):
        done[n - 1, e] = 0 if e in c["unfinished"] else 1
    return dict(obs0=obs0, obs=obs, rew=rew, done=done, lens=lens)


def valid_mask(lens, T):
    return np.arange(T).reshape(-1, 1) < np.asarray(lens).reshape(1, -1)      # [T, B]: step t of env e was taken


def masks_for(c, n_pos, env0=0):
    """The masks of positions 0 .. n_pos - 1 of the dropout envs DROP_BASE + env0 + e in the layout vtb_host.states_from_slots takes, from the
    numpy Philox of oracle/nn_oracle.py (the GPU test holds them to cirs_vtb_rollout_masks, bit for bit)."""
    import nn_oracle
    envs, pos = DROP_BASE + env0 + np.arange(len(c["lens"])), np.arange(n_pos)
    one = lambda layer, site, n_elem: nn_oracle.dropout_scale(DROP_SEED, c["dropout"], envs, pos, layer, site, n_elem)      # noqa: E731
    m = {"pos": one(0, vtb_host.DROP_POS, ACTION_DIM)}
    for l in range(c["nlayers"]):
        for site, n_elem in ((vtb_host.DROP_ATTN, n_pos * c["nhead"]), (vtb_host.DROP_RES1, ACTION_DIM), (vtb_host.DROP_FF, c["d_hid"]),
                             (vtb_host.DROP_RES2, ACTION_DIM)):
            m[(l, site)] = one(l, site, n_elem)
    return m


def states_of(c, tracker, traj, dtype, masks_fn=None, record=None):
    """States [T + 1, B, S] in `dtype` with autograd through `tracker` (a copy in that dtype).  record: a list that receives
    (linear1 pre-activations [T + 1, B, d_hid], [T + 1, B] bool: in a graph the loss reaches) per layer and pass."""
    masks_fn = masks_fn or functools.partial(masks_for, c)
    T, lens = c["T"], traj["lens"]
    user = torch.as_tensor(traj["obs0"][:, :USER_DIM]).to(dtype)
    rew = torch.as_tensor(traj["rew"]).to(dtype)
    act = torch.as_tensor(traj["obs"][:, :, :ACTION_DIM]).to(dtype)
    cast = lambda m: {k: v.to(dtype) for k, v in m.items()}      # noqa: E731
    hooks, seen = [], []
    if record is not None:
        for lyr in tracker.transformer_encoder.layers:
            hooks.append(lyr.linear1.register_forward_hook(lambda mod, inp, out: seen.append(out.detach())))
    try:
        pos = torch.arange(T + 1).reshape(-1, 1)
        ln = torch.as_tensor(lens).reshape(1, -1)
        if c["dropout"] > 0 and c["redraw"]:
            out = vtb_host.redraw_states(tracker, user, rew, act, lambda call: cast(masks_fn(call + 1, call * len(lens))))
            used = [(pos <= call) & (call < ln) for call in range(T + 1) for _ in range(c["nlayers"])]
        else:
            out = vtb_host.tracker_states(tracker, user, rew, act, cast(masks_fn(T + 1)) if c["dropout"] > 0 else None)
            used = [pos < ln for _ in range(c["nlayers"])]
    finally:
        for h in hooks:
            h.remove()
    if record is not None:
        assert len(seen) == len(used)
        record.extend(zip(seen, used))
    return out


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def ppo_terms(logp, ent, value, adv, ret, v_s, logp_old, h):
    """Per-row quantities of core.host_rl.ppo_objective for the rows of one minibatch (the advantage statistics are theirs), in the dtype of the
    tensors -- without ppo_objective's rounding of the ratio to float32."""
    a = (adv - adv.mean()) / adv.std() if h.whiten_adv else adv
    ratio = torch.exp(logp - logp_old)
    s1, s2 = ratio * a, torch.clamp(ratio, 1.0 - h.clip, 1.0 + h.clip) * a
    surr = torch.minimum(s1, s2)
    gain = torch.maximum(surr, h.dual * a) if h.dual else surr
    vf1 = (ret - value) ** 2
    if h.clip_value:
        vf2 = (ret - (v_s + torch.clamp(value - v_s, -h.clip, h.clip))) ** 2
        vf = torch.maximum(vf1, vf2)
    else:
        vf2, vf = vf1, vf1
    return dict(a=a, ratio=ratio, s1=s1, s2=s2, surr=surr, gain=gain, vf1=vf1, vf2=vf2, vf=vf, ent=ent, value=value, v_s=v_s)


def ppo_loss(t, h):
    """-> (loss, policy term, value term, entropy term): the device's loss record of one minibatch."""
    pt, vt, et = -t["gain"].mean(), t["vf"].mean(), t["ent"].mean()
    return pt + h.c_value * vt - h.c_entropy * et, pt, vt, et


def margins(t, h):
    """Per row the distance of every comparison the objective branches on from its branch point."""
    big = torch.full_like(t["ratio"], np.inf)
    inside = (t["ratio"] > 1.0 - h.clip) & (t["ratio"] < 1.0 + h.clip)
    out = dict(ratio=torch.minimum((t["ratio"] - (1.0 - h.clip)).abs(), (t["ratio"] - (1.0 + h.clip)).abs()))
    if h.clip_value:
        d = (t["value"] - t["v_s"]).abs()
        out["vclip"] = (d - h.clip).abs()
        out["vf"] = torch.where(d > h.clip, (t["vf1"] - t["vf2"]).abs(), big)      # inside the clip range both squares are one number
    if h.dual:
        out["dual"] = (h.dual * t["a"] - t["surr"]).abs()
    out["inside"] = inside      # (not a distance: the exact ties s1 == s2, which the kernel splits as torch does)
    return out


def classes(t, h):
    """Row counts of the branches the minibatch kernel's backward distinguishes."""
    r, a = t["ratio"], t["a"]
    lo, hi = r < 1.0 - h.clip, r > 1.0 + h.clip
    out = {"below+": lo & (a > 0), "below-": lo & (a < 0), "above+": hi & (a > 0), "above-": hi & (a < 0), "tie": ~lo & ~hi,
           "blocked": t["s2"] < t["s1"], "passing": t["s1"] < t["s2"]}      # the clipped side is taken (no gradient) | the free side is
    if h.clip_value:
        d = t["value"] - t["v_s"]
        out.update({"vbind_lo": (d < -h.clip) & (t["vf2"] > t["vf1"]), "vbind_hi": (d > h.clip) & (t["vf2"] > t["vf1"]),
                    "vfree": (d.abs() > h.clip) & (t["vf1"] > t["vf2"]), "vinside": d.abs() < h.clip})
    if h.dual:
        out["dual-"] = (a < 0) & (h.dual * a > t["surr"])
    return {k: int(v.sum()) for k, v in out.items()}


def planned(c):
    """The classes a case must populate with MIN_CLASS_ROWS rows in its first minibatch of the last pass."""
    h = hyper_of(c["hyper"])
    if c["classes"] is None:
        return []
    if c["classes"] == "few":
        return ["tie", "blocked", "passing"]
    return ["below+", "below-", "above+", "above-", "tie"] + (["vbind_lo", "vbind_hi", "vfree", "vinside"] if h.clip_value else []) + \
        (["dual-"] if h.dual else [])


# ---- the builder ---------------------------------------------------------------------------------------------------------------------
def _nudge(bias, bad, rng):
    """Moves the biases of the hidden units `bad` by 0.003 .. 0.03 (fp32)."""
    with torch.no_grad():
        step = torch.as_tensor(rng.uniform(0.003, 0.03, int(bad.sum())) * rng.choice([-1.0, 1.0], int(bad.sum())), dtype=torch.float32)
        bias[bad] += step


def _settle_tracker(c, tracker, traj, rng, rounds=200):
    """Every linear1 pre-activation of every position in a graph the loss reaches at least KINK from 0: the first layer (in forward order) with
    offending units gets those units' biases moved, until none offends.  -> units moved."""
    moved = 0
    for _ in range(rounds):
        rec = []
        with torch.no_grad():
            states_of(c, copy.deepcopy(tracker).double(), traj, torch.float64, record=rec)
        NL = c["nlayers"]
        worst = [None] * NL
        for i, (z, used) in enumerate(rec):
            m = torch.where(used.unsqueeze(-1), z.abs(), torch.full_like(z, np.inf)).amin((0, 1))
            worst[i % NL] = m if worst[i % NL] is None else torch.minimum(worst[i % NL], m)
        for l in range(NL):
            bad = worst[l] < KINK
            if bad.any():
                _nudge(tracker.transformer_encoder.layers[l].linear1.bias, bad, rng)
                moved += int(bad.sum())
                break
        else:
            return moved, float(min(w.min() for w in worst))
    raise AssertionError("the tracker's ReLU margins did not settle")


def _settle_trunk(actor, p64_of, states, rng, rounds=200):
    lin = [m for m in actor.preprocess.model.model if isinstance(m, torch.nn.Linear)]
    moved = 0
    for _ in range(rounds):
        pre = vtb_host.hidden_preactivations(p64_of(), states)
        for i, z in enumerate(pre):
            bad = z.abs().amin(0) < KINK
            if bad.any():
                _nudge(lin[i].bias, bad, rng)
                moved += int(bad.sum())
                break
        else:
            return moved, float(min(z.abs().min() for z in pre))
    raise AssertionError("the trunk's ReLU margins did not settle")


def minibatches(c, n):
    """[(pass, index array into the rows)] in the order the update runs them (row_ranges: a short tail joins the range before it)."""
    from core.host_rl import row_ranges
    bs = n if c["batch_size"] is None else c["batch_size"]
    return bs, [(s, (a, b)) for s in range(c["repeat"]) for a, b in row_ranges(n, bs)]


def _terms_of(case, cols, mb, dtype=torch.float64):
    rq = case["row64"]
    idx = torch.as_tensor(case["perms"][mb[0]][mb[1][0]:mb[1][1]]).long()
    u = case["uniq"][idx]
    col = lambda k: cols[k].to(dtype)[idx]      # noqa: E731
    return ppo_terms(rq["logp"][u], rq["ent"][u], rq["value"][u], col("adv"), col("ret"), col("v_s"), col("logp_old"), case["h"]), idx


def _adjust(case, cols, rounds=12):
    """Moves every row closer than KINK to a branch point of the objective off it: + 0.01 on its logp_old (ratio, dual clip) or its v_s (value
    clip), in fp32, again until no row of any minibatch of any pass offends.  -> rows moved."""
    moved = 0
    for _ in range(rounds):
        bad_l = torch.zeros(case["n"], dtype=torch.bool)
        bad_v = torch.zeros(case["n"], dtype=torch.bool)
        for mb in case["mbs"]:
            t, idx = _terms_of(case, cols, mb)
            m = margins(t, case["h"])
            bl = m["ratio"] < KINK
            if "dual" in m:
                bl |= m["dual"] < KINK
            bad_l[idx[bl]] = True
            if "vclip" in m:
                bad_v[idx[(m["vclip"] < KINK) | (m["vf"] < KINK)]] = True
        if not (bad_l.any() or bad_v.any()):
            return moved
        moved += int(bad_l.sum() + bad_v.sum())
        cols["logp_old"][bad_l] += np.float32(0.01)
        cols["v_s"][bad_v] += np.float32(0.01)
    raise AssertionError("the objective's margins did not settle")


@functools.lru_cache(maxsize=None)
def build(name):
    """-> the case: modules (fp32, CPU), trajectory, rows, columns, permutations, and the float64 forward the columns were placed around.
    Built once, shared, never modified by a test (a test works on copies of the modules)."""
    c = CASES[name]
    rng = np.random.RandomState(c["seed"])
    tracker, actor, critic = make_modules(c)
    traj = _trajectory(c, rng)
    lens, T, B = traj["lens"], c["T"], len(c["lens"])
    h = hyper_of(c["hyper"])
    moved_t, relu_t = _settle_tracker(c, tracker, traj, rng)
    with torch.no_grad():
        states = states_of(c, copy.deepcopy(tracker).double(), traj, torch.float64)
    # the buffer rows (env * T + t): every step in buffer order, or n_draw of them with repetition
    env_all = np.concatenate([np.full(n, e) for e, n in enumerate(lens)])
    t_all = np.concatenate([np.arange(n) for n in lens])
    if c["n_draw"]:
        pick = rng.randint(0, len(env_all), c["n_draw"])
        pick[:4] = (0, 0, 0, len(env_all) - 1)      # one step three times
    else:
        pick = np.arange(len(env_all))
    uniq = torch.as_tensor(pick)
    rows = env_all[pick] * T + t_all[pick]
    n = len(rows)
    st_rows = states[torch.as_tensor(t_all), torch.as_tensor(env_all)]      # [steps, S] float64
    pimg = lambda: {k: v.detach().double() for k, v in images(tracker, actor, critic)[1].items()}      # noqa: E731
    moved_p, relu_p = _settle_trunk(actor, pimg, st_rows, rng)
    # stored raw actions: drawn from the current policy, mu + sigma z (WIDE_DIMS of a conditioned sigma: sigma min(sigma, 1) z around mu = 0)
    with torch.no_grad():
        r0 = vtb_host.policy_rows(pimg(), st_rows, torch.zeros(len(env_all), ACTION_DIM, dtype=torch.float64), 1.0, c["unbounded"])
        z = torch.as_tensor(rng.standard_normal((len(env_all), ACTION_DIM)))
        raw = r0["mu"] + r0["sigma"] * z
        if c["conditioned_sigma"]:
            for d in WIDE_DIMS:
                raw[:, d] = r0["sigma"][:, d] * torch.clamp(r0["sigma"][:, d], max=1.0) * z[:, d]
        raw = raw.float()
        row64 = vtb_host.policy_rows(pimg(), st_rows, raw.double(), 1.0, c["unbounded"])
    act = np.zeros((T, B, ACTION_DIM), np.float32)
    act[t_all, env_all] = raw.numpy()
    traj["act"] = act
    # the columns: ratios 0.55 .. 0.7 | 0.9 .. 1.1 | 1.35 .. 1.7 (and 2.3 .. 3 past a dual clip of 2) in turn, value shifts inside and on
    # both sides of the clip, returns around the value
    k = np.arange(n)
    kind = k % (4 if h.dual else 3)
    target = np.select([kind == 0, kind == 1, kind == 2], [rng.uniform(0.55, 0.7, n), rng.uniform(0.9, 1.1, n), rng.uniform(1.35, 1.7, n)],
                       rng.uniform(2.3, 3.0, n))
    shift = np.select([(k // 4) % 3 == 0, (k // 4) % 3 == 1], [rng.uniform(-0.1, 0.1, n), rng.uniform(0.3, 0.6, n)], -rng.uniform(0.3, 0.6, n))
    order = rng.permutation(n)      # (the classes must not line up with the buffer order)
    target, shift = target[order], shift[order]
    lp, val = row64["logp"][uniq].numpy(), row64["value"][uniq].numpy()
    cols = dict(logp_old=torch.as_tensor((lp - np.log(target)).astype(np.float32)), v_s=torch.as_tensor((val + shift).astype(np.float32)),
                ret=torch.as_tensor((val + 0.7 * rng.standard_normal(n)).astype(np.float32)),
                adv=torch.as_tensor(rng.standard_normal(n).astype(np.float32)))
    perms = [rng.permutation(n) for _ in range(c["repeat"])]
    bs, mbs = minibatches(c, n)
    done_rows = np.zeros(B * T, bool)
    done_rows[env_all * T + t_all] = traj["done"][t_all, env_all].astype(bool)
    unfinished = np.array([e * T + lens[e] - 1 for e in c["unfinished"]], dtype=np.int64)
    case = dict(name=name, c=c, h=h, tracker=tracker, actor=actor, critic=critic, traj=traj, rows=rows, n=n, uniq=uniq, env_all=env_all, t_all=t_all,
                row64=row64, perms=perms, mbs=mbs, batch_size=bs, done_rows=done_rows, unfinished=unfinished, B=B, T=T,
                moved=dict(tracker_units=moved_t, trunk_units=moved_p), relu=dict(tracker=relu_t, trunk=relu_p))
    case["moved"]["rows"] = _adjust(case, cols)
    case["cols"] = cols
    return case


def check_case(case):
    """The builder's conditions, asserted (both test modules call it): margins of every row of every minibatch, class counts, the sigma clamp.
    -> dict(margins, classes of the last pass's first minibatch, relu, sigma) for the log."""
    c, h = case["c"], case["h"]
    low = {}
    for mb in case["mbs"]:
        t, _ = _terms_of(case, case["cols"], mb)
        m = margins(t, h)
        assert int(m.pop("inside").sum()) >= (MIN_CLASS_ROWS if case["n"] >= 4 else 0), "ties"
        for k, v in m.items():
            low[k] = min(low.get(k, np.inf), float(v.min()))
    for k, v in low.items():
        assert v >= KINK, (case["name"], k, v)
    assert case["relu"]["tracker"] >= KINK and case["relu"]["trunk"] >= KINK, case["relu"]
    first_of_last = [mb for mb in case["mbs"] if mb[0] == c["repeat"] - 1][0]
    cl = classes(_terms_of(case, case["cols"], first_of_last)[0], h)
    for k in planned(c):
        assert cl[k] >= MIN_CLASS_ROWS, (case["name"], k, cl)
    sig = {}
    if c["conditioned_sigma"]:
        sp = case["row64"]["sigma_pre"][case["uniq"].unique()]
        sig = dict(low=int((sp < vtb_host.SIGMA_MIN).any(1).sum()), high=int((sp > vtb_host.SIGMA_MAX).any(1).sum()),
                   free=int(((sp > vtb_host.SIGMA_MIN) & (sp < vtb_host.SIGMA_MAX)).all(1).sum()),
                   margin=float(torch.minimum((sp - vtb_host.SIGMA_MIN).abs(), (sp - vtb_host.SIGMA_MAX).abs()).min()))
        assert sig["low"] >= MIN_CLASS_ROWS and sig["high"] >= MIN_CLASS_ROWS and sig["margin"] >= KINK, sig
    return dict(margins=low, classes=cl, relu=case["relu"], sigma=sig, moved=case["moved"])


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def evaluate(case, dtype, masks_fn=None, passes=None):
    """-> (losses [n_mb, 4] float64 array, {name: gradient} of the tracker image, of the policy image, float64 tensors) by autograd in `dtype`:
    the policy's gradient of the LAST minibatch, the tracker's summed over the minibatches of the LAST pass (the tracker optimiser is cleared
    at the start of every pass and steps once, on what the last pass left).  passes: the passes counted instead (a test of the tests)."""
    c, h = case["c"], case["h"]
    passes = (c["repeat"] - 1,) if passes is None else passes
    tracker = copy.deepcopy(case["tracker"]).to(dtype)
    actor, critic = copy.deepcopy((case["actor"], case["critic"]))
    timg, pimg = images(tracker, actor, critic)
    pimg = {k: v.detach().to(dtype).requires_grad_(True) for k, v in pimg.items()}
    states = states_of(c, tracker, case["traj"], dtype, masks_fn)
    st = states[torch.as_tensor(case["t_all"]), torch.as_tensor(case["env_all"])]
    rq = vtb_host.policy_rows(pimg, st, torch.as_tensor(case["traj"]["act"][case["t_all"], case["env_all"]]).to(dtype), 1.0, c["unbounded"])
    cols = {k: v.to(dtype) for k, v in case["cols"].items()}
    losses, g_t, g_p = [], None, None
    for s, (a, b) in case["mbs"]:
        idx = torch.as_tensor(case["perms"][s][a:b]).long()
        u = case["uniq"][idx]
        t = ppo_terms(rq["logp"][u], rq["ent"][u], rq["value"][u], cols["adv"][idx], cols["ret"][idx], cols["v_s"][idx], cols["logp_old"][idx], h)
        out = ppo_loss(t, h)
        losses.append([float(x.detach()) for x in out])
        if s in passes:
            g = torch.autograd.grad(out[0], list(timg.values()) + list(pimg.values()), retain_graph=True, allow_unused=True)
            g = [torch.zeros_like(p) if x is None else x for x, p in zip(g, list(timg.values()) + list(pimg.values()))]
            gt = [x.double() for x in g[:len(timg)]]
            g_t = gt if g_t is None else [x + y for x, y in zip(g_t, gt)]
            g_p = [x.double() for x in g[len(timg):]]
    return np.array(losses), dict(zip(timg, g_t)), dict(zip(pimg, g_p))


def err_of(got, want):
    """max |got - want| / max |want| over a tensor; a reference that is identically zero admits zero only."""
    top = float(want.abs().max())
    if top == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float((got - want).abs().max()) / top


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(losses [n_mb, 4], g64 {name: gradient} over both images, e32 {name: err_of the fp32 evaluation}), computed once."""
    case = build(name)
    losses, gt, gp = evaluate(case, torch.float64)
    _, gt32, gp32 = evaluate(case, torch.float32)
    g64, g32 = dict(gt, **gp), dict(gt32, **gp32)
    assert len(g64) == len(gt) + len(gp)
    return dict(losses=losses, g64=g64, e32={k: err_of(g32[k], g64[k]) for k in g64}, tracker_names=list(gt), policy_names=list(gp))


# ---- the device side -----------------------------------------------------------------------------------------------------------------
class _Buffer:
    """What DeviceVtbLearner.prepare reads of a replay buffer."""

    def __init__(self, case):
        self.size, self.done, self._unfinished = case["T"], case["done_rows"], case["unfinished"]

    def unfinished_index(self):
        return self._unfinished


def to_device(case, device="cuda"):
    """(rows_src, buffer): the trajectory on the device, NaN in every float column behind the episode ends."""
    tr, T, B = case["traj"], case["T"], case["B"]
    gone = ~valid_mask(tr["lens"], T)
    obs, rew, act = tr["obs"].copy(), tr["rew"].copy(), tr["act"].copy()
    obs[gone], rew[gone], act[gone] = np.nan, np.nan, np.nan
    d = lambda x: torch.as_tensor(x).to(device)      # noqa: E731
    traj = dict(obs0=d(tr["obs0"]), obs=d(obs), rew=d(rew), done=d(tr["done"]), act=d(act), len=d(tr["lens"].astype(np.int32)))
    c = case["c"]
    src = types.SimpleNamespace(dropout_p=float(c["dropout"]), drop_env_base=DROP_BASE if c["dropout"] > 0 else 0,
                                dropout_seed=DROP_SEED, dropout_redraw=bool(c["redraw"]), lens=tr["lens"],
                                rollout=types.SimpleNamespace(traj=traj))
    return src, _Buffer(case)


def make_policy(case, lr, betas, max_grad_norm):
    """(HostPPOPolicy, tracker, actor, critic): copies of the case's modules under fresh optimisers (the policy's lists the trunk twice)."""
    from core.host_rl import HostPPOPolicy
    from torch.distributions import Independent, Normal
    tracker, (actor, critic) = copy.deepcopy(case["tracker"]), copy.deepcopy((case["actor"], case["critic"]))
    optim = [torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=lr, betas=betas),
             torch.optim.Adam(tracker.parameters(), lr=lr, betas=betas)]
    policy = HostPPOPolicy(actor, critic, optim, lambda *logits: Independent(Normal(*logits), 1), max_grad_norm=max_grad_norm, **case["c"]["hyper"])
    return policy, tracker, actor, critic


def run_update(case, policy, tracker, actor, critic, device="cuda"):
    """One device update of the case with the returns stage's columns replaced by the case's.  -> losses [n_mb, 4]."""
    from cirs_hip.vtb_learn import DeviceVtbLearner
    src, buf = to_device(case, device)
    ln = DeviceVtbLearner(tracker, actor, critic, case["B"], case["T"], device)
    ln.prepare(policy, src, case["rows"], buf)
    for view, k in zip(ln.row_block(), ("v_s", "adv", "ret", "logp_old")):
        view.copy_(case["cols"][k].to(device))
    rep = ln.learn(policy, case["perms"], case["batch_size"], case["c"]["repeat"])
    return np.stack([rep[k] for k in ("loss", "loss/clip", "loss/vf", "loss/ent")], 1)


def flat_state(params, optim, key=None):
    """The flat float64 image of the parameters (key None) or of one optimiser state entry."""
    return np.concatenate([(p if key is None else optim.state[p][key]).detach().double().reshape(-1).numpy() for p in params])


# ---- clip_grad_norm_ + Adam, fed the device's own gradient ----------------------------------------------------------------------------
# The float64 recurrence of HostPPOPolicy.learn's optimiser schedule: total norm with the trunk's squared norm counted twice (the parameter list
# holds it twice), coef = min(1, max_norm / (norm + 1e-6)), the trunk's gradient scaled by coef twice (clip_grad_norm_ multiplies every
# list entry) and stepped twice (steps 2k + 1, 2k + 2), the heads once (step k + 1); the tracker one plain step.  The bars are gradcase's
# (M_BAR, V_BAR, V_TINY, P_BAR, UPD_BAR), widened as tests/ppogradcase.py widens them, with this kernel's own counts:
# (1) the coefficient.  vtb_learn_adam_kernel sums the squares in float64 (at most 2^18 terms: 2^-35 relative, nothing next to fp32), then
#     (float)sqrt 1 rounding, + 1e-6f 1, the division 1:  e_c = 3 x 2^-24 (half-ulps, relative).  Without clipping coef is the constant 1.
# (2) g * coef (heads) is one more rounding, (g * coef) * coef (trunk) two:  e_g = pow (e_c + 2^-24), carried into m and v as ppogradcase does.
# (3) adam_one forms v' = fma(v, b2, ((1 - b2) g) g): the roundings of 1 - b2, of the two products and of the fma, four of positive terms
#     <= v' -- one fewer than the unfused form V_BAR = 2^-20 (16 half-ulps) was derived for: unchanged.  m' and the update are gradcase's
#     statements (sqrtf and the divisions correctly rounded in this build): M_BAR, UPD_BAR, P_BAR unchanged.
# (4) the trunk's first sub-step leaves no trace; its update enters as an interval, as in ppogradcase.check_clip_adam.
E_COEF = 3.0 * HALF_ULP


def clip_coef(g, n_trunk, max_grad_norm):
    sq = 2.0 * np.sum(g[:n_trunk] ** 2) + np.sum(g[n_trunk:] ** 2)
    norm = float(np.sqrt(sq))
    return norm, min(1.0, float(np.float32(max_grad_norm)) / (norm + float(np.float32(1e-6))))


def check_clip_adam(p0, m0, v0, g, m1, v1, p1, n_trunk, k, max_grad_norm, lr, betas, eps, what=""):
    """Device moments / parameters of the policy image after one minibatch with the heads' step count k before it (flat float64 arrays) against
    the recurrence fed the device's own gradient.  -> (norm, coef, the largest share of each bar used)."""
    from gradcase import M_BAR, P_BAR, UPD_BAR, V_BAR, V_TINY, adam_constants, adam_moments, adam_update
    P = len(g)
    norm, coef = clip_coef(g, n_trunk, max_grad_norm)
    e_c = E_COEF if coef < 1.0 else 0.0
    used = {}
    for tag, sl, pw, steps in (("trunk", slice(0, n_trunk), 2, (2 * k + 1, 2 * k + 2)), ("heads", slice(n_trunk, P), 1, (k + 1,))):
        gs = g[sl] * coef ** pw
        e_g = pw * (e_c + HALF_ULP) if coef < 1.0 else 0.0
        rm, rv, rp = m0[sl], v0[sl], p0[sl]
        bm, bv, bp = np.zeros_like(rm), np.zeros_like(rv), np.zeros_like(rp)
        for q, t in enumerate(steps):
            b1, b2, e, ss, bc2s = adam_constants(t, lr, betas, eps)
            m_in = rm
            rm, rv = adam_moments(rm, rv, gs, b1, b2)
            bm = b1 * bm + M_BAR * (np.abs(m_in) + np.abs(gs)) + (1.0 - b1) * np.abs(gs) * e_g
            bv = b2 * bv + V_BAR * rv + V_TINY + 2.0 * (1.0 - b2) * gs * gs * e_g
            if q + 1 < len(steps):      # a sub-step whose moments the next one overwrites: the update from the recurrence's, as an interval
                _, upd = adam_update(rp, rm, rv, ss, bc2s, e)
                den_lo, den_hi = np.sqrt(np.maximum(rv - bv, 0.0)) / bc2s + e, np.sqrt(rv + bv) / bc2s + e
                corners = np.stack([ss * mm / dd for mm in (rm - bm, rm + bm) for dd in (den_lo, den_hi)])
                bp = bp + np.maximum(corners.max(0) - upd, upd - corners.min(0)) + UPD_BAR * np.abs(corners).max(0)
            else:                       # the last one: from the device's own new moments (gradcase.check_adam)
                _, upd = adam_update(rp, m1[sl], v1[sl], ss, bc2s, e)
                bp = bp + UPD_BAR * np.abs(upd)
            rp = rp - upd
            bp = bp + P_BAR * (np.abs(rp) + np.abs(upd))
        for nm, d, bar in (("m", np.abs(m1[sl] - rm), bm), ("v", np.abs(v1[sl] - rv), bv), ("p", np.abs(p1[sl] - rp), bp)):
            ok = d <= bar
            i = int(np.argmax(d - bar))
            assert ok.all(), f"{what}: Adam {nm} ({tag}): {int((~ok).sum())} entries outside the bar, worst at {i}: |diff| {d[i]:.3e} > {bar[i]:.3e}"
            with np.errstate(divide="ignore", invalid="ignore"):
                used[f"{tag}_{nm}"] = float(np.where(bar > 0, d / bar, 0.0).max())
    return norm, coef, used
