"""Shared cases and the float64 reference of the PPO minibatch step's gradient tests (tests/test_gpu_ppo_step_grads.py,
tests/test_ppo_gradcase_cpu.py): csrc/ppo.hip from trunk_adv_kernel to adam_next_kernel.

ppo_loss restates core/policy/ppo.py:183-212 with its three options (norm_adv, value_clip, dual_clip); test_ppo_gradcase_cpu.py holds it to the
losses the reference recorded (tests/golden/learn.npz, learn_opts.npz).  A case is a set of parameters, a buffer-order batch of mb + 37 rows and
an index list of mb distinct rows in random order: the 37 rows outside the list hold NaN in every float column, so a gather that reads a
neighbouring row, or a padded row that is counted, shows.  Rows a branch of the loss could take differently in fp32 and in float64 are moved
off the branch point by the builder (adjust), never dropped.  Cases come from fixed seeds (no golden file)."""
import functools

import numpy as np
import torch

from cirs_hip.learner import FLAT_ORDER, DeviceLearner, flat_policy_params

EPS32 = float(np.finfo(np.float32).eps)
S, H = 20, 64
EXTRA_ROWS = 37
MARGIN = 1e-4          # 100 x what fp32 loses on the O(1) quantities the branches compare
RELU_MARGIN = 1e-6     # 10 x what fp32 loses on a hidden pre-activation (a sum of 20 / 64 products of O(0.3) terms)
UPPER_CLAMP_ROOM = 1e-6      # 8 eps32: no row's p_a comes this close to 1, so Categorical's upper clamp at 1 - eps32 (fp32 resolves p_a to a few ulp) is never in play
LOGP_NOISE = 0.3       # sd of logp_old around the current policy's log-probability: a quarter of the rows has its ratio clipped against the gradient
HYPER = dict(eps_clip=0.2, vf_coef=0.25, ent_coef=0.0, norm_adv=True, value_clip=True, dual_clip=None)      # the defaults of test_gpu_head_precision
MIN_CLASS_ROWS, CLASS_FROM_MB = 3, 33


def shapes_of(I):
    return dict(w1=(H, S), b1=(H,), w2=(H, H), b2=(H,), wa=(I, H), ba=(I,), wc=(1, H), bc=(1,))


# ---- the loss ----------------------------------------------------------------------------------------------------------------------
def ppo_terms(p, obs, act, adv, ret, v_s, logp_old, *, eps_clip, vf_coef, ent_coef, norm_adv=True, value_clip=True, dual_clip=None, **_):
    """Per-row quantities of ppo.py:183-212 for the rows given (a whole global minibatch: the advantage statistics are theirs), in the dtype of
    the tensors, Categorical's fp32 clamp constant in every dtype (the clamp blocks the gradient of a clamped probability)."""
    h1p = obs @ p["w1"].T + p["b1"]
    h1 = torch.relu(h1p)
    h2p = h1 @ p["w2"].T + p["b2"]
    h2 = torch.relu(h2p)
    z = h2 @ p["wa"].T + p["ba"]
    value = (h2 @ p["wc"].T + p["bc"]).flatten()
    probs = torch.softmax(z, dim=-1)
    logp_all = torch.log(probs.clamp(min=EPS32, max=1 - EPS32))
    logp = logp_all.gather(1, act.view(-1, 1)).squeeze(1)
    ent = -(logp_all * probs).sum(-1)
    a = (adv - adv.mean()) / adv.std() if norm_adv else adv
    ratio = (logp - logp_old).exp()
    s1, s2 = ratio * a, ratio.clamp(1 - eps_clip, 1 + eps_clip) * a
    surr = torch.min(s1, s2)
    clip = -torch.max(surr, dual_clip * a) if dual_clip else -surr      # ppo.py:190-193: for every sign of a
    vf1 = (ret - value).pow(2)
    if value_clip:
        v_clip = v_s + (value - v_s).clamp(-eps_clip, eps_clip)
        vf2 = (ret - v_clip).pow(2)
        vf = torch.max(vf1, vf2)
    else:
        vf2, vf = vf1, vf1
    return dict(clip=clip, vf=vf, ent=ent, p_a=probs.gather(1, act.view(-1, 1)).squeeze(1), ratio=ratio, a=a, s1=s1, s2=s2, surr=surr, value=value,
                vf1=vf1, vf2=vf2, h1p=h1p, h2p=h2p, logp=logp)


def ppo_loss(p, obs, act, adv, ret, v_s, logp_old, *, share=None, **hyper):
    """-> (loss, clip, vf, ent): the step's loss and its three terms as ppo.py forms them (means over the minibatch).  share = (lo, hi): only
    rows lo .. hi - 1 are summed, still divided by the whole minibatch's row count and with its advantage statistics -- the part of the loss a
    data-parallel rank holds."""
    t = ppo_terms(p, obs, act, adv, ret, v_s, logp_old, **hyper)
    n = obs.shape[0]
    sl = slice(0, n) if share is None else slice(*share)
    clip, vf, ent = (t[k][sl].sum() / n for k in ("clip", "vf", "ent"))
    return clip + hyper["vf_coef"] * vf - hyper["ent_coef"] * ent, clip, vf, ent


def loss_and_grads(p, cols, hyper, dtype, share=None):
    """-> (four loss terms as floats, {name: gradient} of the eight tensors and of "obs" (the gathered rows), float64 tensors) by autograd in
    `dtype`.  p: {name: tensor}; cols: (obs, act, adv, ret, v_s, logp_old) of the minibatch's rows in minibatch order."""
    q = {k: p[k].to(dtype).clone().requires_grad_(True) for k in FLAT_ORDER}
    obs, act, adv, ret, v_s, logp_old = cols
    o = obs.to(dtype).clone().requires_grad_(True)
    out = ppo_loss(q, o, act, adv.to(dtype), ret.to(dtype), v_s.to(dtype), logp_old.to(dtype), share=share, **hyper)
    g = torch.autograd.grad(out[0], [q[k] for k in FLAT_ORDER] + [o])
    grads = {k: t.double() for k, t in zip(FLAT_ORDER + ["obs"], g)}
    return [float(x.detach()) for x in out], grads


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _case(I, mb, seed, sharp=2.0, rows_kernel=None, **hyper):
    return dict(I=I, mb=mb, seed=seed, sharp=sharp, rows_kernel=rows_kernel, hyper=dict(HYPER, **hyper))


# The row counts sit on the step's own constants: 4 rows per trunk_adv_kernel workgroup, 8 per R workgroup of trunk_rows_kernel, the 32-row
# MFMA tile, 128 rows per row block of head_bwd_fused_kernel, 32-item tiles in chunks of at least 4, trunk_rows_kernel's ceiling of 2048 padded rows.
SHAPES = {
    "I20-mb2": _case(20, 2, 11),                 # the smallest legal step; one partial item tile
    "I100-mb5": _case(100, 5, 12),               # fewer rows than one R workgroup
    "I160-mb33": _case(160, 33, 13),             # one row into the second row tile; 4 + 1 item tiles
    "I180-mb70": _case(180, 70, 14),             # a partly padded tile; 4 + 2 item tiles, the last partial
    "I224-mb129": _case(224, 129, 1015),          # one live row in the second row block
    "I777-mb200": _case(777, 200, 16),           # an idle wave pair in the second row block
    "I300-mb2047": _case(300, 2047, 17),         # n_pad = 2048: the last size on trunk_rows_kernel, the largest merged minibatch at batch size 1024
    "I300-mb2049": _case(300, 2049, 18),         # the first size that falls to dh2_sum_kernel + trunk_bwd_kernel by itself
    "I10728-mb1051": _case(10728, 1051, 19),     # the benchmark catalogue, 8.2 row blocks
}
# (a seed is a plain number unless the case it gives misses a condition of tests/test_ppo_gradcase_cpu.py -- fewer than three rows with a clamped p_a,
# a hidden pre-activation within RELU_MARGIN of zero; then it is the next of seed + 1000 k that meets them)
OPTIONS = {}
for _name, _seeds in (("I180-mb70", (141, 1142, 143, 144)), ("I224-mb129", (151, 152, 1153, 154))):
    _I, _mb = SHAPES[_name]["I"], SHAPES[_name]["mb"]
    OPTIONS[_name + "-rawadv"] = _case(_I, _mb, _seeds[0], norm_adv=False)
    OPTIONS[_name + "-novclip"] = _case(_I, _mb, _seeds[1], value_clip=False)
    OPTIONS[_name + "-dual3-ent"] = _case(_I, _mb, _seeds[2], dual_clip=3.0, ent_coef=0.01)
    OPTIONS[_name + "-dual1.5-sharp6"] = _case(_I, _mb, _seeds[3], sharp=6.0, dual_clip=1.5)
OPTIONS["I180-mb70-trunkbwd"] = _case(180, 70, 14, rows_kernel="0")      # CIRS_PPO_ROWS_KERNEL=0: the fallback trunk backward at a ragged size
CASES = dict(SHAPES, **OPTIONS)
SHARDS = {"I180-mb70": (23, 1, 46), "I224-mb129": (64, 65)}      # local row counts of the data-parallel split (consecutive runs of the index list)
ADAM_CASES = ("I160-mb33", "I224-mb129", "I300-mb2049")


def forced_actions(I):
    """(the catalogue's last item, the first item of the last chunk of item tiles): test_gpu_head_bwd_roles' choice."""
    n_tiles = -(-I // 32)
    return I - 1, ((n_tiles - 1) // 4) * 4 * 32


def margins(t, hyper):
    """Per row the distance of every comparison the loss branches on from its branch point (float64 terms of ppo_terms)."""
    e = hyper["eps_clip"]
    big = torch.full_like(t["ratio"], np.inf)
    out = dict(ratio=torch.minimum((t["ratio"] - (1 - e)).abs(), (t["ratio"] - (1 + e)).abs()),
               p_a=(t["p_a"] / EPS32 - 1).abs())
    if hyper["value_clip"]:
        d = (t["value"] - t["v_s"]).abs()
        out["vclip"] = (d - e).abs()
        out["vf"] = torch.where(d > e, (t["vf1"] - t["vf2"]).abs(), big)      # inside the clip range both squares are the same number
    if hyper["dual_clip"]:
        out["dual"] = (hyper["dual_clip"] * t["a"] - t["surr"]).abs()
    return out


def classes(t, hyper):
    """Row counts of the branches the step's backward distinguishes."""
    clamped = t["p_a"] < EPS32
    dual = hyper["dual_clip"] * t["a"] > t["surr"] if hyper["dual_clip"] else torch.zeros_like(clamped)
    out = dict(blocked=int(((t["s2"] < t["s1"]) & ~clamped).sum()), passing=int(((t["s1"] <= t["s2"]) & ~clamped & ~dual).sum()),
               clamped=int(clamped.sum()))
    if hyper["value_clip"]:
        out["vclip"] = int((t["vf2"] > t["vf1"]).sum())
    if hyper["dual_clip"]:
        out["dual"] = int(dual.sum())
    return out


def _terms64(p, cols, hyper):
    obs, act, adv, ret, v_s, logp_old = cols
    with torch.no_grad():
        t = ppo_terms({k: v.double() for k, v in p.items()}, obs.double(), act, adv.double(), ret.double(), v_s.double(), logp_old.double(), **hyper)
    t["v_s"] = v_s.double()
    return t


def adjust(p, cols, hyper, rounds=8):
    """Moves every row closer than MARGIN to a branch point off it: + 0.01 on its logp_old (ratio, dual clip) or on its v_s (value clip), in
    fp32, again until no row offends.  -> (cols, rows moved).  A p_a at eps32 is not something a batch column moves: such a case takes another seed."""
    obs, act, adv, ret, v_s, logp_old = cols
    v_s, logp_old = v_s.clone(), logp_old.clone()
    moved = 0
    for _ in range(rounds):
        m = margins(_terms64(p, (obs, act, adv, ret, v_s, logp_old), hyper), hyper)
        bad_l = m["ratio"] < MARGIN
        if "dual" in m:
            bad_l |= m["dual"] < MARGIN
        bad_v = (m["vclip"] < MARGIN) | (m["vf"] < MARGIN) if "vclip" in m else torch.zeros_like(bad_l)
        if not (bad_l.any() or bad_v.any()):
            break
        moved += int(bad_l.sum() + bad_v.sum())
        logp_old[bad_l] += np.float32(0.01)
        v_s[bad_v] += np.float32(0.01)
    return (obs, act, adv, ret, v_s, logp_old), moved


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(name, I, mb, n_rows, hyper, rows_kernel, p {name: fp32 tensor}, cols = the minibatch's rows in minibatch order (fp32 tensors, act int64),
    batch = the buffer-order columns of n_rows rows (NaN outside idx), idx, b_env, b_t, n_env, max_turn, moved).  Built once, shared, never
    modified by a test."""
    c = CASES[name]
    I, mb, sharp, hyper = c["I"], c["mb"], c["sharp"], c["hyper"]
    rng = np.random.RandomState(c["seed"])
    shapes = shapes_of(I)
    scale = dict(w1=0.3, b1=0.1, w2=0.2, b2=0.1, wa=0.25 * sharp, ba=0.1, wc=0.2, bc=0.1)      # test_gpu_head_precision's: logits spread over several units
    p = {k: torch.as_tensor(rng.standard_normal(shapes[k]) * scale[k]).float() for k in FLAT_ORDER}
    obs = torch.as_tensor(rng.standard_normal((mb, S))).float()
    adv = torch.as_tensor(rng.standard_normal(mb)).float()
    ret = torch.as_tensor(rng.standard_normal(mb)).float()
    v_s = torch.as_tensor(rng.standard_normal(mb) * 0.5).float()
    noise = torch.as_tensor(rng.standard_normal(mb) * LOGP_NOISE)
    with torch.no_grad():
        p64 = {k: v.double() for k, v in p.items()}
        z0 = torch.relu(torch.relu(obs.double() @ p64["w1"].T + p64["b1"]) @ p64["w2"].T + p64["b2"]) @ p64["wa"].T + p64["ba"]
        pr = torch.softmax(z0, -1)
        act = torch.multinomial(pr, 1, generator=torch.Generator().manual_seed(c["seed"])).squeeze(1)      # on-policy: most rows take a probable item
        last, chunk0 = forced_actions(I)
        act[0::3] = last
        act[1::3] = chunk0
        lp0 = torch.log(pr.clamp(min=EPS32, max=1 - EPS32)).gather(1, act.view(-1, 1)).squeeze(1)      # what the rollout's Categorical.log_prob stores
    logp_old = (lp0 + noise).float()
    cols, moved = adjust(p, (obs, act, adv, ret, v_s, logp_old), hyper)
    # the buffer-order batch: the minibatch's rows scattered over n_rows rows in random order, NaN in every float column of the others
    n_rows = mb + EXTRA_ROWS
    idx = rng.permutation(n_rows)[:mb].astype(np.int32)
    n_env = 7
    max_turn = -(-n_rows // n_env)                    # n_env (max_turn + 1) >= n_rows cells of the tracker-gradient tensor
    cell = rng.permutation(n_env * (max_turn + 1))[:n_rows]
    batch = {}
    for k, col in zip(("obs", "adv", "ret", "v_s", "logp"), (cols[0], cols[2], cols[3], cols[4], cols[5])):
        full = torch.full((n_rows,) + tuple(col.shape[1:]), float("nan"), dtype=torch.float32)
        full[idx.astype(np.int64)] = col
        batch[k] = full
    a_full = torch.zeros(n_rows, dtype=torch.int32)
    a_full[idx.astype(np.int64)] = cols[1].int()
    batch["act"] = a_full
    return dict(name=name, I=I, mb=mb, n_rows=n_rows, hyper=hyper, rows_kernel=c["rows_kernel"], p=p, cols=cols, batch=batch, idx=idx,
                b_t=(cell // n_env).astype(np.int32), b_env=(cell % n_env).astype(np.int32), n_env=n_env, max_turn=max_turn, moved=moved)


def rel(a, b):
    """||a - b|| / ||b||; a reference that is identically zero (a shard whose only row has a clamped p_a has no head gradient) admits zero only."""
    if float(b.norm()) == 0.0:
        return 0.0 if float(a.norm()) == 0.0 else float("inf")
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def reference(name, share=None):
    """The float64 and fp32 evaluations of a case (share = (lo, hi): of that run of the index list's part of the global loss), computed once:
    dict(loss = the four float64 terms, g64 {name: gradient, "obs" included}, e32 {name: relative error of the fp32 torch evaluation})."""
    case = build(name)
    loss, g64 = loss_and_grads(case["p"], case["cols"], case["hyper"], torch.float64, share)
    _, g32 = loss_and_grads(case["p"], case["cols"], case["hyper"], torch.float32, share)
    if share is not None:      # d loss / d obs of the share: its own rows only (the others' is identically zero)
        g64["obs"], g32["obs"] = g64["obs"][slice(*share)], g32["obs"][slice(*share)]
    return dict(loss=loss, g64=g64, e32={k: rel(g32[k], g64[k]) for k in g64})


def grad_bar(e32):
    """test_gpu_head_precision's rule: as accurate as fp32, within a small factor of what a float32 evaluation loses against float64."""
    return max(4.0 * e32, 3e-6)


def head_bar(e32):
    """... and the head layer, where the bf16 pieces are used, at the fp32 level in absolute terms too."""
    return max(5e-6, 2.0 * max(e32["wa"], e32["ba"]))


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def make_learner(case, max_grad_norm=0.5):
    """A DeviceLearner holding the case's parameters and its buffer-order batch."""
    flat, _ = flat_policy_params(case["I"], init=None)
    flat.copy_(torch.cat([case["p"][k].flatten() for k in FLAT_ORDER]))
    hy = case["hyper"]
    ln = DeviceLearner(flat, case["I"], case["n_env"], case["max_turn"], gamma=0.99, gae_lambda=0.95, eps_clip=hy["eps_clip"], vf_coef=hy["vf_coef"],
                       ent_coef=hy["ent_coef"], max_grad_norm=max_grad_norm, lr=1e-3, norm_adv=hy["norm_adv"], value_clip=hy["value_clip"],
                       rew_norm=False, dual_clip=hy["dual_clip"])
    n, b = case["n_rows"], case["batch"]
    assert case["n_env"] * (case["max_turn"] + 1) >= n and int(case["b_t"].max()) <= case["max_turn"] and int(case["b_env"].max()) < case["n_env"]
    ln._alloc_batch(n)
    ln.n_rows = n
    ln.b_obs[:n].copy_(b["obs"]); ln.b_act[:n].copy_(b["act"]); ln.b_adv[:n].copy_(b["adv"]); ln.b_ret[:n].copy_(b["ret"])
    ln.b_vs[:n].copy_(b["v_s"]); ln.b_logp[:n].copy_(b["logp"])
    ln.b_env[:n].copy_(torch.as_tensor(case["b_env"])); ln.b_t[:n].copy_(torch.as_tensor(case["b_t"]))
    return ln


def split_flat(flat, I):
    """A flat [w1 | b1 | .. | bc] tensor -> {name: view}."""
    out, off = {}, 0
    for k, shp in shapes_of(I).items():
        n = int(np.prod(shp))
        out[k] = flat[off:off + n].view(shp)
        off += n
    return out


# ---- clip_grad_norm_ + Adam, fed the device's own gradient ---------------------------------------------------------------------------
# The float64 recurrence (oracle/nn_oracle.py:176-180, 325-333, adam_substeps): total norm with the trunk's squared norm counted twice,
# coef = min(1, max_norm / (norm + 1e-6)), trunk gradient * coef^2 and two sub-steps 2k + 1, 2k + 2, heads * coef and one step k + 1.
# The bars are gradcase's (M_BAR, V_BAR, V_TINY, P_BAR, UPD_BAR), widened by what the coefficient adds and by what a test cannot see:
#
# (1) the coefficient's own error e_c (relative).  sumsq_partial_kernel + norm_coef_block + clip_coef, counted in half-ulps (2^-24):
#       x * x                                   1    (the factor 2 of the trunk is exact)
#       a thread's sequential sum               n_seq = ceil(ceil(P / 256) / 256) additions
#       block_sum<256>'s tree                   8
#       part_a + part_b (+ 0: exact), the tree of norm_coef_block over the 256 slots: 8
#     every term is positive, so the sum's relative error is at most (1 + n_seq + 16) 2^-24; sqrtf halves it and adds 1, norm + 1e-6 adds 1,
#     the division 1:      e_c = ((17 + n_seq) / 2 + 3) 2^-24.            Without clipping coef is the constant 1: e_c = 0.
# (2) the scaled gradient: g * c (heads) is one more rounding, (g * c) * c (trunk) two:  e_g = pow (e_c + 2^-24), pow = 1 | 2.
#     Through m' = m + (1 - b1)(g - m) it adds (1 - b1) |g| e_g to the bar of m, through v' = b2 v + (1 - b2) g g it adds 2 (1 - b2) g g e_g to v's.
# (3) adam_elem's update p - ss * (m * rcp(sqrt(v) * rbc2s + eps)) in half-ulps: v_sqrt_f32 2, the product with rbc2s 1, rbc2s = fl(1 / s2)
#     against 1 / fl(s2) 2, + eps 1, v_rcp_f32 2, m * 1, ss * 1 = 10 <= the 32 of UPD_BAR = 2^-19: unchanged.
# (4) the trunk's first sub-step leaves no trace: its moments (m1, v1) and parameter are overwritten by the second.  The second sub-step's
#     moments are compared with the recurrence run twice, the bars propagated (m2 = b1 m1 + ..: b1 x the first bar + the second's own;
#     likewise b2 for v).  The parameter is p0 - upd1 - upd2: upd2 from the device's own final moments as gradcase does, upd1 from the
#     recurrence's (m1, v1), its uncertainty the interval of ss m / (sqrt(v) / bc2s + eps) over m1 +- bar, v1 +- bar.  p is rounded twice.
HALF_ULP = 2.0 ** -24


def coef_error(P, clips):
    n_seq = -(-(-(-P // 256)) // 256)
    return ((17 + n_seq) / 2.0 + 3.0) * HALF_ULP if clips else 0.0


def adam_reference(g, I, max_grad_norm):
    """-> (total norm, coef) in float64 from the flat device gradient g (float64 array)."""
    n_trunk = H * S + H + H * H + H
    sq = 2.0 * np.sum(g[:n_trunk] ** 2) + np.sum(g[n_trunk:] ** 2)
    norm = np.sqrt(sq)
    return norm, min(1.0, np.float64(np.float32(max_grad_norm)) / (norm + np.float64(np.float32(1e-6))))


def check_clip_adam(p0, m0, v0, g, m1, v1, p1, I, k, max_grad_norm, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, what=""):
    """Device moments / parameters after the step with opt_step = k (flat fp32 arrays as float64) against the recurrence fed the device's own
    gradient.  -> (coef, the largest share of the bars of m, v, p used)."""
    from gradcase import M_BAR, P_BAR, UPD_BAR, V_BAR, V_TINY, adam_constants, adam_moments, adam_update
    n_trunk = H * S + H + H * H + H
    P = len(g)
    norm, coef = adam_reference(g, I, max_grad_norm)
    e_c = coef_error(P, coef < 1.0)
    used = []
    for tag, sl, pw, steps in (("trunk", slice(0, n_trunk), 2, (2 * k + 1, 2 * k + 2)), ("heads", slice(n_trunk, P), 1, (k + 1,))):
        gs = g[sl] * coef ** pw
        e_g = pw * (e_c + HALF_ULP) if coef < 1.0 else 0.0
        rm, rv, rp = m0[sl], v0[sl], p0[sl]
        bm, bv = np.zeros_like(rm), np.zeros_like(rv)
        bp = np.zeros_like(rp)
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
        for name, d, bar in (("m", np.abs(m1[sl] - rm), bm), ("v", np.abs(v1[sl] - rv), bv), ("p", np.abs(p1[sl] - rp), bp)):
            ok = d <= bar
            i = int(np.argmax(d - bar))
            assert ok.all(), f"{what}: Adam {name} ({tag}): {int((~ok).sum())} entries outside the bar, worst at {i}: |diff| {d[i]:.3e} > {bar[i]:.3e}"
            with np.errstate(divide="ignore", invalid="ignore"):
                used.append(float(np.where(bar > 0, d / bar, 0.0).max()))
    return coef, dict(zip(("trunk_m", "trunk_v", "trunk_p", "heads_m", "heads_v", "heads_p"), used))
