"""The four slot trackers (GRU, LSTM, Avg, Caser) described once each for their GPU tests (a helper, not a test): what differs between them
-- the case module, the float64 restatement, the model arguments, the engine and plugin classes, the example's flags -- and the procedures
tests/test_gpu_slot_{tracker,rollout,plugin}.py share: the teacher-forced replay, the backward's arguments, the stepwise collect and its
checks.

`model` is what a tracker has beyond (U, I, B, T, S): the layer count L of GRU / LSTM, the window W of Avg, (W, heights) of Caser."""
import functools
import importlib.util
import os

import numpy as np
import torch

import avgcase
import casercase
import grucase
import lstmcase
from cirs_hip import avg_host, caser_host, gru_host, lstm_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I, T, S = 200, 300, 8, 20      # the rollout tests' sizes.  I = 300: not a multiple of the sampler's 128-item chunk
SEED, RNG_BASE = 1234, 40


class Slot:
    """One tracker.  A subclass sets the names and modules and says how its model arguments reach each callee."""
    name = display = entry = None      # "gru", "GRU" (what the refusals call it), "cirs_gru_tracker" (the prefix of its backward entry points)
    case = host = None                 # grucase, cirs_hip.gru_host
    short_ws_case = 0                  # the case of the short-workspace test
    carried = ()                       # engine attributes that hold what an env carries between steps, where the restatement reports them
    walk = ()                          # ((B, T, model, parameter seed), ...): the many-env cases, at U, I, S = 50, 80, 20
    rollout_model = rollout_seed = None      # the rollout tests: model arguments (T = 8), parameter seed
    example_model = None               # ... and the model arguments of the example it builds in its refusal test
    plugin_model, plugin_seed = None, 4      # tests/test_gpu_slot_plugin.py
    state_names = ()                   # state_dict names written out: torch's for the recurrence, the reference's for the rest

    def __repr__(self):
        return self.name

    @property
    def CASES(self):
        return self.case.CASES

    @property
    def IDS(self):
        return self.case.IDS

    def split(self, case):
        """(U, I, B, T, S, hot), model"""
        Uc, Ic, B, Tc, model, Sc, hot = case
        return (Uc, Ic, B, Tc, Sc, hot), model

    def params(self, ci):
        (Uc, Ic, _, _, Sc, _), model = self.split(self.CASES[ci])
        return self.param_dict(Uc, Ic, 3, Sc, model)

    def states(self, p, users, acts, rews, model, dtype, carried=None):
        """states [B, T+1, S] of the restatement at `dtype`; `carried`: a dict that receives what self.carried names, [L, B, T+1, D] each"""
        return self.host.states(self.host.cast_params(p, dtype), users, acts, rews, self.host_arg(model)).numpy()

    def grads(self, p, users, acts, rews, lens, G, model, dtype):
        return self.host.grads(p, users, acts, rews, lens, G, self.host_arg(model), dtype)

    def host_arg(self, model):
        return model

    def flags(self, model):
        """the example's flags for `model`, after --tracker <name>"""
        return []

    def plugin_kw(self, model):
        """the plugin class's keywords for `model`, which are the attributes it shows"""
        return {}

    def tracker_class(self):
        import core.state_tracker
        return getattr(core.state_tracker, "StateTracker" + self.display)

    def engine_refusals(self, params):
        """(exception, pattern, thunk) of what the engine's constructor refuses, at the rollout test's sizes"""
        return []

    def check_unambiguous(self, p, users, acts, rews, lens, model):
        """Where the model is not smooth: the inputs must be ones at which float64 itself is unambiguous."""


class _Recurrent(Slot):
    rollout_model, rollout_seed, example_model, plugin_model = 1, 2, 1, 1

    def n_grad_tensors(self, model):
        return 8 + 4 * model      # weight_ih, weight_hh, bias_ih, bias_hh per layer around the eight tensors every slot tracker has

    def plugin_kw(self, model):
        return {"nlayers": model}


class Gru(_Recurrent):
    name, display, entry, case, host = "gru", "GRU", "cirs_gru_tracker", grucase, gru_host
    IDS = [f"U{c[0]}-I{c[1]}-B{c[2]}-T{c[3]}-L{c[4]}-S{c[5]}" + ("-hot" if c[6] else "") for c in grucase.CASES]
    state_names = ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "embedding_dict.feat_item.weight", "decoder.bias")
    walk = ((4100, 3, 1, 5), (2060, 3, 2, 5))      # more than 4 x workgroups-per-CU x CUs of a 256-CU part: 4096 with one layer, 2048 with two

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return grucase.gru_param_dict(Uc, Ic, seed=seed, S=Sc, nlayers=model)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.gru_tracker import gru_param_shapes
        return gru_param_shapes(Uc, Ic, 32, Sc, model)

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return grucase.device_gru_trainable(p, Uc, Ic, B, Tc, model, Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.gru_tracker import DeviceGruTracker
        return DeviceGruTracker(params, Uc, Ic, B, Tc, dim_state=Sc, nlayers=model)


class Lstm(_Recurrent):
    name, display, entry, case, host = "lstm", "LSTM", "cirs_lstm_tracker", lstmcase, lstm_host
    short_ws_case = 1
    carried = ("h", "c")
    state_names = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "embedding_dict.feat_item.weight", "decoder.bias")
    walk = ((3073, 3, 1, 5), (2049, 3, 2, 5))      # one env more than 4 x workgroups-per-CU x CUs: 3 per CU = 3072 with one layer, 2 per CU = 2048 with two

    def states(self, p, users, acts, rews, model, dtype, carried=None):
        return lstm_host.states(lstm_host.cast_params(p, dtype), users, acts, rews, model, carried).numpy()

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return lstmcase.lstm_param_dict(Uc, Ic, seed=seed, S=Sc, nlayers=model)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.lstm_tracker import lstm_param_shapes
        return lstm_param_shapes(Uc, Ic, 32, Sc, model)

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return lstmcase.device_lstm_trainable(p, Uc, Ic, B, Tc, model, Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.lstm_tracker import DeviceLstmTracker
        return DeviceLstmTracker(params, Uc, Ic, B, Tc, dim_state=Sc, nlayers=model)


class Avg(Slot):
    name, display, entry, case, host = "avg", "Avg", "cirs_avg_tracker", avgcase, avg_host
    walk = ((8200, 4, 3, 5),)      # more than 8 x workgroups-per-CU x CUs (4 per CU: 8192); T = 4 with W = 3: windows of one, two and three slots
    rollout_model, rollout_seed, plugin_model = 3, 2, 3      # T = 8: the window slides from position 4 on
    example_model = 2
    state_names = ("embedding_dict.feat_user.weight", "embedding_dict.feat_item.weight", "ffn_user.weight", "ffn_user.bias", "fnn_gate.weight",
                   "fnn_gate.bias", "decoder.weight", "decoder.bias")      # all eight

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return avgcase.avg_param_dict(Uc, Ic, seed=seed, S=Sc)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.avg_tracker import avg_param_shapes
        return avg_param_shapes(Uc, Ic, 32, Sc)

    def n_grad_tensors(self, model):
        return 8

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return avgcase.device_avg_trainable(p, Uc, Ic, B, Tc, model, Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.avg_tracker import DeviceAvgTracker
        return DeviceAvgTracker(params, Uc, Ic, B, Tc, dim_state=Sc, window_size=model)

    def flags(self, model):
        return ["--window-size", str(model)]

    def plugin_kw(self, model):
        return {"window_size": model}

    def engine_refusals(self, params):
        return [(ValueError, "window_size", lambda: self.engine(params, U, I, 6, T, S, 0))]


class Caser(Slot):
    name, display, entry, case, host = "caser", "Caser", "cirs_caser_tracker", casercase, caser_host
    # more than 4 x workgroups-per-CU x CUs (2 per CU: 2048); T = 4 with W = 3 and heights (1, 3): windows with three, two, one and no zero
    # rows.  States only: they are continuous at every max and ReLU, so the near-tie condition of the gradient tests is not needed there
    walk = ((2056, 4, (3, (1, 3)), 5),)
    rollout_model, rollout_seed = (4, (2, 3)), 2      # T = 8: the window slides from position 5 on
    plugin_model = (4, (2, 3))
    example_model = (3, (1, 3))
    state_names = ("horizontal_cnn.0.weight", "horizontal_cnn.1.bias", "vertical_cnn.weight", "vertical_cnn.bias", "fc.weight", "fc.bias",
                   "embedding_dict.feat_item.weight", "decoder.bias")

    def split(self, case):
        Uc, Ic, B, Tc, W, heights, Sc, hot = case
        return (Uc, Ic, B, Tc, Sc, hot), (W, heights)

    def params(self, ci):
        return casercase.case_params(ci)      # the per-case SEEDS: the near-tie condition depends on them

    def host_arg(self, model):
        return model[0]      # the restatement reads the heights off the parameters

    def param_dict(self, Uc, Ic, seed, Sc, model):
        return casercase.caser_param_dict(Uc, Ic, seed, model[0], model[1], S=Sc)

    def param_shapes(self, Uc, Ic, Sc, model):
        from cirs_hip.caser_tracker import caser_param_shapes
        return caser_param_shapes(Uc, Ic, 32, Sc, model[0], model[1])

    def n_grad_tensors(self, model):
        return 12 + 2 * len(model[1])

    def device_trainable(self, p, Uc, Ic, B, Tc, model, Sc):
        return casercase.device_caser_trainable(p, Uc, Ic, B, Tc, model[0], model[1], Sc)

    def engine(self, params, Uc, Ic, B, Tc, Sc, model):
        from cirs_hip.caser_tracker import DeviceCaserTracker
        return DeviceCaserTracker(params, Uc, Ic, B, Tc, dim_state=Sc, window_size=model[0], filter_sizes=model[1])

    def flags(self, model):
        return ["--window-size", str(model[0]), "--filter-sizes", ",".join(map(str, model[1]))]

    def plugin_kw(self, model):
        return {"window_size": model[0], "filter_sizes": model[1]}

    def engine_refusals(self, params):
        return [(ValueError, "window_size", lambda: self.engine(params, U, I, 6, T, S, (17, self.rollout_model[1])))]

    def check_unambiguous(self, p, users, acts, rews, lens, model):
        for what, (margin, e32) in casercase.near_tie_margins(p, users, np.maximum(acts, 0), rews, lens, model[0]).items():
            assert margin >= 8 * e32, f"the rollout's inputs sit near a tie ({what}): choose another parameter seed"


GRU, LSTM, AVG, CASER = SLOTS = [Gru(), Lstm(), Avg(), Caser()]
NAMES = [s.name for s in SLOTS]


def errors32(slot, p, users, acts, rews, lens, model, Tc):
    """float64 states, the live mask (position < lens), their scale, the float32 restatement's own error, and what is carried at both dtypes"""
    c64, c32 = {}, {}
    s64 = slot.states(p, users, acts, rews, model, torch.float64, c64)
    s32 = slot.states(p, users, acts, rews, model, torch.float32, c32)
    live = np.arange(Tc + 1)[None, :] < lens[:, None]
    scale = np.abs(s64[live]).max()
    b = np.arange(len(lens))
    last = lambda c: {k: v.numpy()[:, b, lens - 1] for k, v in c.items()}  # noqa: E731  [L, B, D] of every env's last position
    return s64, live, scale, float(np.abs(s32[live] - s64[live]).max() / scale), last(c64), last(c32)


@functools.lru_cache(maxsize=None)
def reference(slot, ci):
    """Computed once per (tracker, case) and shared: parameters, inputs, the float64 states / carried tensors / gradients and the float32
    restatement's own error."""
    (Uc, Ic, B, Tc, Sc, hot), model = slot.split(slot.CASES[ci])
    p = slot.params(ci)
    users, acts, rews, lens, rng = slot.case.teacher_inputs(Uc, Ic, B, Tc, hot)
    G = rng.normal(size=(Tc + 1, B, Sc)).astype(np.float32)
    s64, live, s_scale, s_err32, c64, c32 = errors32(slot, p, users, acts, rews, lens, model, Tc)
    c_err32 = {k: float(np.abs(c32[k] - c64[k]).max() / np.abs(c64[k]).max()) for k in c64}
    g64 = slot.grads(p, users, acts, rews, lens, G, model, torch.float64)
    g32 = slot.grads(p, users, acts, rews, lens, G, model, torch.float32)
    g_err32 = {k: float(np.abs(g32[k] - g64[k]).max() / (np.abs(g64[k]).max() + 1e-300)) for k in g64}
    return dict(p=p, users=users, acts=acts, rews=rews, lens=lens, G=G, s64=s64, live=live, s_scale=s_scale, s_err32=s_err32, c64=c64,
                c_err32=c_err32, g64=g64, g_err32=g_err32)


def replayed(slot, ci, mode="env_ids"):
    """the case's engine after the teacher-forced replay, and the states it gave"""
    (Uc, Ic, B, Tc, Sc, hot), model = slot.split(slot.CASES[ci])
    ref = reference(slot, ci)
    trk, _ = slot.device_trainable(ref["p"], Uc, Ic, B, Tc, model, Sc)
    return trk, replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], mode)


def replay(trk, users, acts, rews, lens, mode):
    """reset / init / step, teacher-forced: env b gets positions 0 .. lens[b] - 1.  Finished envs are dropped through env_ids (the live rows
    only, in descending env order) or kept in the batch and marked (skip on even steps, item -1 on odd ones).  Returns states [B, T+1, S],
    NaN where no state was produced."""
    B, Tc = acts.shape
    Sc = trk.dim_state
    out = np.full((B, Tc + 1, Sc), np.nan, np.float32)
    trk.reset()
    out[:, 0] = trk.init(torch.as_tensor(users)).cpu().numpy()
    for t in range(Tc):
        live = np.where(lens > t + 1)[0]
        if len(live) == 0:
            break
        if mode == "env_ids":
            ids = live[::-1].copy()
            buf = torch.full((len(ids), Sc), float("nan"), device="cuda")
            trk.step(torch.as_tensor(acts[ids, t]), torch.as_tensor(rews[ids, t]), env_ids=torch.as_tensor(ids.astype(np.int32)).cuda(), out=buf,
                     out_stride=Sc)
            out[ids, t + 1] = buf.cpu().numpy()
        else:
            dead = lens <= t + 1
            buf = torch.full((B, Sc), float("nan"), device="cuda")      # the sentinel: rows of finished envs must keep it
            if t % 2 == 0:
                trk.step(torch.as_tensor(acts[:, t]), torch.as_tensor(rews[:, t]), skip=torch.as_tensor(dead.astype(np.uint8)).cuda(), out=buf, out_stride=Sc)
            else:
                trk.step(torch.as_tensor(np.where(dead, -1, acts[:, t])), torch.as_tensor(rews[:, t]), out=buf, out_stride=Sc)
            got = buf.cpu().numpy()
            assert np.isnan(got[dead]).all(), "a finished env's row of state_out was written"
            out[:, t + 1] = got
    return out


def backward_args(ref, Tc, B, Sc):
    """the arguments of an engine's backward() for the reference's inputs: users, the trajectory, the buffer rows, the upstream gradient"""
    from cirs_hip.rollout import Trajectory
    lens, acts, rews = ref["lens"], ref["acts"], ref["rews"]
    traj = Trajectory(B, Tc, Sc, "cuda")
    a = np.where(np.arange(Tc)[None, :] < lens[:, None] - 1, acts, -1)      # position p reads action p - 1: lens - 1 actions per env
    traj.act.copy_(torch.as_tensor(a.T.copy())); traj.rew.copy_(torch.as_tensor(rews.T.copy()))
    offsets, row_env, row_t = grucase.rows_of(lens)
    d = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    return (torch.as_tensor(ref["users"]), traj, d(row_env), d(row_t), d(offsets), d(lens.astype(np.int32)), int(lens.sum()), d(ref["G"]))


def load_example():
    spec = importlib.util.spec_from_file_location("cirs_rl_kuaishou_synth", os.path.join(ROOT, "examples", "cirs_rl_kuaishou_synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_stack(slot, tab, B, **rollout_kw):
    """DeviceRollout over the slot's engine at the rollout tests' sizes, and the tracker's parameters"""
    import envcase
    import policycase
    import rolloutcase
    from cirs_hip.env import DeviceEnv, DeviceEnvTables
    from cirs_hip.policy import DevicePolicy
    from cirs_hip.rollout import DeviceRollout
    a_env, b_env = envcase.ab_env_tables(tab.raw_uid, tab.raw_pid, tab.alpha_u, tab.beta_i, U, I)
    dt = DeviceEnvTables(tab.mat, tab.normed_mat, tab.item_cats, alpha_env=a_env, beta_env=b_env)
    env = DeviceEnv(dt, B, num_leave_compute=3, leave_threshold=1, max_turn=T, tau=10.0, gamma_exposure=10.0, version="v1")
    p = slot.param_dict(U, I, slot.rollout_seed, S, slot.rollout_model)
    trk = slot.engine({k: v.float().cuda().contiguous() for k, v in p.items()}, U, I, B, T, S, slot.rollout_model)
    arrs = policycase.random_weights(np.random.RandomState(2), I)
    pol = DevicePolicy({rolloutcase.POLICY_NAMES[k]: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in arrs.items()}, I)
    return DeviceRollout(env, trk, pol, **rollout_kw), p


def stepwise(ro, users, *, greedy=False, remove=False, force_length=0):
    """The collect, one public entry point at a time from Python (DeviceEnv.reset / step, DevicePolicy.sample / greedy, the engine's init / step)."""
    env, trk, pol = ro.env, ro.tracker, ro.policy
    B = env.n_env
    dev = env.device
    obs = torch.zeros((T + 1, B, S), device=dev)
    act = torch.zeros((T, B), dtype=torch.int64, device=dev); rew = torch.zeros((T, B), dtype=torch.float64, device=dev)
    done = torch.zeros((T, B), dtype=torch.uint8, device=dev); ctr = torch.zeros((T, B), dtype=torch.float64, device=dev)
    logp = torch.zeros((T, B), device=dev); value = torch.zeros((T, B), device=dev)
    visited = torch.zeros((B, (I + 31) // 32), dtype=torch.int32, device=dev) if remove else None
    users_d = torch.as_tensor(users).to(dev, torch.int32)
    env.reset(users_d)
    trk.reset()
    trk.init(users_d, out=obs[0], out_stride=S)
    rows = torch.arange(B, device=dev)
    for t in range(T):
        kw = dict(visited=visited, skip=env.done, act_out=act[t], logp_out=logp[t], value_out=value[t])
        if greedy:
            pol.greedy(obs[t], **kw)
        else:
            pol.sample(obs[t], seed=SEED, rng_step=RNG_BASE + t, **kw)
        if remove:
            ok = act[t] >= 0
            a = act[t].clamp(min=0)
            bit = torch.ones_like(a) << (a & 31)
            bit = torch.where(bit >= 2 ** 31, bit - 2 ** 32, bit).to(torch.int32)
            visited[rows[ok], (a >> 5)[ok]] |= bit[ok]
        _, r, d, c, _ = env.step(act[t])
        if force_length > 0:
            fd = 1 if t + 1 >= force_length else 0
            ok = act[t] >= 0
            env.done[ok] = fd
            d[ok] = fd
        rew[t], done[t], ctr[t] = r, d, c
        trk.step(act[t], r, out=obs[t + 1], out_stride=S)
    return dict(obs=obs, act=act, rew=rew, done=done, logp=logp, value=value, ctr=ctr, lengths=env.turn.clone())


def assert_same(ro, lengths, want):
    for k in ("obs", "act", "rew", "done", "logp", "value", "ctr"):
        assert torch.equal(getattr(ro.traj, k), want[k]), k
    assert torch.equal(lengths, want["lengths"]), "lengths"


def check_contract(ro, lengths):
    """after an env's done: act -1, rew 0; before: a valid item"""
    act, rew, done = ro.traj.act.cpu().numpy(), ro.traj.rew.cpu().numpy(), ro.traj.done.cpu().numpy()
    ln = lengths.cpu().numpy()
    for b in range(act.shape[1]):
        assert 1 <= ln[b] <= T, (b, ln[b])
        assert (act[:ln[b], b] >= 0).all() and (act[:ln[b], b] < I).all(), (b, act[:, b])
        assert done[ln[b] - 1, b] == 1 and (done[:ln[b] - 1, b] == 0).all(), (b, ln[b], done[:, b])
        assert (act[ln[b]:, b] == -1).all() and (rew[ln[b]:, b] == 0).all() and (done[ln[b]:, b] == 1).all(), (b, ln[b], act[:, b], rew[:, b], done[:, b])


def check_against_float64(slot, ro, p, users, lengths):
    """the independent check: the float64 restatement, teacher-forced on the device's users / acts / rews, reproduces traj.obs"""
    act = ro.traj.act.cpu().numpy().T.copy(); rew = ro.traj.rew.cpu().numpy().T.copy()
    ln = lengths.cpu().numpy()
    s64 = slot.states(p, users, act, rew, slot.rollout_model, torch.float64)
    s32 = slot.states(p, users, act, rew, slot.rollout_model, torch.float32)
    live = np.arange(T + 1)[None, :] <= ln[:, None]      # an env of length n has states 0 .. n
    got = ro.traj.obs.cpu().numpy().transpose(1, 0, 2)
    scale = np.abs(s64[live]).max()
    err, err32 = np.abs(got[live] - s64[live]).max() / scale, np.abs(s32[live] - s64[live]).max() / scale
    bar = slot.case.bar_for(slot.case.STATE_BAR, err32)
    print(f"rollout obs {slot.name} B={len(ln)}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
    assert err <= bar, f"rollout obs {slot.name} B={len(ln)}: device {err:.3e} over the bar {bar:.3e} (float32 restatement {err32:.3e})"
