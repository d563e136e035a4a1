"""DeviceVtbLearner: the VirtualTaobao PPO update (HostPPOPolicy.update of core/host_rl.py) on the GPU, csrc/vtb_learn.hip through
cirs_vtb_learn_prepare / cirs_vtb_learn_update.

The torch modules and optimisers stay authoritative between updates.  An update packs the tracker and policy parameters and their Adam
moments into flat fp32 images (torch's [out][in] layout, module registration order; one H2D copy), runs the whole update on the device
with the host-drawn row permutations, and writes everything back in place (p.data.copy_, the optimisers' state entries, ret_rms)
after one D2H copy.  Layout and refusals: cirs_hip/vtb_model.py and `check_optimisers` (pure host code, no library needed)."""
import ctypes as C
from typing import Dict, List

import numpy as np
import torch
from torch import nn

from .vtb_model import VtbModel, policy_tensors, stream, tracker_tensors, u64


# ---- the parameter images (pure host code) ----------------------------------------------------------------------------------
def policy_params(actor, critic) -> List[nn.Parameter]:
    """The policy image's parameters in order (vtb_model.py policy_tensors); refuses shapes the device learner does not build."""
    return [p for _, p in policy_tensors(actor, critic)]


def tracker_params(tracker) -> List[nn.Parameter]:
    """The tracker image's parameters in order (vtb_model.py tracker_tensors: HostStateTracker registration order)."""
    return [p for _, p in tracker_tensors(tracker)]


def check_optimisers(optim, ppar, tpar):
    """optim = [optim_RL, optim_state]: torch.optim.Adam(lr, betas, eps) only; optim_RL over the policy parameters with the shared
    trunk listed twice (actor + critic), optim_state over the tracker's.  -> the trunk's parameter count (multiplicity 2)."""
    if not isinstance(optim, (list, tuple)) or len(optim) != 2:
        raise ValueError("learner='device' needs optim = [optim_RL, optim_state] (policy and tracker optimisers)")
    for o in optim:
        if type(o) is not torch.optim.Adam:
            raise ValueError(f"learner='device' implements torch.optim.Adam only, got {type(o).__name__}")
        for g in o.param_groups:
            if g.get("amsgrad", False) or g.get("weight_decay", 0) != 0 or g.get("maximize", False):
                raise ValueError("learner='device' implements Adam(lr, betas, eps): amsgrad / weight_decay / maximize are not built")
            if g.get("differentiable", False) or g.get("capturable", False):
                raise ValueError("learner='device': differentiable / capturable Adam is not built")
        if len(o.param_groups) != 1:
            raise ValueError("learner='device' needs one parameter group per optimiser")
    count: Dict[int, int] = {}
    for p in optim[0].param_groups[0]["params"]:
        count[id(p)] = count.get(id(p), 0) + 1
    want = {id(p) for p in ppar}
    if set(count) != want:
        raise ValueError("optim_RL must hold exactly the actor's and the critic's parameters")
    n_trunk = 0
    for i, p in enumerate(ppar):
        if count[id(p)] == 2 and i == n_trunk:
            n_trunk += 1
        elif count[id(p)] != 1:
            raise ValueError("optim_RL: only the shared trunk may be listed twice")
    if {id(p) for p in optim[1].param_groups[0]["params"]} != {id(p) for p in tpar} or len(optim[1].param_groups[0]["params"]) != len(tpar):
        raise ValueError("optim_state must hold exactly the tracker's parameters")
    return n_trunk


def _hyper(o):
    g = o.param_groups[0]
    b1, b2 = g.get("betas", (0.9, 0.999))
    return float(g["lr"]), float(b1), float(b2), float(g.get("eps", 1e-8))


def pack_image(params, optim, dev=None):
    """(params, m, v, step) of a parameter list: one flat image each; empty optimiser state = zero moments, step 0.  All parameters of one
    image must share one step count."""
    flat = torch.cat([p.detach().reshape(-1).float() for p in params])
    ms, vs, steps = [], [], set()
    for p in params:
        st = optim.state.get(p, {})
        if "exp_avg" in st:
            ms.append(st["exp_avg"].detach().reshape(-1).float())
            vs.append(st["exp_avg_sq"].detach().reshape(-1).float())
            steps.add(int(float(st["step"])))
        else:
            ms.append(torch.zeros(p.numel()))
            vs.append(torch.zeros(p.numel()))
            steps.add(0)
    return flat, torch.cat(ms), torch.cat(vs), steps


def unpack_image(params, optim, flat, m, v, steps):
    """Write the images back in place: p.data.copy_ and the optimiser's state entries ("step" as torch keeps it)."""
    o = 0
    for p, s in zip(params, steps):
        n = p.numel()
        with torch.no_grad():
            p.data.copy_(flat[o:o + n].view_as(p))
        st = optim.state[p]
        if "exp_avg" in st:
            st["exp_avg"].copy_(m[o:o + n].view_as(p))
            st["exp_avg_sq"].copy_(v[o:o + n].view_as(p))
            if isinstance(st["step"], torch.Tensor):
                st["step"].fill_(float(s))
            else:
                st["step"] = float(s)
        else:
            st["step"] = torch.tensor(float(s), dtype=torch.float32)
            st["exp_avg"] = m[o:o + n].view_as(p).clone()
            st["exp_avg_sq"] = v[o:o + n].view_as(p).clone()
        o += n


def sample_layout(rows, size, lens, done_rows, unfinished):
    """Host tables of one sample: (t, env) per row, boundary flags, the exclusive ends of the GAE segments, and the CSR from (env, t) to
    the sample positions (a row may be drawn more than once when sample_size > 0)."""
    rows = np.asarray(rows, dtype=np.int64)
    env, t = rows // size, rows % size
    boundary = np.asarray(done_rows, bool) | np.isin(rows, unfinished)
    ends = np.flatnonzero(boundary) + 1
    if len(ends) == 0 or ends[-1] != len(rows):
        ends = np.r_[ends, len(rows)]
    return env, t, boundary, ends


class DeviceVtbLearner:
    """Workspace and launches of one update shape (n_env, max_turn) for a (tracker, actor, critic) triple."""

    def __init__(self, tracker, actor, critic, n_env, max_turn, device):
        from . import abi
        self.tracker, self.actor, self.critic = tracker, actor, critic
        self.model = VtbModel(tracker, actor, critic)
        self.ppar, self.tpar = [p for _, p in self.model.policy_tensors()], [p for _, p in self.model.tracker_tensors()]
        self.n_env, self.max_turn, self.device = int(n_env), int(max_turn), torch.device(device)
        self._lib, self._abi = abi.lib(), abi
        self.cfg = abi.VtbLearnCfg(n_env=self.n_env, max_turn=self.max_turn, model=self.model.model_cfg())
        self._rows_cap = 0
        self.ws = None
        self.pe = tracker.pos_encoder.pe[:, 0, :].detach().float().contiguous().to(self.device)
        self.rms = torch.zeros(3, dtype=torch.float64, device=self.device)

    def sizes(self, n_rows, redraw=False):
        self.cfg.n_rows, self.cfg.n_seg = int(n_rows), 1
        out = (C.c_int64 * 5)()
        name = "cirs_vtb_learn_redraw_sizes" if redraw else "cirs_vtb_learn_sizes"
        self._abi.check(getattr(self._lib, name)(C.byref(self.cfg), C.cast(out, C.c_void_p)), name)
        return [int(x) for x in out]

    # ---- one update ---------------------------------------------------------------------------------------------------------
    def prepare(self, policy, rows_src, rows, buffer):
        """Pack the host state, upload the sample tables and run the returns stage."""
        h = policy.hyper
        opt_p, opt_t = policy.optim
        dev = self.device
        n = len(rows)
        # the dropout key of the collect the rows come from: the forward pass regenerates that collect's masks, per position or, for a
        # dropout_redraw collect, per call (the workspace differs)
        m = self.cfg.model
        m.dropout_p, m.drop_env_base, m.dropout_seed = rows_src.dropout_p, rows_src.drop_env_base, u64(rows_src.dropout_seed)
        self.redraw = bool(getattr(rows_src, "dropout_redraw", False))
        sizes = self.sizes(n, self.redraw)
        n_trk, n_pol, n_ws = sizes[:3]
        self.n_trunk = check_optimisers(policy.optim, self.ppar, self.tpar)
        pflat, pm, pv, psteps = pack_image(self.ppar, opt_p)
        tflat, tm, tv, tsteps = pack_image(self.tpar, opt_t)
        trunk_steps = {int(float(opt_p.state[p]["step"])) if "step" in opt_p.state.get(p, {}) else 0 for p in self.ppar[:self.n_trunk]}
        head_steps = {int(float(opt_p.state[p]["step"])) if "step" in opt_p.state.get(p, {}) else 0 for p in self.ppar[self.n_trunk:]}
        if len(head_steps) != 1 or len(tsteps) != 1 or trunk_steps != {2 * next(iter(head_steps))}:
            raise ValueError("learner='device' needs one Adam step count per optimiser (the shared trunk at twice the heads')")
        assert pflat.numel() == n_pol and tflat.numel() == n_trk, "parameter image size differs from csrc/vtb_learn.hip"
        self.p_step0, self.t_step0 = next(iter(head_steps)), next(iter(tsteps))
        host = torch.cat([tflat, tm, tv, pflat, pm, pv]).pin_memory()
        img = host.to(dev, non_blocking=True)
        self._split = [n_trk] * 3 + [n_pol] * 3      # tracker image, m, v | policy image, m, v
        self.tflat, self.tm, self.tv, self.pflat, self.pm, self.pv = img.split(self._split)
        self.img = img
        # sample tables
        size = buffer.size
        env, t, boundary, ends = sample_layout(rows, size, rows_src.lens, np.asarray(buffer.done)[rows], buffer.unfinished_index())
        T = self.max_turn
        key = env * T + t
        order = np.argsort(key, kind="stable")
        starts = np.searchsorted(key[order], np.arange(self.n_env * T + 1))
        ints = np.concatenate([t, env, ends, order, starts]).astype(np.int32)
        self.ints = torch.as_tensor(ints).to(dev)
        self.bnd = torch.as_tensor(boundary.astype(np.uint8)).to(dev)
        oi = np.cumsum([0, 2 * n, len(ends), n, len(starts)])
        if self.ws is None or self.ws.numel() < n_ws:
            self.ws = torch.zeros(n_ws, dtype=torch.float32, device=dev)
        self.n_rows = n
        self.states_off, self.rowblk_off = sizes[3], sizes[4]
        self.rms.copy_(torch.tensor([policy.ret_rms.mean, policy.ret_rms.var, policy.ret_rms.count], dtype=torch.float64))
        c = self.cfg
        c.n_rows, c.n_seg = n, len(ends)
        c.scale_returns, c.whiten_adv, c.clip_value = int(h.scale_returns), int(h.whiten_adv), int(h.clip_value)
        c.has_dual, c.dual = int(bool(h.dual)), float(h.dual or 0.0)
        c.has_max_norm, c.max_norm = int(bool(h.max_norm)), float(h.max_norm or 0.0)
        c.clip, c.c_value, c.c_entropy = float(h.clip), float(h.c_value), float(h.c_entropy)
        c.discount, c.lam, c.floor = float(h.discount), float(h.lam), float(h.floor)
        c.lr, c.beta1, c.beta2, c.eps = _hyper(opt_p)
        c.t_lr, c.t_beta1, c.t_beta2, c.t_eps = _hyper(opt_t)
        tr = rows_src.rollout.traj
        p = lambda x: x.data_ptr()      # noqa: E731
        base = self.ints.data_ptr()
        self.bufs = self._abi.VtbLearnBufs(tparams=p(self.tflat), t_m=p(self.tm), t_v=p(self.tv), pparams=p(self.pflat), p_m=p(self.pm),
                                           p_v=p(self.pv), pe=p(self.pe), obs0=p(tr["obs0"]), obs=p(tr["obs"]), rew=p(tr["rew"]),
                                           done=p(tr["done"]), act=p(tr["act"]), len=p(tr["len"]), rows=base, boundary=p(self.bnd),
                                           seg_end=base + 4 * int(oi[1]), grad_rows=base + 4 * int(oi[2]), grad_start=base + 4 * int(oi[3]),
                                           rms=p(self.rms), ws=p(self.ws), losses=0)
        name = "cirs_vtb_learn_prepare_redraw" if self.redraw else "cirs_vtb_learn_prepare"
        self._abi.check(getattr(self._lib, name)(C.byref(c), C.byref(self.bufs), stream(self.device)), name)

    def states(self):
        """The learner's tracker states [max_turn + 1, n_env, dim_state] of the last prepare (device view)."""
        o, T, B, S = self.states_off, self.max_turn, self.n_env, self.cfg.model.dim_state
        return self.ws[o:o + (T + 1) * B * S].view(T + 1, B, S)

    def row_block(self):
        """(v_s, adv, returns, logp_old) [n_rows] each of the last returns stage (device views)."""
        o, n = self.rowblk_off, self.n_rows
        return tuple(self.ws[o + i * n:o + (i + 1) * n] for i in range(4))

    def learn(self, policy, perms, batch_size, repeat):
        """The passes and the tracker step; then one D2H copy of losses, images and ret_rms, written back into the host objects."""
        from core.host_rl import row_ranges
        n = self.n_rows
        n_mb = len(row_ranges(n, batch_size)) * repeat
        perm_d = torch.as_tensor(np.stack(perms).astype(np.int32)).to(self.device)
        losses = torch.zeros((n_mb, 4), dtype=torch.float32, device=self.device)
        self.bufs.losses = losses.data_ptr()
        name = "cirs_vtb_learn_update_redraw" if self.redraw else "cirs_vtb_learn_update"
        self._abi.check(getattr(self._lib, name)(C.byref(self.cfg), C.byref(self.bufs), perm_d.data_ptr(), int(repeat), int(batch_size),
                                                 int(bool(policy.hyper.refresh_adv)), int(self.p_step0), int(self.t_step0),
                                                 stream(self.device)), name)
        back = torch.cat([self.img, losses.reshape(-1)]).cpu()
        rms = self.rms.cpu().numpy()
        n_img = self.img.numel()
        img, lo = back[:n_img], back[n_img:n_img + 4 * n_mb].view(n_mb, 4).numpy()
        tflat, tm, tv, pflat, pm, pv = img.split(self._split)
        opt_p, opt_t = policy.optim
        k = n_mb
        unpack_image(self.tpar, opt_t, tflat, tm, tv, [self.t_step0 + 1] * len(self.tpar))
        unpack_image(self.ppar, opt_p, pflat, pm, pv,
                     [2 * (self.p_step0 + k)] * self.n_trunk + [self.p_step0 + k] * (len(self.ppar) - self.n_trunk))
        if policy.hyper.scale_returns:
            policy.ret_rms.mean, policy.ret_rms.var, policy.ret_rms.count = float(rms[0]), float(rms[1]), float(rms[2])
        return {"loss": lo[:, 0].tolist(), "loss/clip": lo[:, 1].tolist(), "loss/vf": lo[:, 2].tolist(), "loss/ent": lo[:, 3].tolist()}
