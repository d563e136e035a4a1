"""DeviceVtbCollector: `Collector(policy, env, buffer, preprocess_fn=tracker.build_state, rollout="device")` over a VirtualTaobao vector env
built with `device=` (BASELINE configs[0] shapes).  Same public surface and result dict as core.host_rl.HostCollector, but a collect is one
cirs_vtb_rollout_collect call (cirs_hip/vtb_rollout.py): the tracker, the actor and the env all step on the GPU, finished envs are dropped.

With a buffer (training collector) the states the learner back-propagates through are rebuilt afterwards in ONE teacher-forced causal pass
of the tracker in torch (cirs_hip/vtb_host.py) with the collect's own dropout masks, and the VectorReplayBuffer is filled in the per-env
segment order HostCollector's per-step adds produce, so HostPPOPolicy.update and onpolicy_trainer run unchanged.  Without a buffer (test
collector) nothing is rebuilt.

dropout_redraw=True: the reference's own dropout procedure -- every build_state call runs the whole prefix again with fresh masks -- instead
of one mask per position for the rest of the episode (cirs_vtb_rollout_collect_redraw); the rebuilt states are then one pass per call
(vtb_host.redraw_states) and the device learner back-propagates through each call's own graph."""
import time
from typing import Any, Callable, Dict, List, Optional

import numpy as np
import torch

from tianshou.data import Batch, VectorReplayBuffer

_MIX = 0x9E3779B97F4A7C15


def _splitmix64(x: int) -> int:
    x = (x + _MIX) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def check_device_vtb(policy, env, preprocess_fn):
    """Raise a clear error unless (device VirtualTB vector env, HostStateTracker.build_state, HostPPOPolicy over ActorProb)."""
    from core.host_rl import HostPPOPolicy, HostStateTracker
    if not getattr(env, "host_mode", False):
        raise ValueError("rollout='device' runs the VirtualTaobao rollout; KuaishouEnv vector envs always collect on the device "
                         "(build the Collector without rollout=)")
    if getattr(env, "_vtb_device", None) is None:
        raise ValueError("rollout='device' needs a VirtualTaobao vector env built with DummyVectorEnv(..., device='cuda')")
    tracker = getattr(preprocess_fn, "__self__", None)
    if not isinstance(tracker, HostStateTracker) or getattr(preprocess_fn, "__name__", "") != "build_state":
        raise ValueError("rollout='device' needs preprocess_fn=tracker.build_state of the VirtualTB-v0 StateTrackerTransformer")
    if not isinstance(policy, HostPPOPolicy):
        raise ValueError("rollout='device' needs the VirtualTB-v0 PPOPolicy (core.host_rl.HostPPOPolicy)")
    if policy.action_type != "continuous":
        raise ValueError("rollout='device' needs a continuous ActorProb actor with an Independent(Normal) policy; "
                         "discrete actors are collected by the host loop")
    from cirs_hip.vtb_model import VtbModel
    VtbModel(tracker, policy.actor)      # the actor's class and shape: refused here, before anything touches the GPU
    return tracker


class DeviceVtbCollector:
    def __init__(self, policy, env, buffer: Optional[VectorReplayBuffer] = None, preprocess_fn: Optional[Callable[..., Any]] = None,
                 exploration_noise: bool = False, remove_recommended_ids=False, force_length=0, dropout_redraw=False):
        self.tracker = check_device_vtb(policy, env, preprocess_fn)
        if not isinstance(dropout_redraw, (bool, np.bool_)):
            raise TypeError(f"dropout_redraw must be a bool, got {dropout_redraw!r}")
        self.dropout_redraw = bool(dropout_redraw)
        if remove_recommended_ids:
            raise ValueError("remove_recommended_ids is a discrete-catalogue feature (KuaishouEnv)")
        self.policy, self.env, self.preprocess_fn = policy, env, preprocess_fn
        self.env_num = len(env)
        # (exploration_noise: HostPPOPolicy.exploration_noise is the identity, so the flag changes nothing)
        self.options = dict(noise=bool(exploration_noise), mask_seen=False, horizon=int(force_length))
        self._keep_buffer = buffer is not None
        self.buffer = VectorReplayBuffer(self.env_num, self.env_num) if buffer is None else buffer
        assert self.buffer.buffer_num >= self.env_num, "one sub-buffer per env"
        # the Gaussian and dropout keys of this collector come from torch's generator (torch.manual_seed determines them)
        self._key = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self._collect_count = 0
        self._rollout = None
        self.reset()

    exploration_noise = property(lambda self: self.options["noise"])
    remove_recommended_ids = property(lambda self: self.options["mask_seen"])
    force_length = property(lambda self: self.options["horizon"])

    # ---- HostCollector's hooks ---------------------------------------------------------------------------------------------
    def reset_stat(self):
        self.collect_step = self.collect_episode = 0
        self.collect_time = 0.0

    def reset_buffer(self, keep_statistics=False):
        self.buffer = type(self.buffer)(self.buffer.maxsize, self.buffer.buffer_num)      # every collect fills a brand-new buffer

    def reset_env(self):
        pass      # every collect resets all envs on the device (cirs_vtb_rollout_collect)

    def reset(self):
        for hook in (self.reset_env, self.reset_buffer, self.reset_stat):
            hook()

    def rollout(self):
        if self._rollout is None:
            from cirs_hip.vtb_rollout import DeviceVtbRollout
            self._rollout = DeviceVtbRollout(self.env.vtb_env(), self.tracker, self.policy.actor, self.policy,
                                             force_length=self.options["horizon"], dropout_redraw=self.dropout_redraw)
        return self._rollout

    def keys(self, collect_id):
        """(Gaussian key, dropout key) of collect number `collect_id`."""
        return self._key, _splitmix64(self._key ^ ((collect_id + 1) * _MIX & 0xFFFFFFFFFFFFFFFF))

    # ---- collect ---------------------------------------------------------------------------------------------------------------
    def collect(self, n_step=None, n_episode=None, random=False, render=None, no_grad=True) -> Dict[str, Any]:
        if random:
            raise NotImplementedError("collect(random=True) runs on the host loop: build the Collector without rollout='device'")
        assert n_step is None and n_episode is not None, "the CIRS scripts collect whole episodes (n_episode)"
        if n_episode != self.env_num:
            raise ValueError("n_episode must equal the number of envs (finished envs are not reset, SURVEY Q4)")
        greedy = bool(self.policy._deterministic_eval and not self.policy.training)      # the mean action (core/policy/ppo.py:152-153)
        self.reset()
        clock = time.time()
        ro = self.rollout()
        cid = self._collect_count
        seed, dseed = self.keys(cid)
        lens = ro.collect(seed, cid, dropout_seed=dseed, greedy=greedy)
        self._collect_count += 1
        self.last_collect = (seed, cid, dseed)
        tr = {k: ro.traj[k].cpu() for k in ("obs0", "obs", "rew", "done", "ctr", "act", "state")}
        from core.vtb_learner import DeviceVtbPPOPolicy
        if self._keep_buffer and isinstance(self.policy, DeviceVtbPPOPolicy):
            res = self._fill_device(ro, tr, lens, (seed, cid, dseed))
        elif self._keep_buffer:
            res = self._fill_buffer(ro, tr, lens, dseed)
        else:
            res = self._summary_only(tr, lens)
        self.collect_time += max(time.time() - clock, 1e-9)
        self.collect_step += res["n/st"]
        self.collect_episode += res["n/ep"]
        return res

    def rebuild_states(self, ro, tr, lens, dropout_seed):
        """The states [Tm+1, B, S] of the last collect, with the tracker's autograd graph (Tm = the longest episode)."""
        Tm = int(lens.max())
        B = self.env_num
        user = tr["obs0"][:, :-3].to(torch.float32)
        rew = tr["rew"][:Tm].to(torch.float32)                     # fp64 -> fp32 once, as torch.as_tensor(rew, float32)
        act = tr["obs"][:Tm, :, :-3].to(torch.float32)             # the action columns of obs_next
        from cirs_hip.vtb_host import redraw_states, tracker_states
        with torch.enable_grad():
            if self.dropout_redraw and ro.dropout_p > 0:
                return redraw_states(self.tracker, user, rew, act, lambda c: ro.call_masks(dropout_seed, c))
            masks = ro.masks(dropout_seed, Tm + 1, n_env=B) if ro.dropout_p > 0 else None
            return tracker_states(self.tracker, user, rew, act, masks)

    def _transitions(self, tr, lens):
        """Per vector step: (active env ids ascending, rew, done, info) -- the order of HostCollector's cohort."""
        simulated = self.env.vtb_env().simulated
        for t in range(int(lens.max())):
            ids = np.flatnonzero(lens > t)
            rew = tr["rew"][t, ids].numpy()
            if not simulated:
                rew = rew.astype(np.int64)     # the raw env's reward is the click count (an int)
            yield t, ids, rew, tr["done"][t, ids].numpy().astype(bool), Batch(CTR=tr["ctr"][t, ids].numpy(), env_id=ids)

    def _fill_buffer(self, ro, tr, lens, dropout_seed):
        states = self.rebuild_states(ro, tr, lens, dropout_seed)
        act = tr["act"].numpy()
        closed: List[tuple] = []
        n_st = 0
        for t, ids, rew, done, info in self._transitions(tr, lens):
            tid = torch.as_tensor(ids)
            row = Batch(obs=states[t, tid], act=act[t, ids], rew=rew, done=done, obs_next=states[t + 1, tid], info=info, policy=Batch())
            _, ep_return, ep_length, ep_first = self.buffer.add(row, buffer_ids=ids)
            n_st += len(ids)
            over = np.flatnonzero(done)
            if len(over):
                closed.append((ep_return[over], ep_length[over], ep_first[over]))
        return self._stats(closed, n_st)

    def _fill_device(self, ro, tr, lens, keys):
        """The device learner's buffer: HostCollector's row order and bookkeeping in one vectorised step (no state rebuild, no per-step
        add); rows are built from the trajectory on first access and the learner reads the device trajectory itself."""
        from core.vtb_learner import VtbDeviceRows
        self.buffer.fill_from_trajectory(VtbDeviceRows(self, ro, lens, keys, tr), lens)
        return self._summary_only(tr, lens)

    def _summary_only(self, tr, lens):
        """The result dict without buffer rows: every episode starts at its sub-buffer's first row of a fresh buffer."""
        ep_rew = np.zeros(self.env_num, np.float64)
        closed: List[tuple] = []
        n_st = 0
        offsets = np.asarray(self.buffer._offset)
        for t, ids, rew, done, _ in self._transitions(tr, lens):
            ep_rew[ids] += np.asarray(rew, np.float64)
            n_st += len(ids)
            fin = ids[done]
            if len(fin):
                closed.append((ep_rew[fin].copy(), np.full(len(fin), t + 1), offsets[fin]))
        return self._stats(closed, n_st)

    @staticmethod
    def _stats(closed, n_st) -> Dict[str, Any]:
        returns, lengths, firsts = (np.concatenate(col) for col in zip(*closed))
        stats = {"rews": returns, "lens": lengths, "idxs": firsts, "n/st": n_st, "n/ep": len(returns)}
        for name, arr in (("rew", returns), ("len", lengths)):
            stats[name], stats[name + "_std"] = arr.mean(), arr.std()
        return stats
