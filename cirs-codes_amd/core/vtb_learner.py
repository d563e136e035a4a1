"""DeviceVtbPPOPolicy: `PPOPolicy(actor, critic, optim, dist, ..., learner="device")` over a continuous ActorProb (CIRS-RL-taobao.py).

A HostPPOPolicy whose update runs on the GPU (cirs_hip/vtb_learn.py, csrc/vtb_learn.hip) over the buffer of a device collect
(Collector(..., rollout="device")): same report dict, same numpy draws (sample_index, one permutation per pass), the host modules,
optimisers and ret_rms written back in place afterwards.  Acting, map_action and process_fn's protocol are HostPPOPolicy's.
One difference from the host learner: torch's generator is not consumed by the update (HostPPOPolicy draws a throwaway sample per
distribution it builds)."""
from typing import Dict, List

import numpy as np
import torch

from core.host_rl import HostPPOPolicy


class VtbDeviceRows:
    """What a device collect leaves in its replay buffer instead of per-step rows: the rollout whose trajectory holds the collect, the
    episode lengths and the collect's keys (seed, collect_id, dropout_seed).  Host rows (HostCollector's layout; obs / obs_next are
    detached copies of the rollout's states) are built on first access."""

    def __init__(self, collector, rollout, lens, keys, host_traj):
        self.collector, self.rollout, self.lens = collector, rollout, np.asarray(lens, dtype=np.int64)
        self.seed, self.collect_id, self.dropout_seed = keys
        self.dropout_p, self.drop_env_base = float(rollout.dropout_p), int(rollout.cfg.model.drop_env_base)     # with dropout_seed: the dropout key
        self.dropout_redraw = bool(rollout.dropout_redraw)      # the learner follows the collect's dropout procedure
        self._host = host_traj

    def is_current(self):
        """True while the rollout's trajectory still holds this collect (the next collect of the same collector overwrites it)."""
        return self.collector.last_collect == (self.seed, self.collect_id, self.dropout_seed) and self.rollout is self.collector._rollout

    def materialise(self, buffer):
        from tianshou.data import Batch
        tr, n = self._host, buffer.maxsize
        e, t, idx = buffer._rows_env, buffer._rows_t, buffer._index
        states = tr["state"]
        S, A = states.shape[-1], tr["act"].shape[-1]
        obs = torch.zeros((n, S), dtype=torch.float32)
        obs_next = torch.zeros((n, S), dtype=torch.float32)
        it, et, tt = (torch.as_tensor(x) for x in (idx, e, t))
        obs[it] = states[tt, et]
        obs_next[it] = states[tt + 1, et]
        act = np.zeros((n, A), dtype=np.float32)
        rew, done, ctr, env_id = np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n), np.zeros(n, dtype=np.int64)
        act[idx] = tr["act"].numpy()[t, e]
        rew[idx] = tr["rew"].numpy()[t, e]
        if not self.rollout.vtb.simulated:
            rew[idx] = rew[idx].astype(np.int64)
        done[idx] = tr["done"].numpy()[t, e].astype(bool)
        ctr[idx] = tr["ctr"].numpy()[t, e]
        env_id[idx] = e
        return Batch(obs=obs, act=act, rew=rew, done=done, obs_next=obs_next, info=Batch(CTR=ctr, env_id=env_id), policy=Batch())


class DeviceVtbPPOPolicy(HostPPOPolicy):
    def __init__(self, actor, critic, optim, dist_fn, *args, **kwargs):
        super().__init__(actor, critic, optim, dist_fn, *args, **kwargs)
        from cirs_hip.vtb_learn import check_optimisers, policy_params
        self._learner = None
        check_optimisers(optim, policy_params(actor, critic), self._tracker_params_or_none())

    def _tracker_params_or_none(self):
        """The tracker is not known to the policy before a Collector binds it: the second optimiser's own list stands in."""
        return list(self.optim[1].param_groups[0]["params"]) if isinstance(self.optim, (list, tuple)) and len(self.optim) == 2 else []

    def _get_learner(self, src):
        from cirs_hip.vtb_learn import DeviceVtbLearner
        ro = src.rollout
        key = (id(ro.tracker), ro.vtb.n_env, ro.vtb.max_turn)
        if self._learner is None or self._learner_key != key:
            self._learner = DeviceVtbLearner(ro.tracker, self.actor, self.critic, ro.vtb.n_env, ro.vtb.max_turn, ro.device)
            self._learner_key = key
        return self._learner

    def update(self, sample_size, buffer, batch_size=None, repeat=1, **kwargs) -> Dict[str, List[float]]:
        if buffer is None:
            return dict()
        src = getattr(buffer, "_traj", None)
        if not isinstance(src, VtbDeviceRows):
            raise ValueError("learner='device' updates from the buffer of a device collect: build the training Collector with "
                             "rollout='device' over DummyVectorEnv(..., device='cuda')")
        if not src.is_current():
            raise ValueError("this buffer's device trajectory was overwritten by a later collect of its Collector")
        rows = buffer.sample_index(sample_size)
        n = len(rows)
        bs = n if batch_size is None else int(batch_size)
        self.updating = True
        try:
            ln = self._get_learner(src)
            ln.prepare(self, src, rows, buffer)
            perms = [np.random.permutation(n) for _ in range(int(repeat))]
            report = ln.learn(self, perms, bs, int(repeat))
        finally:
            self.updating = False
        if self.lr_scheduler:
            self.lr_scheduler.step()
        return report
