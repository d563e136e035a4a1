"""GPU: the actor-head logits handed from head_stats_kernel to head_bwd_fused_kernel through the minibatch workspace (the default) against the
backward kernel forming them a second time (CIRS_PPO_HEAD_RECOMPUTE=1).  Both forms consume the same accumulator bits -- the same MFMA sequence on
the same fp16 planes, summed acc + (acc1 + acc2) -- so every comparison here is torch.equal: no tolerance applies."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from test_gpu_learn import _random_case, make_learner, rollout_time_value_logp, upload_traj

pytestmark = pytest.mark.gpu


def _nan_fill(ln, mb):
    """Every byte of the minibatch workspace 0xff (fp32: NaN, int32: -1): a slab tile, row or flag that a kernel reads without anybody having
    written it in this step then shows as a non-finite result instead of passing on the zeros of a fresh allocation."""
    ln.workspace(mb).fill_(255)


def _run_learn(monkeypatch, recompute, case, I, B, T, bs, rep, ent_coef, perms):
    from cirs_hip.learner import minibatch_slices
    from cirs_hip.rollout import Trajectory
    pp, lens, acts, rews, dones, obs, n, _ = case
    monkeypatch.setenv("CIRS_PPO_HEAD_RECOMPUTE", "1" if recompute else "0")      # (read per call)
    value, logp = rollout_time_value_logp(pp, obs, acts, lens)
    traj = Trajectory(B, T, 20, "cuda")
    upload_traj(traj, acts, rews, dones, lens, obs, value, logp)
    ln, _ = make_learner(pp, I, B, T, [0.95, 0.95, 0.2, 0.25, ent_coef, 0.5, 1e-3, bs, rep])
    assert ln.prepare(traj, lens) == n
    _nan_fill(ln, max(e - s for s, e in minibatch_slices(n, bs)))
    losses = ln.learn(bs, rep, perms=perms)
    torch.cuda.synchronize()
    ln.check_handoffs()
    return losses.clone(), ln.params.clone(), ln.adam_m.clone(), ln.adam_v.clone(), ln.dobs.clone()


def _assert_same_bits(a, b):
    for name, x, y in zip(("losses", "params", "adam_m", "adam_v", "dobs"), a, b):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} of {x.numel()} elements differ, max |d| = {float((x - y).abs().max()):.3e}"
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())


# I, B, T, batch, repeat, ent_coef, CIRS_PPO_MERGE_KERNEL
#   500 items, 24 x 10: one row tile per minibatch, last item tile partial (500 = 15 x 32 + 20), several minibatches, a merged last one of another size
#   10728 items, 100 x 30, batch 512: four row blocks -> head_stats_kernel walks 4 item tiles per chunk and head_bwd_fused_kernel 6: a slab index that
#       depended on either chunking would pair the wrong tiles
#   ent_coef = 0.01: the kEnt instantiations;  CIRS_PPO_MERGE_KERNEL=1: the kMerge = false instantiations (what the item-sharded learner launches)
@pytest.mark.parametrize("I,B,T,bs,rep,ent_coef,merge_kernel", [(500, 24, 10, 32, 2, 0.0, "0"), (10728, 100, 30, 512, 2, 0.0, "0"),
                                                              (3327, 24, 10, 64, 2, 0.01, "0"), (500, 24, 10, 32, 2, 0.0, "1"),
                                                              (3327, 24, 10, 64, 1, 0.01, "1")])
def test_handed_over_logits_give_the_bits_of_the_recompute(I, B, T, bs, rep, ent_coef, merge_kernel, monkeypatch):
    monkeypatch.setenv("CIRS_PPO_MERGE_KERNEL", merge_kernel)
    case = _random_case(I, B, T, seed=I + bs)
    perms = [case[7].permutation(case[6]) for _ in range(rep)]
    outs = [_run_learn(monkeypatch, recompute, case, I, B, T, bs, rep, ent_coef, perms) for recompute in (False, True)]
    _assert_same_bits(outs[0], outs[1])


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_row_counts_off_the_tile_sizes_read_nothing_unwritten(ent_coef, monkeypatch):
    """Minibatches of 70 and 200 rows (neither a multiple of the 32-row tile nor of the 128-row block: the last row tile is partly padding and the
    last row block has an idle wave), one cirs_ppo_minibatch call each, every byte of the workspace set before each call.  What this reaches: the
    padding ROWS inside the last row tile (rows mb .. n_pad - 1, whose slab values must be finite because lse = 1e30 does not neutralise a NaN) and
    slab tiles left over from nothing (a wrong index would read 0xff bytes).  What it cannot reach: a whole row tile at or beyond mb -- every caller
    passes n_pad = n_pad_of(mb), so no such tile exists below n_pad; the statistics kernel's "every row tile below n_pad" is a guard for a caller
    that pads further.  Bit identity with the recompute, and finite losses / parameters."""
    from cirs_hip import abi
    from cirs_hip.rollout import Trajectory
    I, B, T = 3327, 24, 30
    case = _random_case(I, B, T, seed=77)
    pp, lens, acts, rews, dones, obs, n, rng = case
    assert n >= 270
    rows = rng.permutation(n).astype(np.int32)
    value, logp = rollout_time_value_logp(pp, obs, acts, lens)
    outs = []
    for recompute in (False, True):
        monkeypatch.setenv("CIRS_PPO_HEAD_RECOMPUTE", "1" if recompute else "0")
        traj = Trajectory(B, T, 20, "cuda")
        upload_traj(traj, acts, rews, dones, lens, obs, value, logp)
        ln, _ = make_learner(pp, I, B, T, [0.95, 0.95, 0.2, 0.25, ent_coef, 0.5, 1e-3, 200, 1])
        assert ln.prepare(traj, lens) == n
        ln.dobs.zero_()
        losses = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
        for k, (s0, e0) in enumerate(((0, 70), (70, 270))):
            idx = torch.as_tensor(rows[s0:e0]).cuda()
            ws = ln.workspace(200)
            _nan_fill(ln, 200)
            abi.check(ln._lib.cirs_ppo_minibatch(C.byref(ln.cfg), ln.params.data_ptr(), ln.grads.data_ptr(), ln.adam_m.data_ptr(), ln.adam_v.data_ptr(),
                                                 ln.opt_step, C.byref(ln.batch), idx.data_ptr(), e0 - s0, ln.dobs.data_ptr(), ln.n_env,
                                                 losses[k].data_ptr(), ws.data_ptr(), ws.numel(), ln._stream()), "cirs_ppo_minibatch")
            ln.opt_step += 1
        torch.cuda.synchronize()
        outs.append((losses.clone(), ln.params.clone(), ln.adam_m.clone(), ln.adam_v.clone(), ln.dobs.clone()))
    _assert_same_bits(outs[0], outs[1])


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_item_sharded_entry_point_hands_over_the_same_bits(ent_coef, monkeypatch):
    """cirs_ppo_minibatch_tp (DeviceLearner.learn_tp, two item shards as threads on one device: the statistics kernel runs in phase 1 and the
    backward in phase 2 of a step, both on the rank's workspace): hand-over against recompute, bit for bit on every rank -- losses, all parameters
    incl. the rank's shard of the head, both Adam moments, d obs.  500 items per shard: the shard's last item tile is partial."""
    import torch.distributed as dist
    from cirs_hip.distributed import Collectives
    from cirs_hip.learner import DeviceLearner, flat_policy_params, minibatch_slices
    from cirs_hip.rollout import Trajectory
    from test_gpu_engine_dp import FakeCollectives
    from test_gpu_learn import POL
    W, Is, B, T, bs = 2, 500, 40, 12, 100
    I = W * Is
    pp, lens, acts, rews, dones, obs, n, rng = _random_case(I, B, T, seed=91)
    value, logp = rollout_time_value_logp(pp, obs, acts, lens)
    perms = [rng.permutation(n) for _ in range(2)]
    traj = Trajectory(B, T, 20, "cuda")
    upload_traj(traj, acts, rews, dones, lens, obs, value, logp)
    max_mb = max(e - s for s, e in minibatch_slices(n, bs))

    def run_all(recompute):
        monkeypatch.setenv("CIRS_PPO_HEAD_RECOMPUTE", "1" if recompute else "0")
        fake = FakeCollectives(W)
        monkeypatch.setattr(dist, "all_reduce", fake.all_reduce)
        monkeypatch.setattr(dist, "all_gather_into_tensor", fake.all_gather_into_tensor)
        monkeypatch.setattr(dist, "get_backend", lambda group=None: "nccl")
        ranks, results = [], [None] * W
        for r in range(W):
            shard = dict(pp)
            shard["wa"], shard["ba"] = pp["wa"][r * Is:(r + 1) * Is].contiguous(), pp["ba"][r * Is:(r + 1) * Is].contiguous()
            flat, _ = flat_policy_params(Is, init={POL[k]: v for k, v in shard.items()})
            ranks.append(DeviceLearner(flat, Is, B, T, gamma=0.95, gae_lambda=0.95, eps_clip=0.2, vf_coef=0.25, ent_coef=ent_coef, max_grad_norm=0.5,
                                       lr=1e-3, norm_adv=True, value_clip=True, rew_norm=True))

        def run(r):
            try:
                fake.local.rank = r
                ranks[r].prepare(traj, lens)
                _nan_fill(ranks[r], max_mb)
                results[r] = ranks[r].learn_tp(bs, 2, perms, r, W, r * Is, Collectives())
            except Exception as exc:  # noqa: BLE001
                fake.errors.append(exc)
                fake.bar.abort()

        threads = [threading.Thread(target=run, args=(r,)) for r in range(W)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not fake.errors, fake.errors
        torch.cuda.synchronize()
        return [(results[r].clone(), ranks[r].params.clone(), ranks[r].adam_m.clone(), ranks[r].adam_v.clone(), ranks[r].dobs.clone()) for r in range(W)]

    a, b = run_all(False), run_all(True)
    for r in range(W):
        _assert_same_bits(a[r], b[r])
