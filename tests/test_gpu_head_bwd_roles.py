"""GPU: the two-role form of head_bwd_fused_kernel (the hand-over instantiations: role A forms dZ and d h2 for item tile t while role B forms the
dWa product of tile t - 1 and sums tile t - 2) against the untouched one-role recompute kernel (CIRS_PPO_HEAD_RECOMPUTE=1).  Both forms run the same
operation sequence per output, so every comparison is torch.equal: no tolerance applies.

The shapes are the smallest at which a two-stage pipeline can go wrong.  The backward kernel never walks fewer than 4 item tiles per chunk, so the
catalogue size decides the LAST chunk's length:
    20 items   one partial tile, one chunk: fill and drain only, the partial tile is first and last
    100        4 tiles, the last partial: the smallest steady state
    160        4 + 1: a one-tile last chunk (drain only)
    180        4 + 2, the last partial: a two-tile chunk ending in the partial tile
    224        4 + 3: an odd tile count (buffer parity)
Each case runs minibatches of 32 rows (one live wave pair, three idle pairs), 70 and 200 rows (row tiles partly padding; 200: a second row block
whose last pair is idle), every byte of the workspace set to 0xff before each call.  The five cases cover the four instantiations (entropy term in
dZ or not, merge in the prologue or as a launch of its own).  The actions are chosen, not drawn: every third step takes the catalogue's last item
(the last, possibly partial tile), every third the first item of the last chunk (the first tile of a chunk), the others item 0 or a random one."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_learn import _random_case, make_learner, rollout_time_value_logp, upload_traj

pytestmark = pytest.mark.gpu

ROWS = (32, 70, 200)
TILE, TILES_PER_CHUNK = 32, 4


def _case(I):
    B, T = 24, 30
    pp, lens, acts, rews, dones, obs, n, rng = _random_case(I, B, T, seed=1000 + I)
    assert n >= sum(ROWS)
    n_tiles = -(-I // TILE)
    last_chunk_first_item = ((n_tiles - 1) // TILES_PER_CHUNK) * TILES_PER_CHUNK * TILE
    acts = acts.copy()
    acts[:, 0::3] = I - 1
    acts[:, 1::3] = last_chunk_first_item
    acts[:, 2::6] = 0
    value, logp = rollout_time_value_logp(pp, obs, acts, lens)
    rows = rng.permutation(n).astype(np.int32)
    return B, T, pp, lens, acts, rews, dones, obs, n, value, logp, rows


def _run(monkeypatch, recompute, case, I, ent_coef):
    from cirs_hip import abi
    from cirs_hip.rollout import Trajectory
    B, T, pp, lens, acts, rews, dones, obs, n, value, logp, rows = case
    monkeypatch.setenv("CIRS_PPO_HEAD_RECOMPUTE", "1" if recompute else "0")      # (read per call)
    traj = Trajectory(B, T, 20, "cuda")
    upload_traj(traj, acts, rews, dones, lens, obs, value, logp)
    ln, _ = make_learner(pp, I, B, T, [0.95, 0.95, 0.2, 0.25, ent_coef, 0.5, 1e-3, max(ROWS), 1])
    assert ln.prepare(traj, lens) == n
    # the chosen actions reach the kernel: rows of the last tile and of the last chunk's first tile are in every minibatch
    ln.dobs.zero_()
    losses = torch.zeros((len(ROWS), 4), dtype=torch.float32, device="cuda")
    s0 = 0
    for k, mb in enumerate(ROWS):
        idx = torch.as_tensor(rows[s0:s0 + mb]).cuda()
        s0 += mb
        ws = ln.workspace(max(ROWS))
        ws.fill_(255)      # fp32: NaN, int32: -1 -- whatever a kernel reads without anybody having written it in this step shows as a non-finite result
        abi.check(ln._lib.cirs_ppo_minibatch(C.byref(ln.cfg), ln.params.data_ptr(), ln.grads.data_ptr(), ln.adam_m.data_ptr(), ln.adam_v.data_ptr(),
                                             ln.opt_step, C.byref(ln.batch), idx.data_ptr(), mb, ln.dobs.data_ptr(), ln.n_env,
                                             losses[k].data_ptr(), ws.data_ptr(), ws.numel(), ln._stream()), "cirs_ppo_minibatch")
        ln.opt_step += 1
    torch.cuda.synchronize()
    return losses.clone(), ln.params.clone(), ln.adam_m.clone(), ln.adam_v.clone(), ln.dobs.clone()


# I, ent_coef, CIRS_PPO_MERGE_KERNEL: every item count, and all four (kEnt, kMerge) instantiations of the hand-over form
@pytest.mark.parametrize("I,ent_coef,merge_kernel", [(20, 0.0, "0"), (100, 0.01, "0"), (160, 0.0, "1"), (180, 0.01, "1"), (224, 0.0, "0"),
                                                     (180, 0.0, "0"), (20, 0.01, "1")])
def test_two_role_backward_gives_the_bits_of_the_recompute_kernel(I, ent_coef, merge_kernel, monkeypatch):
    monkeypatch.setenv("CIRS_PPO_MERGE_KERNEL", merge_kernel)
    case = _case(I)
    acts, lens = case[4], case[3]
    taken = np.concatenate([acts[b, :lens[b]] for b in range(len(lens))])
    assert (taken == I - 1).any() and (taken == ((-(-I // TILE) - 1) // TILES_PER_CHUNK) * TILES_PER_CHUNK * TILE).any()
    a, b = (_run(monkeypatch, recompute, case, I, ent_coef) for recompute in (False, True))
    for name, x, y in zip(("losses", "params", "adam_m", "adam_v", "dobs"), a, b):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} of {x.numel()} elements differ, max |d| = {float((x - y).abs().max()):.3e}"
        assert bool(torch.isfinite(x).all()), name
