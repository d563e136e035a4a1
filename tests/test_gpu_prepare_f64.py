"""GPU: the PPO process_fn stage (csrc/ppo.hip: gae_kernel, offsets_kernel, compact_obs_kernel, returns_kernel, prepare_tail_kernel) through the five
entry forms of DeviceLearner against the float64 / long double restatement of tests/preparecase.py, at the shapes where the kernels' loops change
course: every residue of gae_kernel's 8-step pass and its look-ahead, the 64-env workgroup, one and several envs per thread of the offsets scan,
one row per thread and the 8 x 1024 pass of the return reduction (each -1 / +1), N = 1.  Every batch array is allocated for B * T rows and filled
with a sentinel first: rows < n are checked exactly (copies, indices, offsets, count) or per element at 2^-24 |w| + 2^-40 M (advantages, returns),
rows >= n must still hold the sentinel, the running mean / variance sit within 1e-12 of long double, and the forms leave identical bits.
Margins as measured: profiles/prepare_f64_margins.md."""
import numpy as np
import pytest
import torch

import preparecase as pc

pytestmark = pytest.mark.gpu

# (a) prepare, (b) prepare with the lengths on the device, (c) prepare_async, (d) prepare_async with 1 / 8 permutations drawn in its last launch,
# (e) readback_lens first: prepare_async then finds the offsets formed
FORMS = ("sync", "sync_lens_dev", "async", "async_perms1", "async_perms8", "readback_async")
SENTINEL = dict(b_obs=np.nan, b_act=-7, b_adv=np.nan, b_ret=np.nan, b_vs=np.nan, b_logp=np.nan, b_env=-7, b_t=-7)
PERM_SEED, PERM_TAG = 4242, 17


def _learner(B, T, rew_norm):
    from cirs_hip.learner import DeviceLearner, flat_policy_params
    flat, _ = flat_policy_params(pc.N_ITEMS)
    return DeviceLearner(flat, pc.N_ITEMS, B, T, gamma=0.99, gae_lambda=0.95, rew_norm=rew_norm)


def _regeometry(ln, B, T):
    """the carried sequences run cases of different B x T on ONE learner (its rms_state is what is carried): new extents, scratch re-made"""
    ln.n_env, ln.max_turn = B, T
    ln._prep_scratch = None


_TRAJ = {}


def _upload(c):
    """the case's trajectory on the device, uploaded once per case and never written by the stage"""
    from cirs_hip.rollout import Trajectory
    key = id(c)
    if key not in _TRAJ:
        _TRAJ.clear()                      # one case at a time (the parametrisation runs the forms of a case back to back)
        traj = Trajectory(c["B"], c["T"], pc.S, "cuda")
        for k in ("value", "logp", "rew", "act", "done", "obs"):
            getattr(traj, k).copy_(torch.as_tensor(c[k]))
        _TRAJ[key] = (traj, torch.as_tensor(c["lens"]).cuda())
    return _TRAJ[key]


def _run(ln, form, c):
    """one call of the stage through `form` on sentinel-filled B * T-row batch arrays -> every array as numpy (all rows), rms, offsets, n, permutations"""
    B, T, lens = c["B"], c["T"], c["lens"]
    traj, lens_dev = _upload(c)
    ln._alloc_batch(B * T)
    for name, v in SENTINEL.items():
        getattr(ln, name).fill_(v)
    k = {"async_perms1": 1, "async_perms8": 8}.get(form, 0)
    if k:
        ln._perm_buf = torch.full((8 * B * T,), -7, dtype=torch.int32, device="cuda")
        ln.perm_seed, ln.perm_tag = PERM_SEED, PERM_TAG
        perm_ptr = ln._perm_buf.data_ptr()
    if form == "sync":
        n = ln.prepare(traj, lens)
    elif form == "sync_lens_dev":
        n = ln.prepare(traj, lens, lens_dev=lens_dev)
    else:
        if form == "readback_async":
            pinned = torch.zeros(B, dtype=torch.int32).pin_memory()
            ln.readback_lens(lens_dev, pinned)
        ln.prepare_async(traj, lens_dev, perm_repeat=k)
        n = ln.finish_prepare(lens)
    torch.cuda.synchronize()
    got = {name: getattr(ln, name).cpu().numpy() for name in pc.BATCH}
    assert all(len(got[name]) >= B * T for name in pc.BATCH)       # (more where an earlier call of a carried sequence was larger)
    got.update(n=n, rms=ln.rms_state.cpu().numpy(), offsets=ln.offsets_dev.cpu().numpy())
    if form not in ("sync", "sync_lens_dev"):
        assert int(ln._n_dev.cpu()) == n, f"{form}: the device's row count"
    if form == "readback_async":
        np.testing.assert_array_equal(pinned.numpy(), lens)
    if k:       # the permutations of the last launch: cirs_random_permutations' of the same key, row stride n, nothing beyond k * n
        from cirs_hip import abi
        want = torch.empty((k, n), dtype=torch.int32, device="cuda")
        abi.check(abi.lib().cirs_random_permutations(n, PERM_SEED, PERM_TAG, k, want.data_ptr(), torch.cuda.current_stream().cuda_stream), "perms")
        perms = ln._perms_on_device(n, k, None)
        assert ln._perm_buf.data_ptr() == perm_ptr == perms.data_ptr() and ln.perm_tag == PERM_TAG + k, form
        assert torch.equal(perms, want), f"{form}: permutations"
        assert np.array_equal(np.sort(perms.cpu().numpy(), axis=1), np.tile(np.arange(n, dtype=np.int32), (k, 1))), form
        assert bool((ln._perm_buf[k * n:] == -7).all()), f"{form}: _perm_buf written beyond k * n"
    return got


def _same_bits(a, b, n, what):
    for name in pc.BATCH:
        np.testing.assert_array_equal(pc.bits(a[name][:n]), pc.bits(b[name][:n]), err_msg=f"{what}: {name}")
    np.testing.assert_array_equal(pc.bits(a["rms"]), pc.bits(b["rms"]), err_msg=f"{what}: rms_state")
    np.testing.assert_array_equal(a["offsets"], b["offsets"], err_msg=what)


def _line(case_id, form, used):
    print(f"prepare {case_id} {form}: adv used/bar {used[0]:.3g}  ret used/bar {used[1]:.3g}  rms mean {used[2]:.3g} var {used[3]:.3g}  != float32(w): {used[4]}")


@pytest.mark.parametrize("case_id", pc.IDS)
def test_prepare_against_float64(case_id):
    c, w64, wld = pc.reference(case_id)
    rew_norm = pc.CASES[case_id][1]
    first = None
    for form in FORMS:
        got = _run(_learner(c["B"], c["T"], rew_norm), form, c)
        used = pc.check_outputs(got, c, w64, wld, pc.RMS0, rew_norm, SENTINEL, f"{case_id} {form}")
        _line(case_id, form, used)
        if first is None:
            first = got
        else:           # "same kernels: same bits"
            _same_bits(first, got, w64["n"], f"{case_id}: {form} vs {FORMS[0]}")


@pytest.mark.parametrize("seq_id", list(pc.SEQUENCES))
def test_carried_running_variance_against_float64(seq_id):
    """consecutive calls on one learner, the restatement carrying its own running mean / variance alongside (float64 and long double each their own)"""
    calls = pc.sequence_reference(seq_id)
    per_form = []
    for form in FORMS:
        ln, outs = None, []
        for i, (c, w64, wld) in enumerate(calls):
            if ln is None:
                ln = _learner(c["B"], c["T"], True)
            else:
                _regeometry(ln, c["B"], c["T"])
            before = ln.rms_state.cpu().numpy()
            got = _run(ln, form, c)
            used = pc.check_outputs(got, c, w64, wld, before, True, SENTINEL, f"{seq_id}[{i}] {form}")
            _line(f"{seq_id}[{i}]={pc.SEQUENCES[seq_id][i]}", form, used)
            outs.append(got)
        per_form.append(outs)
    for form, outs in zip(FORMS[1:], per_form[1:]):
        for i, (a, b) in enumerate(zip(per_form[0], outs)):
            _same_bits(a, b, calls[i][1]["n"], f"{seq_id}[{i}]: {form} vs {FORMS[0]}")


def test_a_second_run_gives_identical_bits():
    c, w64, _ = pc.reference("rows-8193")
    for form in FORMS:
        a, b = (_run(_learner(c["B"], c["T"], True), form, c) for _ in range(2))
        _same_bits(a, b, w64["n"], f"rows-8193 {form}: second run")
