"""GPU: a slot tracker (csrc/{gru,lstm,avg,caser,nextitnet,stamp}_tracker.hip) against its float64 restatement (cirs_hip/*_host.py): every state of
every live (env, position) through reset / init / step, what the LSTM carries, every gradient tensor of the backward against float64 autograd.

The checks are written once here, over a record of tests/slotcase.py (nextitnetcase.py and stampcase.py for those two);
tests/test_gpu_{gru,lstm,avg,caser,nextitnet,stamp}_tracker.py bind them to their tracker under the test names and ids those files have
always had.  (This file is named like a test module so that pytest rewrites its assertions; it collects no item of its own.)  The Caser cases' inputs are ones where float64 itself is unambiguous at every max and ReLU
(tests/test_caser_host_cpu.py checks that on the CPU): no case and no element is skipped or masked."""
import ctypes as C

import numpy as np
import torch

from slotcase import backward_args, errors32, reference, replay, replayed


def states_match_float64_restatement(slot, ci, mode):
    (U, I, B, T, S, hot), model = slot.split(slot.CASES[ci])
    ref, bar_for, STATE_BAR = reference(slot, ci), slot.case.bar_for, slot.case.STATE_BAR
    trk, got = replayed(slot, ci, mode)
    live = ref["live"]
    assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
    np.testing.assert_array_equal(trk.len.cpu().numpy(), ref["lens"])
    err = np.abs(got[live] - ref["s64"][live]).max() / ref["s_scale"]
    bar = bar_for(STATE_BAR, ref["s_err32"])
    print(f"states {slot.name} {slot.IDS[ci]} {mode}: device {err:.3e}  float32 restatement {ref['s_err32']:.3e}  bar {bar:.3e}")
    assert err <= bar
    # what every (layer, env) carries after the replay (the LSTM's h and c; `model` is then its layer count): the restatement's tensors of
    # that env's last position
    assert set(ref["c64"]) == set(slot.carried)
    for name in slot.carried:
        have, want = getattr(trk, name).cpu().numpy().astype(np.float64), ref["c64"][name]
        assert have.shape == want.shape == (model, B, 32)
        err = np.abs(have - want).max() / np.abs(want).max()
        bar = bar_for(STATE_BAR, ref["c_err32"][name])
        print(f"carried {name} {slot.name} {slot.IDS[ci]} {mode}: device {err:.3e}  float32 restatement {ref['c_err32'][name]:.3e}  bar {bar:.3e}")
        assert err <= bar, name


def backward_matches_float64_autograd(slot, ci):
    (U, I, B, T, S, hot), model = slot.split(slot.CASES[ci])
    ref = reference(slot, ci)
    trk, _ = replayed(slot, ci)
    args = backward_args(ref, T, B, S)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    lens, acts = ref["lens"], ref["acts"]
    touched_items = np.unique(np.concatenate([acts[b, :lens[b] - 1] for b in range(B)]))
    touched_users = np.unique(ref["users"])
    assert set(trk.grad_views) == set(ref["g64"]) == set(slot.param_shapes(U, I, S, model))
    assert len(trk.grad_views) == slot.n_grad_tensors(model)
    for k, gv in trk.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), ref["g64"][k]
        scale = np.abs(want).max() + 1e-300
        err = np.abs(got - want).max() / scale
        bar = slot.case.bar_for(slot.case.GRAD_BAR, ref["g_err32"][k])
        print(f"grad {slot.name} {slot.IDS[ci]} {k}: device {err:.3e}  float32 restatement {ref['g_err32'][k]:.3e}  bar {bar:.3e}")
        assert err <= bar, k
    gi = trk.grad_views["embedding_dict.feat_item.weight"].cpu().numpy()
    gu = trk.grad_views["embedding_dict.feat_user.weight"].cpu().numpy()
    assert (np.delete(gi, touched_items, axis=0) == 0).all() and (np.delete(gu, touched_users, axis=0) == 0).all()
    # a second call: the same bits (fixed reduction orders, no atomics)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args)
    assert torch.equal(trk.flat_grad, first)


def backward_refuses_a_short_workspace(slot):
    from cirs_hip import abi
    ci = slot.short_ws_case
    (U, I, B, T, S, hot), model = slot.split(slot.CASES[ci])
    trk, _ = replayed(slot, ci)
    users, traj, row_env, row_t, offsets, lens, n_rows, G = backward_args(reference(slot, ci), T, B, S)
    users = users.to("cuda", torch.int32)
    lib = abi.lib()
    need = getattr(lib, slot.entry + "_backward_workspace_bytes")(C.byref(trk.cfg), n_rows)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    backward = getattr(lib, slot.entry + "_backward")

    def call(nbytes, stream):
        rc = backward(C.byref(trk.cfg), C.byref(trk.w), C.byref(trk.st), users.data_ptr(), traj.act.data_ptr(), traj.rew.data_ptr(),
                      row_env.data_ptr(), row_t.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n_rows, G.data_ptr(), C.byref(trk.g),
                      ws.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        return rc
    trk.flat_grad.fill_(float("nan"))
    assert call(need - 1, None) == -1 and b"workspace too small" in lib.cirs_last_error()
    assert torch.isnan(trk.flat_grad).all(), "a refused call launched something"
    assert call(need, torch.cuda.current_stream().cuda_stream) == 0 and not torch.isnan(trk.flat_grad).any()


def states_when_a_launch_walks_several_env_groups(slot, walk):
    """More envs than one pass of the launch covers on a 256-CU part (slotcase says how many that is per tracker): every wavefront (GRU, LSTM)
    or workgroup (Avg, Caser) then walks a second group of envs, the last one a ragged tail.  Same bar as above."""
    U, I, S = 50, 80, 20
    B, T, model, seed = walk
    p = slot.param_dict(U, I, seed, S, model)
    users, acts, rews, lens, _ = slot.case.teacher_inputs(U, I, B, T)
    s64, live, scale, err32, _, _ = errors32(slot, p, users, acts, rews, lens, model, T)
    trk, _ = slot.device_trainable(p, U, I, B, T, model, S)
    for mode in ("env_ids", "skip"):
        got = replay(trk, users, acts, rews, lens, mode)
        assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
        np.testing.assert_array_equal(trk.len.cpu().numpy(), lens)
        err = np.abs(got[live] - s64[live]).max() / scale
        bar = slot.case.bar_for(slot.case.STATE_BAR, err32)
        print(f"states {slot.name} B={B} {mode}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar
