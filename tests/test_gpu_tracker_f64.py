"""GPU: the Transformer state tracker (csrc/tracker.hip, csrc/tracker_bwd.hip) against the float64 run of its restatement (oracle/nn_oracle.py on
float64 parameters), at the shapes where its dispatch changes (tests/trackercase.py): every state of every live (env, position) through reset / init /
step, every gradient tensor of backward(), backward(last_rows_only=True) and prefix_states.  One bar everywhere, relative to the largest live state or
to max|want| of the tensor:  err(device, float64) <= max(4 x err(float32 restatement, float64), 3e-6)."""
import numpy as np
import pytest
import torch

import trackercase as tc
from test_gpu_tracker_bwd import rows_of

pytestmark = pytest.mark.gpu


def _path(monkeypatch, path):
    if path == "rows":
        monkeypatch.setenv("CIRS_TRACKER_ATTN_ROWS", "1")
    else:
        monkeypatch.delenv("CIRS_TRACKER_ATTN_ROWS", raising=False)


def check_states(what, got, ref):
    live = ref["live"]
    assert not np.isnan(got[live]).any() and np.isnan(got[~live]).all()
    err = float(np.abs(got[live] - ref["s64"][live]).max() / ref["s_scale"])
    bar = tc.bar_for(ref["s_e32"])
    print(f"states {what}: device {err:.3e}  float32 restatement {ref['s_e32']:.3e}  bar {bar:.3e}  share {err / bar:.2f}")
    assert err <= bar, what


def check_grads(what, trk, g64, e32):
    worst = []
    for k, gv in trk.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), g64[k]
        scale = np.abs(want).max()
        if scale == 0:      # no live row contributes (the gate and the item table when no action is read): nothing may be written but zeros
            print(f"grad {what} {k}: want is all zero")
            assert (got == 0).all(), k
            continue
        err, bar = float(np.abs(got - want).max() / scale), tc.bar_for(e32[k])
        print(f"grad {what} {k}: device {err:.3e}  float32 restatement {e32[k]:.3e}  bar {bar:.3e}  share {err / bar:.2f}")
        worst.append((err / bar, k))
    print(f"grad {what}: largest share {max(worst)[0]:.2f} ({max(worst)[1]})")
    assert max(worst)[0] <= 1.0, [w for w in worst if w[0] > 1.0]


def check_untouched_rows(trk, ref):
    users, items = tc.touched(ref)
    gu = trk.grad_views["embedding_dict.feat_user.weight"].cpu().numpy()
    gi = trk.grad_views["embedding_dict.feat_item.weight"].cpu().numpy()
    assert (np.delete(gu, users, axis=0) == 0).all() and (np.delete(gi, items, axis=0) == 0).all()


@pytest.mark.parametrize("name", list(tc.CASES))
def test_states_match_float64(name):
    ref = tc.reference(name)
    c = ref["case"]
    trk = tc.device_tracker(c, ref["p"])
    got = tc.replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids", pad=c["pad"])
    np.testing.assert_array_equal(trk.len.cpu().numpy(), ref["lens"])
    check_states(name, got, ref)


@pytest.mark.parametrize("mode", ["env_ids", "skip"])
@pytest.mark.parametrize("name", tc.MODE_CASES)
def test_states_with_finished_envs_in_the_batch(name, mode):
    """env_ids in descending order; skip on even steps and item -1 on odd ones: a finished env's wavefront returns early inside its workgroup, its
    row of the state buffer keeps the NaN it held."""
    ref = tc.reference(name)
    c = ref["case"]
    trk = tc.device_tracker(c, ref["p"])
    got = tc.replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], mode, pad=3)
    np.testing.assert_array_equal(trk.len.cpu().numpy(), ref["lens"])
    check_states(f"{name} {mode}", got, ref)


@pytest.mark.parametrize("mult,extra,packing", [(1, 1, (2, 1)), (2, 1, (4, 1)), (2, 3, (4, 3))], ids=["CUs+1", "2CUs+1", "2CUs+3"])
def test_states_at_every_wavefront_packing_of_the_step_launch(mult, extra, packing):
    """launch_tracker packs 1, 2 or 4 wavefronts per workgroup for n <= CUs, n <= 2 CUs and more.  n = CUs + 1: two per workgroup, the last one half
    empty; n = 2 CUs + 1 and 2 CUs + 3: four per workgroup with tails of 1 and 3.  init and the first step see all n envs; later steps drop finished
    envs (env_ids) or keep them in the batch, interleaved with live ones (skip / item -1)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = mult * cus + extra
    wpw = 1 if B <= cus else 2 if B <= 2 * cus else 4
    assert (wpw, B % wpw) == packing, "a CU count at which this env count leaves no ragged last workgroup"
    U, I, T = 50, 80, 3
    lens = np.random.RandomState(B).randint(2, T + 2, size=B)
    c = tc._case(U, I, T, lens, seed=5)
    p, users, acts, rews, G, g_last = tc.inputs(c)
    r64 = tc.restatement(c, p, users, acts, rews, G, g_last, torch.float64, want_grads=False)
    r32 = tc.restatement(c, p, users, acts, rews, G, g_last, torch.float32, want_grads=False)
    live = tc.live_mask(lens, T)
    scale = float(np.abs(r64["states"][live]).max())
    ref = dict(live=live, s64=r64["states"], s_scale=scale, s_e32=float(np.abs(r32["states"][live] - r64["states"][live]).max() / scale))
    assert (lens[::2] == 2).any() and (lens[1::2] == 2).any() and (lens == T + 1).any()
    trk = tc.device_tracker(c, p)
    for mode in ("env_ids", "skip"):
        got = tc.replay(trk, users, acts, rews, lens, mode)
        np.testing.assert_array_equal(trk.len.cpu().numpy(), lens)
        check_states(f"B={B} ({wpw} wavefronts per workgroup) {mode}", got, ref)


@pytest.mark.parametrize("name,path", tc.BACKWARD_RUNS, ids=[f"{k}-{p}" for k, p in tc.BACKWARD_RUNS])
def test_backward_matches_float64_autograd(name, path, monkeypatch):
    _path(monkeypatch, path)
    ref = tc.reference(name)
    c = ref["case"]
    trk = tc.device_tracker(c, ref["p"])
    tc.replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    args = tc.backward_args(ref)
    G = torch.as_tensor(ref["G"]).cuda()
    trk.flat_grad.fill_(float("nan"))      # the pass overwrites: nothing of what the buffer held may survive
    trk.backward(*args, G)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    check_grads(f"{name} {path}", trk, ref["g64"], ref["e32"])
    check_untouched_rows(trk, ref)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args, G)
    assert torch.equal(trk.flat_grad, first), "a second call gave other bits"


@pytest.mark.parametrize("name", tc.SPECIAL_CASES)
def test_last_row_backward_matches_float64_autograd(name):
    """backward(last_rows_only=True) against the float64 gradient of a G that is zero except on every env's last row -- directly, not through the
    general pass."""
    ref = tc.reference(name)
    c = ref["case"]
    trk = tc.device_tracker(c, ref["p"])
    tc.replay(trk, ref["users"], ref["acts"], ref["rews"], ref["lens"], "env_ids")
    args = tc.backward_args(ref)
    g_last = torch.as_tensor(ref["g_last"]).cuda()
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args, g_last, last_rows_only=True)
    first = trk.flat_grad.clone()
    assert not torch.isnan(first).any()
    check_grads(f"{name} last rows", trk, ref["g64_last"], ref["e32_last"])
    check_untouched_rows(trk, ref)
    trk.flat_grad.fill_(float("nan"))
    trk.backward(*args, g_last, last_rows_only=True)
    assert torch.equal(trk.flat_grad, first), "a second call gave other bits"


@pytest.mark.parametrize("name", tc.SPECIAL_CASES)
def test_prefix_states_match_float64(name):
    """prefix_states: the state of every env's last row, against float64; envs without rows keep what the buffer held."""
    ref = tc.reference(name)
    c = ref["case"]
    lens, S, B = ref["lens"], c["S"], len(ref["lens"])
    trk = tc.device_tracker(c, ref["p"])
    tc.replay(trk, ref["users"], ref["acts"], ref["rews"], lens, "env_ids")
    _, _, row_env, row_t, offsets, dlens, n_rows = tc.backward_args(ref)
    out = torch.full((B, S + 3), float("nan"), device="cuda")
    trk.prefix_states(row_env, row_t, offsets, dlens, n_rows, out, out_stride=S + 3)
    got = out.cpu().numpy()
    assert np.isnan(got[:, S:]).all() and np.isnan(got[lens == 0]).all() and not np.isnan(got[lens > 0, :S]).any()
    has = np.where(lens > 0)[0]
    want = ref["s64"][has, lens[has] - 1]
    err, bar = float(np.abs(got[has, :S] - want).max() / ref["s_scale"]), tc.bar_for(ref["s_e32"])
    print(f"prefix states {name}: device {err:.3e}  float32 restatement {ref['s_e32']:.3e}  bar {bar:.3e}  share {err / bar:.2f}")
    assert err <= bar


def test_helpers_agree_with_the_present_tests():
    """trackercase's row description is the one tests/test_gpu_tracker_bwd.py feeds the backward with."""
    lens = np.array([3, 0, 5, 1])
    for a, b in zip(tc.rows_of(lens), rows_of(lens)):
        np.testing.assert_array_equal(a, b)
