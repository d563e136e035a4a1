"""GPU: StateTrackerCaser behind the plugin objects (Collector / PPOPolicy / CollectorSet / the example script), wired as
tests/test_gpu_lstm_plugin.py wires the LSTM tracker: one collect + update, checkpoint round trip, the test collectors."""
import types

import numpy as np
import pytest
import torch

import casercase
from cirs_hip import caser_host
from test_gpu_lstm_plugin import load_example

pytestmark = pytest.mark.gpu
W, HEIGHTS, PSEED = 4, (2, 3), 4
N_TENSORS = 12 + 2 * len(HEIGHTS)
ARGV = ["--n-users", "100", "--n-items", "300", "--training-num", "16", "--episode-per-collect", "16", "--test-num", "8", "--batch-size", "64",
        "--max_turn", "8", "--tau", "10", "--force_length", "5", "--leave_threshold", "1", "--num_leave_compute", "3", "--tracker", "caser",
        "--window-size", str(W), "--filter-sizes", ",".join(map(str, HEIGHTS))]


@pytest.fixture(scope="module")
def wired():
    ex = load_example()
    args = ex.get_args(ARGV)
    tab, train_envs, st, policy, coll = ex.build(args)
    return ex, args, st, policy, coll


def test_collect_and_update_through_the_plugin_objects(wired):
    from core.state_tracker import StateTrackerCaser, _RecurrentStateTracker
    ex, args, st, policy, coll = wired
    assert isinstance(st, StateTrackerCaser) and isinstance(st, _RecurrentStateTracker) and st.window_size == W and st.filter_sizes == HEIGHTS
    sd = st.state_dict()
    from cirs_hip.caser_tracker import caser_param_shapes
    assert list(sd) == list(caser_param_shapes(100, 300, 32, 20, W, HEIGHTS)) and len(sd) == N_TENSORS
    # O(1) parameters (the init's embeddings are N(0, 1e-4): gradients of every tensor below would sit at the round-off floor)
    U, I, B, T, S = 100, 300, 16, 8, 20
    st.load_state_dict(casercase.caser_param_dict(U, I, PSEED, W, HEIGHTS, S=S))
    p0 = {k: v.detach().cpu().clone() for k, v in st.state_dict().items()}
    users = np.random.RandomState(5).randint(0, U, B)
    res = coll.collect(n_episode=B, users=users)
    assert res["n/ep"] == B and res["n/st"] == int(res["lens"].sum())
    buf = coll.buffer
    steps0 = st.adam_steps
    losses = policy.update(0, buf, batch_size=64, repeat=2)
    assert set(losses) == {"loss", "loss/clip", "loss/vf", "loss/ent"}
    assert all(np.isfinite(v).all() for v in losses.values())
    assert st.adam_steps == steps0 + 1
    # the gradient left in the engine: the restatement's autograd with the learner's d loss / d obs as the upstream gradient
    ro = buf._rollout
    eng = ro.tracker
    lens = np.asarray(buf._lengths)
    acts = ro.traj.act.cpu().numpy().T.copy(); rews = ro.traj.rew.cpu().numpy().T.copy()
    G = policy._learner.dobs.cpu().numpy()
    assert G.shape == (T + 1, B, S)
    # the gradient check below presupposes what the cases presuppose: float64 itself is unambiguous at every max and ReLU of this rollout
    for what, (margin, e32) in casercase.near_tie_margins(p0, users, np.maximum(acts, 0), rews, lens, W).items():
        assert margin >= 8 * e32, f"the rollout's inputs sit near a tie ({what}): choose another PSEED"
    g64 = caser_host.grads(p0, users, acts, rews, lens, G, W, torch.float64)
    g32 = caser_host.grads(p0, users, acts, rews, lens, G, W, torch.float32)
    changed = 0
    for k, gv in eng.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), g64[k]
        scale = np.abs(want).max() + 1e-300
        err, err32 = np.abs(got - want).max() / scale, np.abs(g32[k] - want).max() / scale
        bar = casercase.bar_for(casercase.GRAD_BAR, err32)
        print(f"plugin grad {k}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar, k
        now = st.state_dict()[k].detach().cpu()
        assert torch.isfinite(now).all(), k
        if np.abs(got).max() > 0:
            assert not torch.equal(now, p0[k]), k + " has a gradient and did not move"
            changed += 1
        else:
            assert torch.equal(now, p0[k]), k + " has no gradient and moved"
    assert changed == N_TENSORS


def test_state_dict_round_trip_gives_the_same_greedy_collect(wired):
    from cirs_hip.rollout import DeviceRollout
    from core.state_tracker import StateTrackerCaser
    ex, args, st, policy, coll = wired
    users = torch.as_tensor(np.random.RandomState(6).randint(0, 100, 16))
    ro = coll._get_rollout()
    l1 = ro.collect(users, greedy=True)
    want = {k: getattr(ro.traj, k).clone() for k in ("obs", "act", "rew", "logp", "value")}
    cols = ([types.SimpleNamespace(vocabulary_size=100)], [types.SimpleNamespace(vocabulary_size=300)], [])
    fresh = StateTrackerCaser(*cols, dim_model=32, dim_state=20, dim_max_batch=16, device="cuda:0", seed=77, MAX_TURN=8, window_size=W, filter_sizes=HEIGHTS)
    assert not torch.equal(fresh.flat, st.flat)
    fresh.load_state_dict(st.state_dict())
    assert torch.equal(fresh.flat, st.flat)
    ro2 = DeviceRollout(ro.env, fresh.engine(16), ro.policy)
    l2 = ro2.collect(users, greedy=True)
    assert torch.equal(l1, l2)
    # (states past an env's end are not written by a collect: the first rollout's buffer still holds those of its earlier collects)
    live = torch.arange(9, device=l1.device)[:, None] <= l1[None, :].to(torch.int64)
    for k, v in want.items():
        if k == "obs":
            assert torch.equal(ro2.traj.obs[live], v[live]), k
        else:
            assert torch.equal(getattr(ro2.traj, k), v), k


def test_collector_set_over_the_caser_tracker(wired):
    ex, args, st, policy, coll = wired
    cs = ex.build_test_collectors(args, policy, st)
    res = cs.collect(n_episode=8)
    assert {"n/st", "rew", "NX_0_n/st", "NX_5_lens"} <= set(res)
    assert (res["NX_5_lens"] == 5).all()
    nx = cs.collector_dict["NX_0"].buffer
    acts = nx._traj.act.cpu().numpy()
    for b in range(8):
        a = acts[:nx._lengths[b], b]
        assert len(set(a.tolist())) == len(a) and (a >= 0).all()


def test_example_runs_with_the_caser_tracker(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ex = load_example()
    policy, st, result = ex.main(ARGV + ["--epoch", "2", "--step-per-epoch", "60"])
    assert type(st).__name__ == "StateTrackerCaser" and st.window_size == W and st.filter_sizes == HEIGHTS and st.adam_steps >= 2
    assert result["train_step"] >= 120
    assert all(torch.isfinite(v).all() for v in st.state_dict().values())
