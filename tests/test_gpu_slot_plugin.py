"""GPU: StateTrackerGRU / LSTM / Avg / Caser behind the plugin objects (Collector / PPOPolicy / CollectorSet / the example script), wired as
tests/test_gpu_plugin_surface.py wires the Transformer tracker: one collect + update, checkpoint round trip, the test collectors.
tests/slotcase.py describes each tracker."""
import types

import numpy as np
import pytest
import torch

from slotcase import NAMES, SLOTS, load_example

pytestmark = pytest.mark.gpu
ARGV = ["--n-users", "100", "--n-items", "300", "--training-num", "16", "--episode-per-collect", "16", "--test-num", "8", "--batch-size", "64",
        "--max_turn", "8", "--tau", "10", "--force_length", "5", "--leave_threshold", "1", "--num_leave_compute", "3"]


def argv(slot):
    return ARGV + ["--tracker", slot.name] + slot.flags(slot.plugin_model)


@pytest.fixture(scope="module", params=SLOTS, ids=NAMES)
def wired(request):
    slot = request.param
    ex = load_example()
    args = ex.get_args(argv(slot))
    tab, train_envs, st, policy, coll = ex.build(args)
    return slot, ex, args, st, policy, coll


def test_collect_and_update_through_the_plugin_objects(wired):
    from core.state_tracker import _RecurrentStateTracker
    slot, ex, args, st, policy, coll = wired
    model, n_tensors = slot.plugin_model, slot.n_grad_tensors(slot.plugin_model)
    assert isinstance(st, slot.tracker_class()) and isinstance(st, _RecurrentStateTracker)
    for k, v in slot.plugin_kw(model).items():
        assert getattr(st, k) == v, k
    sd = st.state_dict()
    assert set(slot.state_names) <= set(sd) and len(sd) == n_tensors
    assert list(sd) == list(slot.param_shapes(100, 300, 20, model))
    # O(1) parameters (the init's embeddings are N(0, 1e-4): gradients of every tensor below would sit at the round-off floor)
    U, I, B, T, S = 100, 300, 16, 8, 20
    st.load_state_dict(slot.param_dict(U, I, slot.plugin_seed, S, model))
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
    slot.check_unambiguous(p0, users, acts, rews, lens, model)      # what the gradient check below presupposes, as the cases do
    g64 = slot.grads(p0, users, acts, rews, lens, G, model, torch.float64)
    g32 = slot.grads(p0, users, acts, rews, lens, G, model, torch.float32)
    assert set(eng.grad_views) == set(g64)
    changed = 0
    for k, gv in eng.grad_views.items():
        got, want = gv.cpu().numpy().astype(np.float64), g64[k]
        scale = np.abs(want).max() + 1e-300
        err, err32 = np.abs(got - want).max() / scale, np.abs(g32[k] - want).max() / scale
        bar = slot.case.bar_for(slot.case.GRAD_BAR, err32)
        print(f"plugin grad {slot.name} {k}: device {err:.3e}  float32 restatement {err32:.3e}  bar {bar:.3e}")
        assert err <= bar, k
        now = st.state_dict()[k].detach().cpu()
        assert torch.isfinite(now).all(), k
        if np.abs(got).max() > 0:
            assert not torch.equal(now, p0[k]), k + " has a gradient and did not move"
            changed += 1
        else:
            assert torch.equal(now, p0[k]), k + " has no gradient and moved"
    # every tensor takes part in every live state and the upstream gradient is dense: each has a gradient
    assert changed == n_tensors


def test_state_dict_round_trip_gives_the_same_greedy_collect(wired):
    from cirs_hip.rollout import DeviceRollout
    slot, ex, args, st, policy, coll = wired
    users = torch.as_tensor(np.random.RandomState(6).randint(0, 100, 16))
    ro = coll._get_rollout()
    l1 = ro.collect(users, greedy=True)
    want = {k: getattr(ro.traj, k).clone() for k in ("obs", "act", "rew", "logp", "value")}
    cols = ([types.SimpleNamespace(vocabulary_size=100)], [types.SimpleNamespace(vocabulary_size=300)], [])
    fresh = slot.tracker_class()(*cols, dim_model=32, dim_state=20, dim_max_batch=16, device="cuda:0", seed=77, MAX_TURN=8,
                                 **slot.plugin_kw(slot.plugin_model))
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


def test_collector_set_over_the_tracker(wired):
    slot, ex, args, st, policy, coll = wired
    cs = ex.build_test_collectors(args, policy, st)
    res = cs.collect(n_episode=8)
    assert {"n/st", "rew", "NX_0_n/st", "NX_5_lens"} <= set(res)
    assert (res["NX_5_lens"] == 5).all()
    nx = cs.collector_dict["NX_0"].buffer
    acts = nx._traj.act.cpu().numpy()
    for b in range(8):
        a = acts[:nx._lengths[b], b]
        assert len(set(a.tolist())) == len(a) and (a >= 0).all()


@pytest.mark.parametrize("slot", SLOTS, ids=NAMES)
def test_example_runs_with_the_tracker(slot, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ex = load_example()
    policy, st, result = ex.main(argv(slot) + ["--epoch", "2", "--step-per-epoch", "60"])
    assert type(st).__name__ == "StateTracker" + slot.display and st.adam_steps >= 2
    for k, v in slot.plugin_kw(slot.plugin_model).items():
        assert getattr(st, k) == v, k
    assert result["train_step"] >= 120
    assert all(torch.isfinite(v).all() for v in st.state_dict().values())
