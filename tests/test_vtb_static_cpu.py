"""CPU: evaluation.test_taobao's host path against the reference's own run (tests/golden/vtbstatic.npz, written by
tools/gen_golden_vtbstatic.py), and everything of the device path that is decided on the host: the model-shape and env-mode refusals,
the argument validation of the cirs_vtb_static_* entry points (before any launch) and the layouts of their structs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import vtbcase
import vtbstaticcase as case
from cirs_hip import abi


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "vtbstatic.npz"))


def _golden_model(z):
    model = case.two_task_model(case.DNN, stressed=False)
    model.load_state_dict({k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("sd_")})
    return model.eval()


def _static_env(golden_dir, N=case.N_LEAVE, thr=case.THR, T=case.MAX_TURN):
    env = vtbcase.base_vtb(golden_dir, N, thr, T)
    env.set_state_mode(True)
    return env


@pytest.mark.parametrize("tag,eps", case.RUNS)
def test_host_path_reproduces_the_reference(golden_dir, tag, eps):
    import evaluation
    z = _golden(golden_dir)
    assert z["env_params"].tolist() == [case.N_LEAVE, case.THR, case.MAX_TURN]
    model = _golden_model(z)
    torch.manual_seed(case.TORCH_SEED)
    np.random.seed(case.NUMPY_SEED)
    env = _static_env(golden_dir)          # constructed after the seeding, as the generator does: the constructor draws too
    rec = case.Recorder(model, env)
    rec.env.static = True
    res = evaluation.test_taobao(rec, rec.env, eps, num_trajectory=case.N_TRAJ)
    got = rec.arrays()
    assert got["state"].shape == z[f"{tag}_state"].shape, "another number of env steps than the reference played"
    np.testing.assert_array_equal(got["state"], z[f"{tag}_state"])          # one-hot user, last draws, turn: integers
    np.testing.assert_array_equal(got["reward"], z[f"{tag}_reward"])
    np.testing.assert_array_equal(got["done"], z[f"{tag}_done"])
    np.testing.assert_allclose(got["action"], z[f"{tag}_action"], rtol=1e-5, atol=0)
    np.testing.assert_allclose(got["reward_pred"], z[f"{tag}_reward_pred"], rtol=1e-5, atol=0)
    np.testing.assert_allclose([res[k] for k in case.KEYS], z[f"{tag}_result"], rtol=1e-6, atol=0)
    assert set(res) == set(case.KEYS)
    if eps > 0:   # the exploration branch was taken somewhere: its actions are float64 uniforms of [0, 1), not fp32 predictions
        ex = (got["action"] != got["action"].astype(np.float32)).any(1)
        assert ex.any() and not ex.all()
        assert (got["action"][ex] >= 0).all() and (got["action"][ex] < 1).all()


def test_host_path_never_touches_the_device(golden_dir, monkeypatch):
    import evaluation
    from cirs_hip import vtb_static

    def boom(*a, **k):
        raise AssertionError("the host path must not load the library or build a device evaluation")

    monkeypatch.setattr(abi, "lib", boom)
    monkeypatch.setattr(vtb_static.DeviceVtbStaticEval, "__init__", boom)
    monkeypatch.setattr(torch.Tensor, "cuda", boom)
    z = _golden(golden_dir)
    res = evaluation.test_taobao(_golden_model(z), _static_env(golden_dir), 0.3, device=None, num_trajectory=3)
    assert set(res) == set(case.KEYS) and 1 <= res["len_tra"] <= case.MAX_TURN


def test_non_static_env_is_refused(golden_dir):
    import evaluation
    from cirs_hip.vtb_static import DeviceVtbStaticEval
    env = vtbcase.base_vtb(golden_dir, 4, 0.02, 7)
    model = case.two_task_model((32, 16))
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="static"):
            evaluation.test_taobao(model, env, device=dev)
    with pytest.raises(ValueError, match="static"):
        DeviceVtbStaticEval(env, model, 4)


def test_model_shape_refusals_happen_on_the_host(golden_dir):
    import collections
    from core.user_model_mmoe import UserModel_MMOE
    from deepctr_torch.inputs import DenseFeat
    from cirs_hip.vtb_static import DeviceVtbStaticEval, policy_shape

    def build(x_dim=91, ys=(("feat_item", 27), ("y", 1)), **kw):
        yc = [DenseFeat(n, d) for n, d in ys]
        tasks = collections.OrderedDict({f.name: "regression" for f in yc})
        return UserModel_MMOE([DenseFeat("feat_user", x_dim)], yc, len(tasks), tasks, {f.name: f.dimension for f in yc}, seed=1, device="cpu", **kw)

    ok = [dict(dnn_hidden_units=(256, 256)), dict(dnn_hidden_units=(96,), num_experts=2, expert_dim=5), dict(dnn_hidden_units=(8, 256, 1)),
          dict(dnn_hidden_units=(64,), num_experts=8, expert_dim=8), dict(dnn_hidden_units=(64,), num_experts=64, expert_dim=1)]
    for kw in ok:
        s = policy_shape(build(**kw))
        assert s["hidden"] == list(kw["dnn_hidden_units"]) and s["task_dim"] == [27, 1] and s["d_in"] == 91
    bad = [(dict(dnn_hidden_units=(257,)), "hidden widths"), (dict(dnn_hidden_units=(8, 8, 8, 8)), "4 hidden layers"),
           (dict(dnn_hidden_units=(64,), num_experts=5, expert_dim=13), "5 experts of dim 13"), (dict(x_dim=118, dnn_hidden_units=(64,)), "118 inputs"),
           (dict(ys=(("y", 1),), dnn_hidden_units=(64,)), "tasks"), (dict(ys=(("y", 1), ("feat_item", 27)), dnn_hidden_units=(64,)), "tasks"),
           (dict(ys=(("feat_item", 26), ("y", 1)), dnn_hidden_units=(64,)), "tasks"),
           (dict(ys=(("feat_item", 27), ("y", 1), ("z", 1)), dnn_hidden_units=(64,)), "tasks"),
           (dict(ys=(("feat_item", 27), ("y", 2)), dnn_hidden_units=(64,)), "tasks")]
    env = _static_env(golden_dir)
    for kw, why in bad:
        model = build(**kw)
        with pytest.raises(ValueError, match=why):
            policy_shape(model)
        with pytest.raises(ValueError, match=why):       # device="cuda" on a machine without one: the refusal comes first
            DeviceVtbStaticEval(env, model, 4, device="cuda")
    with pytest.raises(ValueError, match="not a UserModel_MMOE"):
        policy_shape(torch.nn.Linear(91, 28))
    # the trainer keeps refusing the two-task model: training it on the device is not part of this path
    with pytest.raises(ValueError, match="one regression task"):
        from core.user_model_mmoe import loss_taobao
        build(dnn_hidden_units=(64, 64)).compile("adam", loss_func=loss_taobao)


def _cfg(**kw):
    from cirs_hip.vtb_static import shape_struct
    shape = dict(d_in=91, n_dnn=2, hidden=[256, 256], experts=4, expert_dim=8, n_tasks=2, task_dim=[27, 1])
    shape.update({k: kw.pop(k) for k in list(kw) if k in shape})
    base = dict(n_traj=100, max_turn=50, num_leave_compute=5, leave_threshold=3.0, epsilon=0.3, policy=shape_struct(shape))
    base.update(kw)
    return abi.VtbStaticCfg(**base)


def test_struct_sizes_match_header_layout():
    assert C.sizeof(abi.VtbMmoeShape) == 10 * 4
    assert C.sizeof(abi.VtbMmoeWeights) == 15 * 8
    assert C.sizeof(abi.VtbStaticCfg) == 4 * 4 + 2 * 8 + 10 * 4
    assert C.sizeof(abi.VtbStaticOut) == 8 * 8
    assert abi.vtb_static_metrics_bytes(100) == 4 * 8 + 2 * 8 + 4 * 100
    # the env's ABI is untouched
    assert C.sizeof(abi.VtbCfg) == 14 * 4 + 3 * 8 and C.sizeof(abi.VtbWeights) == 20 * 8


def test_entry_points_validate_before_any_launch():
    lib = abi.lib()
    assert lib.cirs_vtb_static_workspace_bytes(C.byref(_cfg())) == 12 * 100
    assert lib.cirs_vtb_static_workspace_bytes(C.byref(_cfg(n_traj=37, hidden=[96, 0], n_dnn=1, experts=2, expert_dim=5))) == 12 * 37
    assert lib.cirs_vtb_static_workspace_bytes(None) == -1 and b"cfg is null" in lib.cirs_last_error()
    bad = [(dict(n_traj=0), b"n_traj"), (dict(n_traj=(1 << 20) + 1), b"n_traj"), (dict(max_turn=0), b"max_turn"), (dict(max_turn=16384), b"max_turn"),
           (dict(num_leave_compute=-1), b"num_leave_compute"), (dict(epsilon=-0.1), b"epsilon"), (dict(epsilon=1.5), b"epsilon"),
           (dict(epsilon=float("nan")), b"epsilon"), (dict(leave_threshold=float("nan")), b"leave_threshold"), (dict(d_in=118), b"d_in must be 91"),
           (dict(n_dnn=0), b"hidden layers"), (dict(n_dnn=4), b"hidden layers"), (dict(hidden=[256, 257]), b"hidden widths"),
           (dict(hidden=[0, 64]), b"hidden widths"), (dict(experts=9, expert_dim=8), b"experts"), (dict(experts=0), b"experts"),
           (dict(n_tasks=1), b"two tasks"), (dict(task_dim=[27, 2]), b"two tasks"), (dict(task_dim=[1, 27]), b"two tasks")]
    for kw, name in bad:
        assert lib.cirs_vtb_static_workspace_bytes(C.byref(_cfg(**kw))) == -1, kw
        assert name in lib.cirs_last_error(), (kw, lib.cirs_last_error())
        rc = lib.cirs_vtb_static_eval(C.byref(_cfg(**kw)), None, None, 0, None, None, 0, None)
        assert rc == -1 and name in lib.cirs_last_error(), kw
    # null arguments, in the order they are checked; a valid cfg never gets as far as a launch without them
    cfg, w, pw, out = _cfg(), abi.VtbWeights(), abi.VtbMmoeWeights(), abi.VtbStaticOut()

    def rc_msg(*args):
        return lib.cirs_vtb_static_eval(*args), lib.cirs_last_error()

    assert rc_msg(None, None, None, 0, None, None, 0, None) == (-1, b"vtb static cfg is null")
    assert rc_msg(C.byref(cfg), None, None, 0, None, None, 0, None) == (-1, b"vtb weights is null")
    assert rc_msg(C.byref(cfg), C.byref(w), None, 0, None, None, 0, None) == (-1, b"policy weights is null")
    assert rc_msg(C.byref(cfg), C.byref(w), C.byref(pw), 0, None, None, 0, None) == (-1, b"vtb static out is null")
    assert rc_msg(C.byref(cfg), C.byref(w), C.byref(pw), 0, C.byref(out), None, 0, None) == (-1, b"generator weight is null")
    for k in abi.VTB_WEIGHT_FIELDS[:10]:
        setattr(w, k, 64)       # never dereferenced on the host
    assert rc_msg(C.byref(cfg), C.byref(w), C.byref(pw), 0, C.byref(out), None, 0, None) == (-1, b"policy weight is null")
    pw = abi.VtbMmoeWeights(dnn_w=(C.c_void_p * 3)(64, 64, None), dnn_b=(C.c_void_p * 3)(64, 64, None), expert_w=64, expert_b=64,
                            gate_w=(C.c_void_p * 2)(64, 64), tower_w=(C.c_void_p * 2)(64, 64), lin_w=64, bias=(C.c_void_p * 2)(64, 64))
    assert rc_msg(C.byref(cfg), C.byref(w), C.byref(pw), 0, C.byref(out), None, 0, None) == (-1, b"vtb static out has a null field")
    out = abi.VtbStaticOut(**{k: 64 for k, _ in abi.VtbStaticOut._fields_})
    assert rc_msg(C.byref(cfg), C.byref(w), C.byref(pw), 0, C.byref(out), None, 0, None) == (-1, b"workspace is null")
    rc, msg = rc_msg(C.byref(cfg), C.byref(w), C.byref(pw), 0, C.byref(out), 64, 12 * 100 - 1, None)
    assert rc == -1 and b"workspace too small" in msg
    rc, msg = rc_msg(C.byref(cfg), C.byref(w), C.byref(pw), 0, C.byref(out), 68, 12 * 100, None)
    assert rc == -1 and b"aligned" in msg
    # the noise export
    assert lib.cirs_vtb_static_noise(0, None, None, 0, None, None) == 0
    assert lib.cirs_vtb_static_noise(0, None, None, -1, None, None) == -1 and b"n must be" in lib.cirs_last_error()
    assert lib.cirs_vtb_static_noise(0, None, None, 3, None, None) == -1 and b"null argument" in lib.cirs_last_error()


def _double(seq):
    m = torch.nn.Sequential(*[torch.nn.Linear(l.in_features, l.out_features) if isinstance(l, torch.nn.Linear) else torch.nn.LeakyReLU() for l in seq]).double()
    m.load_state_dict({k: v.double() for k, v in seq.state_dict().items()})
    return m


@pytest.mark.parametrize("shape,n", case.GPU_CASES)
@pytest.mark.parametrize("eps", case.GPU_EPS)
def test_margin_cap_holds_for_the_gpu_cases_inputs(golden_dir, shape, n, eps):
    """tests/test_gpu_vtb_static.py lets the top-2 margin protocol excuse at most 0.1 % of a run's click / second draws and no user
    draw.  Both are conditions on the inputs, checked here for each of its cases (same model, exit threshold, max_turn, n, epsilon and
    seed number): the host path plays the case, and on every (user, turn, action) it visits the fp32 mirror's draw is compared with a
    float64 restatement of the same module under the same Gumbels; likewise every user draw against a float64 generator.
    What this cannot use without a GPU is the device's Philox stream: the Gumbels here come from torch's generator seeded with the
    case's seed, so the visited states are draws from the same distribution as the device run's, not the same draws."""
    s = case.GPU_SHAPES[shape]
    model = case.two_task_model(s["dnn"], s["num_experts"], s["expert_dim"])
    torch.manual_seed(case.GPU_SEED)
    np.random.seed(case.GPU_SEED)
    env = vtbcase.base_vtb(golden_dir, case.GPU_N_LEAVE, s["thr"], case.GPU_T)
    env.set_state_mode(True)
    zs = []
    rand = torch.rand

    def rec_rand(*a, **k):      # the generator's z of every user draw
        z = rand(*a, **k)
        zs.append(z.clone())
        return z

    import evaluation
    rec = case.Recorder(model, env)
    rec.env.static = True
    torch.rand = rec_rand
    try:
        evaluation.test_taobao(rec, rec.env, eps, num_trajectory=n)
    finally:
        torch.rand = rand
    d = rec.arrays()
    k = len(d["done"])
    x = torch.from_numpy(np.concatenate([d["state"][:, :88], d["state"][:, 90:91], d["action"]], 1).astype(np.float32))
    gen = torch.Generator().manual_seed(case.GPU_SEED)
    g = -torch.log(-torch.log(torch.rand((k, 21), generator=gen).clamp(1e-7, 1 - 1e-7)))
    with torch.no_grad():
        v32, v64 = env.action_model(x) + g, _double(env.action_model)(x.double()) + g.double()
    differ = int((v32[:, :11].argmax(1) != v64[:, :11].argmax(1)).sum() + (v32[:, 11:].argmax(1) != v64[:, 11:].argmax(1)).sum())
    z = torch.cat(zs)
    gu = -torch.log(-torch.log(torch.rand((len(z), 88), generator=gen).clamp(1e-7, 1 - 1e-7)))
    with torch.no_grad():
        u32, u64 = env.generator(z) + gu, _double(env.generator)(z.double()) + gu.double()
    udiffer = sum(int((u32[:, lo:hi].argmax(1) != u64[:, lo:hi].argmax(1)).sum()) for lo, hi in vtbcase.GROUPS)
    print(f"{shape} n={n} eps={eps}: {k} steps, {differ} of {2 * k} click / second draws and {udiffer} of {11 * len(z)} user draws differ fp32 vs float64")
    assert len(z) >= n and differ <= 0.001 * 2 * k and udiffer == 0
