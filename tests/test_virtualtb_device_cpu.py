"""CPU: the device VirtualTaobao entry points validate their arguments on the host before any launch (safe without a GPU), and
DummyVectorEnv without `device` keeps the host path of VirtualTB-v0 / SimulatedEnv(VirtualTB-v0) exactly."""
import ctypes as C
import os

import numpy as np
import torch

from cirs_hip import abi


def _cfg(**kw):
    c = dict(n_env=4, max_turn=50, num_leave_compute=5, simulated=1, version=1, use_exposure=1, mmoe_d_in=118, mmoe_dnn_layers=2,
             mmoe_h1=128, mmoe_h2=128, mmoe_experts=4, mmoe_expert_dim=8, mmoe_tasks=1, mmoe_task_dim=1, leave_threshold=3.0, tau=1.0,
             gamma_exposure=1.0)
    c.update(kw)
    return abi.VtbCfg(**c)


def _weights(skip=()):
    return abi.VtbWeights(**{k: (None if k in skip else 0x1000 + 0x100 * i) for i, k in enumerate(abi.VTB_WEIGHT_FIELDS)})


def _err(lib):
    return lib.cirs_last_error().decode()


def test_vtb_entry_points_reject_bad_arguments():
    lib = abi.lib()
    st = abi.VtbState()
    w = _weights()
    step = lambda cfg, w, st, n=1, act=1: lib.cirs_vtb_step(cfg and C.byref(cfg), w and C.byref(w), C.byref(st), 0, act, None, n,
                                                          1, 1, 1, 1, None, None)
    assert step(None, w, st) == -1 and "cfg" in _err(lib)
    assert step(_cfg(), None, st) == -1 and "weights" in _err(lib)
    assert step(_cfg(version=3), w, st) == -1 and "version" in _err(lib)
    assert step(_cfg(max_turn=0), w, st) == -1 and "max_turn" in _err(lib)
    assert step(_cfg(n_env=0), w, st) == -1 and "n_env" in _err(lib)
    assert step(_cfg(mmoe_experts=3), w, st) == -1 and "MMoE shape" in _err(lib)
    assert step(_cfg(mmoe_dnn_layers=3), w, st) == -1 and "MMoE shape" in _err(lib)
    assert step(_cfg(), _weights(skip=("mm_wg",)), st) == -1 and "MMoE weight" in _err(lib)
    assert step(_cfg(), _weights(skip=("act_w2",)), st) == -1 and "action-model" in _err(lib)
    assert step(_cfg(), w, st, n=5) == -1 and "n out of range" in _err(lib)
    assert step(_cfg(), w, st) == -1 and "state" in _err(lib)          # null state fields
    assert step(_cfg(), w, st, n=0) == 0                               # empty batch: nothing to do
    # the raw kind needs no MMoE
    assert step(_cfg(simulated=0, mmoe_experts=0), _weights(skip=("mm_w1",)), st) == -1 and "state" in _err(lib)
    full = abi.VtbState(**{k: 0x2000 for k, _ in abi.VtbState._fields_})
    assert step(_cfg(), w, full, act=None) == -1 and "null action" in _err(lib)
    assert lib.cirs_vtb_reset(None, C.byref(w), C.byref(st), 0, None, 1, None, None) == -1 and "cfg" in _err(lib)
    assert lib.cirs_vtb_reset(C.byref(_cfg()), C.byref(w), C.byref(st), 0, None, 2, None, None) == -1 and "state" in _err(lib)
    assert lib.cirs_vtb_noise(0, None, None, 3, None, None) == -1 and "null" in _err(lib)
    assert lib.cirs_vtb_noise(0, None, None, 0, None, None) == 0
    assert lib.cirs_vtb_mmoe_forward(C.byref(_cfg(mmoe_h1=64)), C.byref(w), 1, 1, 1, None) == -1 and "MMoE shape" in _err(lib)
    assert lib.cirs_vtb_mmoe_forward(C.byref(_cfg()), C.byref(w), None, 1, 1, None) == -1 and "null" in _err(lib)


def test_vtb_struct_layout():
    assert C.sizeof(abi.VtbCfg) == 14 * 4 + 3 * 8
    assert C.sizeof(abi.VtbWeights) == 20 * 8
    assert C.sizeof(abi.VtbState) == 8 * 8


def _run_host(golden_dir, device_kw):
    import gym
    from gym.envs.registration import register
    import vtbcase
    from tianshou.env import DummyVectorEnv
    from cirs_hip import gymlite
    gymlite.install()
    model, _ = vtbcase.golden_mmoe(golden_dir)
    register(id="VirtualTB-v0", entry_point="environments.VirtualTaobao.virtualTB.envs.virtualTB:VirtualTB",
             kwargs=dict(num_leave_compute=4, leave_threshold=2.4, max_turn=9, data_dir=os.path.join(golden_dir, "virtualtb")))
    register(id="SimulatedEnv-v0", entry_point="core.env.simulatedEnv.simulated_env:SimulatedEnv",
             kwargs=dict(user_model=model, task_name="VirtualTB-v0", version="v2", tau=1.0, gamma_exposure=0.5))
    out = []
    for name in ("SimulatedEnv-v0", "VirtualTB-v0"):
        torch.manual_seed(5)
        venv = DummyVectorEnv([lambda: gym.make(name) for _ in range(3)], **device_kw)
        assert venv.host_mode and venv._vtb is None
        venv.seed(7)
        rng = np.random.RandomState(1)
        res = [venv.reset()]
        for k in range(10):     # up to t == max_turn, the last turn the simulated kind can step
            ids = np.array([0, 2]) if k % 3 == 2 else np.arange(3)
            o, r, d, info = venv.step(rng.uniform(-1, 1, (len(ids), 27)).astype(np.float32), ids)
            res += [o, r, d, info["CTR"], info["env_id"]]
        out.append(res)
    return out


def test_vector_env_without_device_keeps_the_host_path(golden_dir):
    a = _run_host(golden_dir, {})
    b = _run_host(golden_dir, dict(device=None))
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            assert np.asarray(x).dtype == np.asarray(y).dtype
            np.testing.assert_array_equal(x, y)
    assert a[1][2].dtype == np.int64 and a[0][1].shape == (3, 30)    # raw kind: integer click rewards; obs [k, 30]
