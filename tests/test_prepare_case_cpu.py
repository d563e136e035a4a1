"""CPU: the numpy restatement of the PPO process_fn stage (tests/preparecase.py) is anchored to the reference -- the oracle's GAE and RunningMeanStd,
the C oracle's _gae_return and the reference's own recordings -- and to long double, never to the device.  tests/test_gpu_prepare_f64.py then holds
the kernels of csrc/ppo.hip to it at 2^-40 M; that bar rests on the 2^-44 M asserted here.

Worst float64-versus-long-double ratio over all cases and carried calls (fractions of 2^-44 M): adv 0.0098, unnorm 0.0088, ret 0.59 (the second call
of carry-b, whose scale is 1e-4; 0.0094 elsewhere) -- profiles/prepare_f64_margins.md."""
import numpy as np
import pytest
import torch

import nn_oracle
import oracle_lib
import preparecase as pc
from conftest import close
from test_oracle_learn import POL, load_learn

CALLS = [(k, None) for k in pc.IDS] + [(s, i) for s in pc.SEQUENCES for i in range(len(pc.SEQUENCES[s]))]
CALL_IDS = [k if i is None else f"{k}[{i}]" for k, i in CALLS]


def _call(key, i):
    """(case, float64 restatement, long double restatement, rms before the call, rew_norm)"""
    if i is None:
        return pc.reference(key) + (pc.RMS0, pc.CASES[key][1])
    seq = pc.sequence_reference(key)
    return seq[i] + (pc.RMS0 if i == 0 else seq[i - 1][1]["rms"], True)


def _flat(x_tb, lens):
    return np.concatenate([x_tb[:int(L), b] for b, L in enumerate(lens)])


@pytest.mark.parametrize("key,i", CALLS, ids=CALL_IDS)
def test_restatement_equals_the_oracle_functions(key, i):
    """On the flattened buffer, formed here without the restatement: GAE == nn_oracle.gae_numpy == the C oracle's oracle_gae_return, returns and the
    running statistics == compute_returns' expressions and nn_oracle.RunningMeanStd.  The operations are the same ones in the same order: exact."""
    c, w, _, rms0, rew_norm = _call(key, i)
    lens = c["lens"]
    scale = np.sqrt(np.float64(rms0[1]) + 1e-8) if rew_norm else np.float64(1.0)
    value, rew, done = _flat(c["value"], lens), _flat(c["rew"], lens), _flat(c["done"], lens).astype(bool)
    assert done[-1] and not np.isnan(value).any() and not np.isnan(rew).any()
    v_s = value.astype(np.float64) * scale
    v_ns = np.roll(value, -1).astype(np.float64) * scale * (~done)
    adv = nn_oracle.gae_numpy(v_s, v_ns, rew, done.astype(np.float64), pc.GAMMA, pc.LAM)
    np.testing.assert_array_equal(w["adv"], adv)
    out = np.zeros_like(rew)
    end = np.ascontiguousarray(done, np.uint8)
    assert oracle_lib.lib().oracle_gae_return(v_s.ctypes.data, v_ns.ctypes.data, rew.ctypes.data, end.ctypes.data, len(rew), pc.GAMMA, pc.LAM, out.ctypes.data) == 0
    np.testing.assert_array_equal(w["adv"], out)
    unnorm = adv + v_s
    np.testing.assert_array_equal(w["unnorm"], unnorm)
    np.testing.assert_array_equal(w["ret"], unnorm / scale)
    rms = nn_oracle.RunningMeanStd()
    rms.mean, rms.var, rms.count = rms0
    if rew_norm:
        rms.update(unnorm)
    np.testing.assert_array_equal(np.array(w["rms"], np.float64), [rms.mean, rms.var, rms.count])
    assert w["rms"][2] == rms.count and (rew_norm or tuple(w["rms"]) == tuple(rms0))
    # the exact copies and the buffer order
    np.testing.assert_array_equal(w["v_s"], value)
    np.testing.assert_array_equal(w["logp_old"], _flat(c["logp"], lens))
    np.testing.assert_array_equal(w["act"], _flat(c["act"], lens))
    np.testing.assert_array_equal(w["obs"], np.concatenate([c["obs"][:int(L), b] for b, L in enumerate(lens)]))
    np.testing.assert_array_equal(w["offsets"], np.cumsum(lens) - lens)
    assert w["n"] == lens.sum() == len(adv)
    for k in ("adv", "unnorm", "ret", "v_s", "logp_old", "obs"):
        assert not np.isnan(w[k].astype(np.float64)).any(), f"poison reached {k}"
    assert (w["act"] >= 0).all() and np.isfinite(w["M"])


@pytest.mark.parametrize("key,i", CALLS, ids=CALL_IDS)
def test_float64_restatement_against_long_double(key, i):
    """max |float64 - long double| <= 2^-44 M for adv, unnorm and ret: what the device bar (2^-40 M, 16 x this) takes for granted"""
    _, w64, wld, _, _ = _call(key, i)
    assert wld["adv"].dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63, "long double is no wider than double on this platform"
    used = pc.f64_vs_longdouble(w64, wld)
    print(f"prepare {CALL_IDS[CALLS.index((key, i))]}: f64 vs long double  adv {used['adv']:.2g}  unnorm {used['unnorm']:.2g}  ret {used['ret']:.2g}  of 2^-44 M, M {w64['M']:.3g}")
    assert max(used.values()) <= 1.0, used
    for a, b in zip(w64["rms"], wld["rms"]):
        assert abs(np.longdouble(a) - b) <= np.longdouble(1e-14) * max(abs(b), 1)


def _values(pp, obs_bts, lens):
    """critic values at rollout time, [T, B] float32 (torch fp32 on the host, as tests/test_gpu_learn.py forms the kernels' input)"""
    B, T = obs_bts.shape[0], obs_bts.shape[1] - 1
    value = np.zeros((T, B), np.float32)
    with torch.no_grad():
        for b in range(B):
            L = int(lens[b])
            value[:L, b] = nn_oracle.policy_forward(pp, torch.as_tensor(obs_bts[b, :L]))[1].numpy()
    return value


def _recorded(z, pp, pre):
    lens = z[pre + "lens"]
    B, T = z[pre + "acts"].shape
    return dict(value=_values(pp, z[pre + "obs"], lens), logp=np.zeros((T, B), np.float32), rew=z[pre + "rews"].T, act=z[pre + "acts"].T,
                done=z[pre + "dones"].T, obs=z[pre + "obs"].transpose(1, 0, 2), lens=lens)


def test_restatement_reproduces_the_reference_recordings(golden_dir):
    """tests/golden/learn.npz: both recorded rounds (the second from the first round's running variance and the updated critic) at the tolerances
    tests/test_gpu_learn.py and tests/test_gpu_tracker_bwd.py hold the device to; learn_opts.npz: the first pass's advantages."""
    z, _, pp, _ = load_learn(golden_dir)
    gamma, lam = float(z["hyper"][0]), float(z["hyper"][1])
    c1 = _recorded(z, pp, "")
    w1 = pc.restate(c1, c1["lens"], pc.RMS0, gamma, lam, True, np.float64)
    close(w1["adv"].astype(np.float32), z["b_adv"], 1e-5, 2e-6, "prepare restatement: b_adv")
    close(w1["ret"].astype(np.float32), z["b_returns"], 1e-5, 2e-6, "prepare restatement: b_returns")
    close(w1["v_s"], z["b_v_s"], 1e-5, 2e-6, "prepare restatement: b_v_s")
    np.testing.assert_array_equal(w1["act"], z["b_act"].astype(np.int64))
    close(np.array(w1["rms"], np.float64), z["ret_rms"], 1e-5, 0.0, "prepare restatement: ret_rms")
    pp2 = {k: torch.as_tensor(z["post_pol_" + name]).float() for k, name in POL.items()}
    c2 = _recorded(z, pp2, "r2_")
    w2 = pc.restate(c2, c2["lens"], w1["rms"], gamma, lam, True, np.float64)
    close(w2["adv"].astype(np.float32), z["r2_b_adv"], 1e-5, 2e-6, "prepare restatement: r2_b_adv")
    close(w2["ret"].astype(np.float32), z["r2_b_returns"], 1e-5, 2e-6, "prepare restatement: r2_b_returns")
    close(w2["v_s"], z["r2_b_v_s"], 1e-5, 2e-6, "prepare restatement: r2_b_v_s")
    close(np.array(w2["rms"], np.float64), z["r2_ret_rms"], 1e-5, 0.0, "prepare restatement: r2_ret_rms")
    assert w2["rms"][2] == z["lens"].sum() + z["r2_lens"].sum()
    # the carried variance matters on this fixture: from a fresh RunningMeanStd the second round's returns miss their bar
    fresh = pc.restate(c2, c2["lens"], pc.RMS0, gamma, lam, True, np.float64)
    assert np.abs(fresh["ret"] - z["r2_b_returns"]).max() > 1e-2
    zo, _, ppo, _ = load_learn(golden_dir, "learn_opts")
    co = _recorded(zo, ppo, "")
    wo = pc.restate(co, co["lens"], pc.RMS0, float(zo["hyper"][0]), float(zo["hyper"][1]), True, np.float64)
    close(wo["adv"].astype(np.float32), zo["b_adv"], 1e-5, 2e-6, "prepare restatement: learn_opts b_adv")


# ---- the inputs themselves ---------------------------------------------------------------------------------------------------------
TABLE = {"one": (1, 1), "every-length": (26, 25), "long": (5, 100), "wave-63": (63, 17), "wave-64": (64, 17), "wave-65": (65, 17), "envs-1025": (1025, 8),
         "envs-2049": (2049, 9), "rows-1023": (130, 12), "rows-1024": (130, 12), "rows-1025": (130, 12), "rows-8191": (1030, 12), "rows-8192": (1030, 12),
         "rows-8193": (1030, 12), "rows-16385": (1100, 30), "one-b": (1, 1)}


def test_the_cases_reach_the_edges_they_are_named_for():
    assert set(pc.SPECS) == set(TABLE)
    assert set(pc.CASES) == (set(TABLE) - {"one-b"}) | {"every-length/raw", "rows-8193/raw"}
    assert pc.CASES["every-length/raw"] == ("every-length", False) and pc.CASES["rows-8193/raw"] == ("rows-8193", False)
    for k, (B, T) in TABLE.items():
        sp = pc.SPECS[k]
        assert (sp["B"], sp["T"]) == (B, T) and sp["lens"].shape == (B,) and sp["lens"].min() >= 1 and sp["lens"].max() <= T, k
    lens = {k: sp["lens"] for k, sp in pc.SPECS.items()}
    assert lens["one"].tolist() == [1] and lens["one-b"].tolist() == [1] and pc.SPECS["one"]["seed"] != pc.SPECS["one-b"]["seed"]
    assert sorted(lens["every-length"].tolist()) == list(range(1, 26)) + [25]
    assert lens["long"].tolist() == [100, 1, 99, 64, 65]
    for B in (63, 64, 65):
        assert lens[f"wave-{B}"].tolist() == [(b % 17) + 1 for b in range(B)]
    for k, N in pc.ROW_CASES.items():                                # lens_with_sum: the exact row count of each row case, lengths not all alike
        assert int(lens[k].sum()) == N and len(set(lens[k].tolist())) >= TABLE[k][1] // 2, k
    assert sorted(pc.ROW_CASES.values()) == [1023, 1024, 1025, 8191, 8192, 8193, 16385]
    assert lens["envs-2049"].sum() > 8192 and set(lens["envs-1025"].tolist()) == set(range(1, 9)) and set(lens["envs-2049"].tolist()) == set(range(1, 10))
    assert pc.SEQUENCES == {"carry-a": ["every-length", "one", "wave-65"], "carry-b": ["one", "one-b", "every-length"]}
    seq = pc.sequence_reference("carry-b")
    assert seq[0][1]["rms"][1] == 0.0 and seq[1][1]["scale"] == np.sqrt(1e-8)      # the second call starts from variance 0, scale 1e-4
    rng = np.random.RandomState(0)
    for B, T, N in ((1, 1, 1), (3, 4, 3), (3, 4, 12), (7, 5, 20)):
        got = pc.lens_with_sum(B, T, N, rng)
        assert got.sum() == N and got.min() >= 1 and got.max() <= T and got.shape == (B,)


@pytest.mark.parametrize("name", list(TABLE))
def test_every_dead_slot_is_poisoned(name):
    c = pc.trajectory(name)
    B, T, lens = c["B"], c["T"], c["lens"].astype(np.int64)
    assert c["value"].dtype == np.float32 and c["logp"].dtype == np.float32 and c["rew"].dtype == np.float64 and c["obs"].dtype == np.float32
    assert c["obs"].shape == (T + 1, B, pc.S)
    t = np.arange(T)[:, None]
    live, dead = t < lens[None, :], t >= lens[None, :]
    for k in ("value", "logp", "rew"):
        assert np.isnan(c[k][dead]).all() and np.isfinite(c[k][live]).all(), k
    assert (c["act"][dead] == -1).all() and (c["act"][live] >= 0).all() and (c["act"][live] < pc.N_ITEMS).all()
    assert (c["logp"][live] < 0).all() and (np.abs(c["rew"][live]) <= 1).all()
    last = t == (lens - 1)[None, :]
    assert (c["done"][dead] == 1).all() and (c["done"][last] == 1).all() and (c["done"][live & ~last] == 0).all()      # among the live steps: 1 only at lens - 1
    t1 = np.arange(T + 1)[:, None]
    assert np.isnan(c["obs"][t1 > lens[None, :]]).all() and np.isfinite(c["obs"][t1 <= lens[None, :]]).all()
