"""Test-side helpers of the VirtualTaobao static-baseline evaluation (evaluation.test_taobao, cirs_hip/vtb_static.py): the fixture's
settings (shared with tools/gen_golden_vtbstatic.py), the two-task model, a recorder of what test_taobao feeds and gets, and the CPU
replay of a device run through the noise-fed mirror of tests/vtbcase.py."""
import collections

import numpy as np
import torch

import vtbcase

# ---- tests/golden/vtbstatic.npz ---------------------------------------------------------------------------------------------------
DNN, N_TRAJ, N_LEAVE, THR, MAX_TURN = (32, 16), 8, 4, 0.02, 7
TORCH_SEED, NUMPY_SEED = 11, 5
RUNS = (("e0", 0.0), ("e3", 0.3))
KEYS = ("ctr", "click_loss", "len_tra", "R_tra")

# ---- the device cases of tests/test_gpu_vtb_static.py (tests/test_vtb_static_cpu.py checks their inputs on the CPU) ------------------
GPU_N_LEAVE, GPU_T, GPU_SEED = 5, 50, 1234
GPU_SHAPES = {"script": dict(dnn=(256, 256), num_experts=4, expert_dim=8, thr=0.4), "odd": dict(dnn=(96,), num_experts=2, expert_dim=5, thr=0.12)}
GPU_CASES = [("script", 100), ("script", 37), ("odd", 100), ("odd", 37)]
GPU_EPS = (0.0, 0.3)


def stress(model, seed=3):
    """Scale the initial weights up the way `_stressed_mmoe` does (the reference's init std of 1e-4 makes every output round-off)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith("dnn.") and name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.15)
            elif name.endswith("weight") and "linear_model" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        for t in model.tower_network:
            t.weight.mul_(0.05)
    return model


def two_task_model(dnn=(256, 256), num_experts=4, expert_dim=8, stressed=True, seed=3):
    """MLP-taobao.py:64-120's model: x = feat_user (91), y = feat_item (27) + y (1)."""
    from core.user_model_mmoe import UserModel_MMOE
    from deepctr_torch.inputs import DenseFeat
    x_columns = [DenseFeat("feat_user", 91)]
    y_columns = [DenseFeat("feat_item", 27)] + [DenseFeat("y", 1)]
    tasks = collections.OrderedDict({f.name: "regression" for f in y_columns})
    model = UserModel_MMOE(x_columns, y_columns, len(tasks), tasks, {f.name: f.dimension for f in y_columns}, num_experts=num_experts,
                           expert_dim=expert_dim, dnn_hidden_units=dnn, seed=2022, device="cpu")
    return (stress(model, seed) if stressed else model).eval()


def forward64(model, x):
    """UserModel_MMOE.forward restated in numpy float64 on the module's own parameters (the module's forward casts its input to fp32)."""
    d = lambda t: t.detach().double().numpy()   # noqa: E731
    x = np.asarray(x, np.float64)
    h = x
    for lin in model.dnn.linears:
        h = np.maximum(h @ d(lin.weight).T + d(lin.bias), 0.0)
    mm = model.mmoe_layer
    ex = (h @ d(mm.expert_network.weight).T + d(mm.expert_network.bias)).reshape(len(x), mm.out_dim, mm.num_experts)
    outs = []
    for i, gate in enumerate(mm.gating_networks):
        z = h @ d(gate.weight).T
        g = np.exp(z - z.max(1, keepdims=True))
        g /= g.sum(1, keepdims=True)
        logit = np.einsum("nde,ne->nd", ex, g) @ d(model.tower_network[i].weight).T
        if model.linear_model_task[i] is not None:
            logit = logit + x @ d(model.linear_model_task[i].weight)
        outs.append(logit + d(model.out[i].bias))
    return np.concatenate(outs, 1)


class Recorder:
    """Stands in for the model AND wraps the env of one test_taobao call: logs (state, action, reward_pred, reward, done) per step."""

    def __init__(self, model, env):
        self.model, self.device, self.y_index = model, model.device, model.y_index
        self.rows = []
        rec = self

        class Env:
            def reset(self):
                rec.state = np.asarray(env.reset(), np.float64).copy()
                return rec.state

            def step(self, action):
                s, r, d, info = env.step(action)
                rec.rows.append((rec.state, np.asarray(action, np.float64).copy(), rec.pred, int(r), bool(d)))
                rec.state = np.asarray(s, np.float64).copy()
                return s, r, d, info

        self.env = Env()

    def __call__(self, x):
        with torch.no_grad():
            res = self.model(x)
        self.pred = float(res.reshape(-1)[self.y_index["y"][0]])
        return res

    def arrays(self):
        return dict(state=np.array([r[0] for r in self.rows]), action=np.array([r[1] for r in self.rows]),
                    reward_pred=np.array([r[2] for r in self.rows]), reward=np.array([r[3] for r in self.rows], np.int64),
                    done=np.array([r[4] for r in self.rows]))


# ---- device runs ------------------------------------------------------------------------------------------------------------------
def fetch_noise(ev, lens):
    """noise[i][t] for every played turn (and turn 0's row carries the trajectory's user draw)"""
    ids = np.repeat(np.arange(len(lens)), lens)
    turns = np.concatenate([np.arange(n) for n in lens])
    flat = ev.noise(ids, turns).cpu().numpy()
    out, k = [], 0
    for n in lens:
        out.append(flat[k:k + n])
        k += n
    return out


def replay_env_side(base, tr, noise, epsilon):
    """Teacher-forced env side: the device's recorded actions and exported noise through the CPU mirror (vtbcase.NoiseVTB in static
    mode).  Exits, lengths, states (last draws, turn column), user draws and epsilon decisions must match exactly (a user draw that
    differs from the mirror's own argmax fails, margin or not); click / second draws run under vtbcase.pick's top-2 margin protocol (a disagreement outside the margin asserts there).  Returns the number of
    draws and of draws excused by the margin."""
    n = len(tr["len"])
    forced0, draws, forced_steps = vtbcase.STATS["forced"], 0, 0
    for i in range(n):
        L = int(tr["len"][i])
        assert 1 <= L <= base.max_turn, (i, L)
        nz = noise[i]
        # event layout of the mirror: [0] = reset (user draw: columns 21..237 of any row), [1 + t] = step t
        rows = np.concatenate([nz[:1, :237], nz[:, :237]], 0)
        m = vtbcase.make_mirrors(base, 1, [rows])[0]
        m.force_user = tr["user"][i]
        s = m.reset()
        assert vtbcase.STATS["forced"] == forced0 + forced_steps, f"trajectory {i}: a user draw differs from the CPU mirror's (they must match exactly)"
        for t in range(L):
            what = f"trajectory {i} turn {t}"
            np.testing.assert_array_equal(np.asarray(s, np.float32), tr["state"][i, t], err_msg=what)
            explore = bool(epsilon > 0 and float(nz[t, 237]) < epsilon)
            assert explore == bool(tr["explore"][i, t]), what
            if explore:
                np.testing.assert_array_equal(tr["action"][i, t], nz[t, 238:265], err_msg=what)
            done_dev = bool(tr["done"][i, t])
            # the second draw shows in the next state; at a done step nothing exposes it
            m.force_ab = (int(tr["reward"][i, t]), None if done_dev else int(tr["state"][i, t + 1, 89]))
            m.force_user = None        # the user the mirror redraws on done is never seen (test_taobao resets)
            s, r, d, _ = m.step(tr["action"][i, t])
            assert bool(d) == done_dev and (t == L - 1) == done_dev, what
            assert int(r) == int(tr["reward"][i, t]), what
        forced_steps = vtbcase.STATS["forced"] - forced0
        draws += 11 + 2 * L - 1        # the draws the device exposes: the user's groups, clicks per turn, the second draw before done
        assert (tr["state"][i, L:] == 0).all() and (tr["action"][i, L:] == 0).all() and not tr["done"][i, L:].any()
    return draws, vtbcase.STATS["forced"] - forced0


def metrics_from_trajectory(tr):
    """The four metrics recomputed in float64 from a trajectory, sums in (trajectory, turn) order, plus (clicks, turns)."""
    clicks = turns = 0
    closs = np.float64(0.0)
    for i, L in enumerate(tr["len"]):
        per = np.float64(0.0)
        for t in range(int(L)):
            per += abs(np.float64(tr["reward_pred"][i, t]) - np.float64(tr["reward"][i, t]))
        closs += per
        clicks += int(tr["reward"][i, :L].sum())
        turns += int(L)
    n = len(tr["len"])
    return {"ctr": clicks / turns, "click_loss": float(closs) / turns, "len_tra": turns / n, "R_tra": clicks / n}, (clicks, turns)
