"""Test-side helpers for the device VirtualTaobao env (cirs_hip/virtualtb.py): the mirror's VirtualTB / SimulatedEnv fed with the
device's counter-based noise.

NoiseVTB overrides the two draw sites of the mirror (environments/VirtualTaobao/virtualTB/envs/virtualTB.py): `_draw_user` takes z and
the 88 group Gumbels, `_user_response` the 21 step Gumbels, from DeviceVirtualTB.noise() for the env's current event, and chooses by
argmax(logit + g) over the mirror's own torch modules.  Where the device's choice is known (`force_*`), a disagreement is accepted only
inside the margin protocol: the CPU gap between its own pick and the device's pick of logit + g is <= 1e-5 * max(1, |logit|); the CPU
side then takes the device's choice (teacher forcing) and the event is counted."""
import collections
import os

import numpy as np
import torch

GROUPS = [(0, 8), (8, 16), (16, 27), (27, 38), (38, 49), (49, 60), (60, 62), (62, 64), (64, 67), (67, 85), (85, 88)]
STATS = {"draws": 0, "forced": 0, "min_gap": float("inf")}


def pick(logits, g, forced=None, what=""):
    """argmax(logits + g) (fp32, ties -> lowest) under the margin protocol against the device's choice `forced`."""
    v = logits.detach().to(torch.float32) + torch.as_tensor(g, dtype=torch.float32)
    i = int(torch.argmax(v))
    STATS["draws"] += 1
    if len(v) > 1:
        top = torch.topk(v, 2).values
        STATS["min_gap"] = min(STATS["min_gap"], float(top[0] - top[1]))
    if forced is None or int(forced) == i:
        return i
    f = int(forced)
    gap = float(v[i] - v[f])
    tol = 1e-5 * max(1.0, abs(float(logits[i])), abs(float(logits[f])))
    assert gap <= tol, f"{what}: device picked {f}, CPU {i}, gap {gap:.3g} > {tol:.3g}"
    STATS["forced"] += 1
    return f


def golden_mmoe(golden_dir):
    from core.user_model_mmoe import UserModel_MMOE
    from deepctr_torch.inputs import DenseFeat
    z = np.load(os.path.join(golden_dir, "virtualtb.npz"))
    x_columns, y_columns = [DenseFeat("user_feat", 91), DenseFeat("feat_item", 27)], [DenseFeat("y", 1)]
    tasks = collections.OrderedDict({f.name: "regression" for f in y_columns})
    model = UserModel_MMOE(x_columns, y_columns, len(tasks), tasks, {f.name: f.dimension for f in y_columns}, dnn_hidden_units=(128, 128),
                           seed=2022, device="cpu")
    model.load_state_dict({k[len("mmoe_"):]: torch.as_tensor(z[k]) for k in z.files if k.startswith("mmoe_") and k not in ("mmoe_x", "mmoe_y")})
    return model.eval(), z


def base_vtb(golden_dir, N=5, thr=3.0, T=50):
    from environments.VirtualTaobao.virtualTB.envs.virtualTB import VirtualTB
    return VirtualTB(num_leave_compute=N, leave_threshold=thr, max_turn=T, data_dir=os.path.join(golden_dir, "virtualtb"))


def _noise_vtb_class():
    from environments.VirtualTaobao.virtualTB.envs.virtualTB import VirtualTB

    class NoiseVTB(VirtualTB):
        def _draw_user(self):
            n = self.noise[self.cur_event]
            with torch.no_grad():
                x = self.generator(torch.from_numpy(n[21:149].copy()).unsqueeze(0))[0]
            g = n[149:]
            one_hot = np.zeros(88, np.float32)
            for gi, (lo, hi) in enumerate(GROUPS):
                f = None if self.force_user is None else int(self.force_user[gi]) - lo
                one_hot[lo + pick(x[lo:hi], g[lo:hi], f, f"user group {gi}")] = 1.0
            return one_hot

        def _user_response(self, action):
            n = self.noise[self.cur_event]
            user = torch.FloatTensor(self.cur_user).unsqueeze(0)
            page = torch.FloatTensor([[self.total_turn]])
            with torch.no_grad():
                x = self.action_model(torch.cat((user, page, torch.FloatTensor(action).unsqueeze(0)), dim=-1))[0]
            a = pick(x[:11], n[:11], self.force_ab[0], "clicks")
            b = pick(x[11:], n[11:21], self.force_ab[1], "second draw")
            return np.array([a, b])

        def reset(self):
            self.cur_event = self.next_event
            self.next_event += 1
            return super().reset()

        def step(self, action):
            self.cur_event = self.next_event
            self.next_event += 1
            return super().step(action)

    return NoiseVTB


def make_mirrors(base, n, noise, user_model=None, version="v1", tau=1.0, gamma_exposure=1.0, use_exposure=True):
    """n noise-fed CPU envs sharing `base`'s modules; noise[i] = DeviceVirtualTB.noise rows of env i, indexed by event."""
    cls = _noise_vtb_class()
    out = []
    for i in range(n):
        m = cls.__new__(cls)
        m.__dict__.update(base.__dict__)
        m.noise, m.next_event, m.force_user, m.force_ab = noise[i], 0, None, (None, None)
        if user_model is None:
            out.append(m)
            continue
        from core.env.simulatedEnv.simulated_env import SimulatedEnv
        s = SimulatedEnv.__new__(SimulatedEnv)
        s.__dict__.update(dict(user_model=user_model, env_task=m, observation_space=m.observation_space, action_space=m.action_space,
                               env_name="VirtualTB-v0", version=version, tau=tau, use_exposure_intervention=use_exposure,
                               alpha_u=None, beta_i=None, normed_mat=None, gamma_exposure=gamma_exposure, r_decay=1,
                               cum_reward=0, total_turn=0))
        s._reset_history()
        out.append(s)
    return out


def inner(env):
    return env.env_task if hasattr(env, "user_model") else env


def fetch_noise(eng, n, events):
    ids = np.repeat(np.arange(n), events)
    ev = np.tile(np.arange(events), n)
    return eng.noise(ids, ev).cpu().numpy().reshape(n, events, -1)
