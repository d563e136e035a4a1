"""VirtualTaobao user model end to end on synthetic data: write a `dataset.txt`-shaped log from the raw device VirtualTB env, train
UserModel_MMOE on the device (the run of CIRS-UserModel-taobao.py), reload the two artefacts the way CIRS-RL-taobao.py does, build the
device SimulatedEnv on the trained model and run one collect.

    python examples/cirs_usermodel_taobao_synth.py [workdir]"""
import os
import pickle
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))
import numpy as np
import torch

from cirs_hip.synthetic import write_virtualtaobao_log
from core.env.simulatedEnv.simulated_env import SimulatedEnv
from core.user_model_mmoe import UserModel_MMOE
from core.user_model_train import train_user_model_taobao
from environments.VirtualTaobao.virtualTB.envs.virtualTB import VirtualTB


def main(workdir):
    log = os.path.join(workdir, "dataset.txt")
    base = VirtualTB(num_leave_compute=5, leave_threshold=4.5, max_turn=50)
    n = write_virtualtaobao_log(log, n_sessions=2000, seed=0, vtb_env=base)
    print(f"log: {n} rows in 2000 sessions -> {log}")
    res = train_user_model_taobao(log, save_root=workdir, dnn=(128, 128), epoch=5, batch_size=100)     # (128, 128): what the device env steps
    print("loss per epoch:", [round(h["loss"], 4) for h in res.history])
    with open(res.paths.params, "rb") as fh:
        params = pickle.load(fh)
    params["device"] = "cpu"
    user_model = UserModel_MMOE(**params)
    user_model.load_state_dict(torch.load(res.paths.state_dict))
    sim = SimulatedEnv.__new__(SimulatedEnv)
    sim.__dict__.update(dict(user_model=user_model.eval(), env_task=base, observation_space=base.observation_space, action_space=base.action_space,
                             env_name="VirtualTB-v0", version="v1", tau=0.01, use_exposure_intervention=True, alpha_u=None, beta_i=None,
                             normed_mat=None, gamma_exposure=1.0, r_decay=1, cum_reward=0, total_turn=0))
    sim._reset_history()
    env = sim.build_device_env(64, device="cuda", seed=1)
    env.reset()
    rng = np.random.RandomState(0)
    total = np.zeros(64)
    for _ in range(10):
        obs, rew, done, ctr = env.step(torch.as_tensor(rng.uniform(-1, 1, (64, 27)).astype(np.float32)))
        total += rew.cpu().numpy()
    print("10 random steps of 64 simulated envs on the trained model: mean predicted reward per step", float(total.mean() / 10))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        with tempfile.TemporaryDirectory() as d:
            main(d)
