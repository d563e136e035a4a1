"""Generate tests/golden/vtbstatic.npz by running the REFERENCE implementation (development machine only; no test calls this).

Run as `python tools/gen_golden_vtbstatic.py` from the repository root.  Through oracle/ref_harness.py, like
tools/gen_golden_mmoetrain.py:

  the reference's own evaluation.test_taobao (evaluation.py:238-282) on the reference's VirtualTB in static-state mode with the
  reference's two-task UserModel_MMOE built as MLP-taobao.py:64-120 builds it (x: feat_user 91; y: feat_item 27, y 1), its weights
  scaled up the way tests' `_stressed_mmoe` does (the reference initialises the DNN with std 1e-4, where every output is round-off).
  The loop's `num_trajectory = 100` is patched down to N_TRAJ in the function's source; nothing else of it is touched.  Two runs,
  epsilon = 0 and epsilon = 0.3, each from torch.manual_seed / np.random.seed given below, the env constructed after the seeding
  (its constructor draws from torch's generator).

Stored: the model's state dict, per env step the state fed to the model, the action, reward_pred, the reward and done, and the result
dicts.  Only arrays are written."""
import collections
import inspect
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _no_network_get(*args, **kwargs):
    raise OSError("network access is disabled in the fixture generator")


# DeepCTR-Torch starts a version check against the package index when it is imported: give it a `requests` that refuses at once
sys.modules["requests"] = types.SimpleNamespace(get=_no_network_get, codes=types.SimpleNamespace(ok=200))

import ref_harness  # noqa: E402

ref_harness.install()

import torch  # noqa: E402

import vtbstaticcase as case  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _model():
    from core.user_model_mmoe import UserModel_MMOE
    from deepctr_torch.inputs import DenseFeat
    x_columns = [DenseFeat("feat_user", 91)]
    y_columns = [DenseFeat("feat_item", 27)] + [DenseFeat("y", 1)]
    tasks = collections.OrderedDict({f.name: "regression" for f in y_columns})
    model = UserModel_MMOE(x_columns, y_columns, len(tasks), tasks, {f.name: f.dimension for f in y_columns}, num_experts=4, expert_dim=8,
                           dnn_hidden_units=case.DNN, seed=2022, device="cpu")
    case.stress(model)
    return model.eval()


def _test_taobao():
    """evaluation.test_taobao with its trajectory count patched down"""
    import evaluation
    src = inspect.getsource(evaluation.test_taobao)
    assert src.count("num_trajectory = 100") == 1
    ns = dict(vars(evaluation))
    exec(compile(src.replace("num_trajectory = 100", f"num_trajectory = {case.N_TRAJ}"), "test_taobao_patched", "exec"), ns)
    return ns["test_taobao"]


def main():
    from virtualTB.envs.virtualTB import VirtualTB
    model = _model()
    test_taobao = _test_taobao()
    out = {"sd_" + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    out["env_params"] = np.array([case.N_LEAVE, case.THR, case.MAX_TURN], np.float64)
    for tag, eps in case.RUNS:
        torch.manual_seed(case.TORCH_SEED)
        np.random.seed(case.NUMPY_SEED)
        env = VirtualTB(num_leave_compute=case.N_LEAVE, leave_threshold=case.THR, max_turn=case.MAX_TURN)
        env.set_state_mode(True)
        rec = case.Recorder(model, env)
        res = test_taobao(rec, rec.env, eps)
        for k, v in rec.arrays().items():
            out[f"{tag}_{k}"] = v
        out[f"{tag}_result"] = np.array([res[k] for k in case.KEYS], np.float64)
        d = rec.arrays()
        lens = np.diff(np.r_[-1, np.flatnonzero(d["done"])])
        print(tag, "epsilon", eps, res, "lengths", lens.tolist(), "clicks", d["reward"].tolist())
    path = os.path.join(GOLDEN, "vtbstatic.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
