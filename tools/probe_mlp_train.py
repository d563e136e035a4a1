"""Probe: time of one optimiser step of the VirtualTaobao two-task MLP baselines (the script shape of MLP-taobao.py: dnn (256, 256),
batch 100; and batch 2048) through cirs_mlp_train_epoch, against THE SAME STEP IN PLAIN TORCH (cirs_hip.mmoe_host.mlp_forward /
loss_taobao_mlp) on the same GPU and on 16 host threads; and one fit_data epoch including the per-epoch test_taobao(device="cuda") call.
Warm-up, median of 7 epochs, device events around the epoch call.

    python tools/probe_mlp_train.py                  every mode below as a child process of its own under `timeout -k 10`, stopping at
                                                     the first one that fails -> one JSON line
    python tools/probe_mlp_train.py --mode device | torch-gpu | torch-cpu | fit      one mode in this process -> one JSON line
    python tools/probe_mlp_train.py --kernels-only   a few epochs, for a kernel trace in a run of its own
                                                     (rocprofv3 --kernel-trace --stats -- python tools/probe_mlp_train.py --kernels-only)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, DNN, BATCHES = 16384, (256, 256), (100, 2048)
MODES = (("device", 120), ("torch-gpu", 180), ("torch-cpu", 300), ("fit", 180))
KERNELS_ONLY = "--kernels-only" in sys.argv


def _data():
    import mlpcase
    return mlpcase.stressed_init(DNN, scale=mlpcase.dnn_scale(DNN)), mlpcase.inputs(N)


def device():
    import torch
    import mlpcase
    from cirs_hip.mmoe_train import MlpTrainer
    init, (x, y) = _data()
    x, y = (torch.as_tensor(a, dtype=torch.float32).cuda() for a in (x, y))
    order = torch.arange(N, device="cuda")
    out = {}
    for bs in BATCHES:
        tr = MlpTrainer(init, l2_linear=mlpcase.L2_LINEAR, l2_all=mlpcase.L2_ALL)
        steps = (N + bs - 1) // bs
        for _ in range(2):
            tr.epoch(x, y, order, bs)
        torch.cuda.synchronize()
        if KERNELS_ONLY:
            continue
        ts = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); tr.epoch(x, y, order, bs); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / steps)
        ms = statistics.median(ts)
        out[f"b{bs}"] = dict(epoch_ms_per_step=ms, epoch_rows_per_s=bs / ms * 1e3)
    return out


def torch_steps(dev, steps):
    import torch
    import mlpcase
    from cirs_hip import mmoe_host
    torch.set_num_threads(16)
    init, (x, y) = _data()
    x, y = (torch.as_tensor(a, dtype=torch.float32).to(dev) for a in (x, y))
    out = {}
    for bs in BATCHES:
        p = {k: torch.nn.Parameter(torch.as_tensor(v).to(dev)) for k, v in init.items()}
        opt = torch.optim.Adam(list(p.values()), lr=1e-3)

        def run(k):
            for st in range(k):
                s0 = (st * bs) % (N - bs + 1)
                loss = mmoe_host.loss_taobao_mlp(mmoe_host.mlp_forward(p, x[s0:s0 + bs]), y[s0:s0 + bs])
                reg = mlpcase.L2_LINEAR * (p["linear_model.weight"] ** 2).sum()
                for v in p.values():
                    reg = reg + torch.sum(mlpcase.L2_ALL * v * v)
                opt.zero_grad(); (loss + reg).backward(); opt.step()
            if dev != "cpu":
                torch.cuda.synchronize()
        run(5)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); run(steps); ts.append((time.perf_counter() - t0) / steps)
        out[f"b{bs}"] = dict(ms_per_step=1e3 * statistics.median(ts))
    return out


def fit():
    """One fit_data epoch at batch 100 with and without the per-epoch test_taobao(device="cuda") of 100 trajectories."""
    import functools
    import torch
    import mlpcase
    import vtbstaticcase
    from core.static_dataset import StaticDataset
    from core.user_model_mmoe import loss_taobao_mlp
    from environments.VirtualTaobao.virtualTB.envs.virtualTB import VirtualTB
    from evaluation import test_taobao
    init, (x, y) = _data()
    env = VirtualTB(num_leave_compute=5, leave_threshold=1.0, max_turn=50)
    env.set_state_mode(True)
    out = {}
    for with_eval in (False, True):
        m = vtbstaticcase.two_task_model(DNN, stressed=False)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in init.items()})
        m.compile("adam", loss_func=loss_taobao_mlp)
        if with_eval:
            m.compile_RL_test(functools.partial(test_taobao, env=env, device="cuda"))
        ds = StaticDataset(m.feature_columns, m.y_columns, num_workers=0)
        ds.compile_dataset(x, y)
        m.fit_data(ds, batch_size=100, epochs=1, shuffle=True)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter(); m.fit_data(ds, batch_size=100, epochs=1, shuffle=True); ts.append(time.perf_counter() - t0)
        out["epoch_s_with_test_taobao" if with_eval else "epoch_s"] = statistics.median(ts)
    return out


def main():
    if KERNELS_ONLY:
        device()
        return
    if "--mode" in sys.argv:
        mode = sys.argv[sys.argv.index("--mode") + 1]
        res = {"device": device, "torch-gpu": lambda: torch_steps("cuda", 40), "torch-cpu": lambda: torch_steps("cpu", 10), "fit": fit}[mode]()
        print(json.dumps(res))
        return
    out = {}
    for mode, limit in MODES:      # a step that faults or hangs ends the probe: nothing more is started on the GPU after it
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--mode", mode], capture_output=True, text=True)
        if r.returncode != 0:
            print(json.dumps(dict(out, failed=mode, returncode=r.returncode, stderr=r.stderr[-2000:])))
            sys.exit(1)
        out[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    for bs in BATCHES:
        d = out["device"][f"b{bs}"]["epoch_ms_per_step"]
        out[f"speedup_b{bs}"] = dict(vs_torch_gpu=out["torch-gpu"][f"b{bs}"]["ms_per_step"] / d, vs_torch_cpu16=out["torch-cpu"][f"b{bs}"]["ms_per_step"] / d)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
