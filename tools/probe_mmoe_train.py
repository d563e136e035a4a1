"""Probe: time of one optimiser step of the VirtualTaobao MMoE user model through cirs_mmoe_train_epoch and through
UserModel_MMOE.fit_data, against THE SAME STEP IN PLAIN TORCH (cirs_hip.mmoe_host.torch_train) on the same GPU and on 16 host threads;
and cirs_vtb_exposure_history against the numpy loop.  Warm-up, median of repeats, device events around the epoch call.

    python tools/probe_mmoe_train.py                  -> one JSON line
    python tools/probe_mmoe_train.py --mode device    cirs_mmoe_train_epoch alone (epoch_ms_per_step per shape and batch), for A/B runs
    python tools/probe_mmoe_train.py --kernels-only   a few epochs and one exposure call, for a kernel trace
                                                      (rocprofv3 --kernel-trace --stats -- python tools/probe_mmoe_train.py --kernels-only)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import mmoecase
from cirs_hip import mmoe_host
from cirs_hip.mmoe_train import MMoETrainer, vtb_exposure_history

N = 16384
KERNELS_ONLY = "--kernels-only" in sys.argv
DEVICE_ONLY = sys.argv[1:] == ["--mode", "device"]


def epoch_ms(dnn, bs, repeats=7):
    init = mmoecase.stressed_init(dnn)
    x, y, s = (torch.as_tensor(a, dtype=torch.float32).cuda() for a in mmoecase.inputs(N))
    tr = MMoETrainer(init, l2_linear=mmoecase.L2_LINEAR, l2_all=mmoecase.L2_ALL)
    order = torch.arange(N, device="cuda")
    steps = (N + bs - 1) // bs
    for _ in range(2):
        tr.epoch(x, y, s, order, bs)
    torch.cuda.synchronize()
    if KERNELS_ONLY:
        return None
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); tr.epoch(x, y, s, order, bs); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / steps)
    return statistics.median(ts)


def fit_ms(dnn, bs, repeats=5):
    from core.static_dataset import StaticDataset
    from core.user_model_mmoe import loss_taobao
    m = mmoecase.model(dnn)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in mmoecase.stressed_init(dnn).items()})
    m.compile("adam", loss_func=loss_taobao)
    xc, yc = mmoecase.columns()
    ds = StaticDataset(xc, yc, num_workers=0)
    ds.compile_dataset(*mmoecase.inputs(N))
    m.fit_data(ds, batch_size=bs, epochs=1, shuffle=True)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); m.fit_data(ds, batch_size=bs, epochs=1, shuffle=True); ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts) / ((N + bs - 1) // bs)


def torch_ms(dnn, bs, device, steps, repeats=3):
    init = mmoecase.stressed_init(dnn)
    x, y, s = mmoecase.inputs(N)
    x, y, s = (torch.as_tensor(a, dtype=torch.float32).to(device) for a in (x, y, s))
    p = {k: torch.nn.Parameter(torch.as_tensor(v).to(device)) for k, v in init.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)

    def run(k):
        for st in range(k):
            sl = slice((st * bs) % (N - bs + 1), (st * bs) % (N - bs + 1) + bs)
            loss = mmoe_host.loss_taobao(mmoe_host.forward(p, x[sl]), y[sl].reshape(-1, 1), s[sl].reshape(-1, 1))
            reg = mmoecase.L2_LINEAR * (p["linear_model.weight"] ** 2).sum()
            for v in p.values():
                reg = reg + torch.sum(mmoecase.L2_ALL * v * v)
            opt.zero_grad(); (loss + reg).backward(); opt.step()
        if device != "cpu":
            torch.cuda.synchronize()
    run(5)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); run(steps); ts.append((time.perf_counter() - t0) / steps)
    return 1e3 * statistics.median(ts)


def exposure(n_rows, numpy_rows=10000):
    rng = np.random.RandomState(0)
    ts = (np.arange(n_rows) % 50) + 1                 # sessions of 50 rows
    act = rng.uniform(-1, 1, (n_rows, 27))
    vtb_exposure_history(ts[:1000], act[:1000], 0.01)
    torch.cuda.synchronize()
    if KERNELS_ONLY:
        vtb_exposure_history(ts, act, 0.01); torch.cuda.synchronize()
        return None
    t0 = time.perf_counter(); vtb_exposure_history(ts, act, 0.01); torch.cuda.synchronize(); dev = time.perf_counter() - t0
    t0 = time.perf_counter(); mmoe_host.exposure_virtualtaobao(ts[:numpy_rows], act[:numpy_rows], 0.01); host = time.perf_counter() - t0
    return dict(rows=n_rows, device_s_incl_copies=dev, numpy_s_extrapolated_from=numpy_rows, numpy_s=host * n_rows / numpy_rows)


def main():
    out = {}
    torch.set_num_threads(16)
    for dnn in ((64, 64), (128, 128)):
        for bs in (100, 2048):
            key = f"{dnn[0]}x{dnn[1]}_b{bs}"
            ms = epoch_ms(dnn, bs)
            if KERNELS_ONLY:
                continue
            r = dict(epoch_ms_per_step=ms, epoch_rows_per_s=bs / ms * 1e3)
            if DEVICE_ONLY:
                out[key] = r
                continue
            f = fit_ms(dnn, bs)
            r.update(fit_data_ms_per_step=f, fit_data_rows_per_s=bs / f * 1e3)
            tg = torch_ms(dnn, bs, "cuda", 40)
            tc = torch_ms(dnn, bs, "cpu", 20)
            r.update(torch_gpu_ms_per_step=tg, torch_cpu16_ms_per_step=tc, speedup_vs_torch_gpu=tg / ms, speedup_vs_torch_cpu16=tc / ms)
            out[key] = r
    if DEVICE_ONLY:
        print(json.dumps(out))
        return
    e = exposure(1000000)
    if not KERNELS_ONLY:
        out["exposure"] = e
        print(json.dumps(out))


if __name__ == "__main__":
    main()
