"""Scratch probe: throughput of cirs_deepfm_train_step at the shipped model's shape (7176 x 10729, E = 16), batch 2048, and the
torch-fp32 restatement of the same step on the host cores for comparison.

--epoch    per optimiser step over a resident data set of 50 batches: (a) the per-step route fit_data took before the whole-pass
           entry (torch gathers x[idx], y[idx], score[idx] + step()), (b) epoch() for the pairwise loss, (c) epoch() for the IPS and
           PD losses; each the median of 5 timed passes after one warm-up pass.
--scores   ips_scores / popularity_scores on a 10^6-row synthetic log against the reference's pandas `map` formulation on the host.
--dice     per optimiser step of the DICE baseline over a resident data set of 50 batches: DiceTrainer.epoch() against the same steps
           in plain torch on the same GPU (the loop of dice_host.torch_train on device tensors: autograd + torch.optim.Adam, parameters and
           optimiser built once outside the timed passes, losses kept on the device); each the median of 5 timed passes after one warm-up pass, device first and torch second, then both once more.
--validate one evaluate_data (mae, mse) over the scripts' validation set, the whole small matrix 1411 x 3327 = 4.69 M rows, for the pairwise
           DeepFM and DICE: (a) the per-row forward entry over all rows in one call + a torch float64 reduction of the predictions, (b) the
           reference-shaped loop, 2048 rows per forward call with a read-back each, metrics on the host, (c) the fused call
           (cirs_*_validate, sums read back); wall-clock medians after one warm-up pass (5 passes; 3 for (b)), in the order a, c, b, then a
           and c once more; and the fused launch pair's time from device events (median of 20)."""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, torch
from cirs_hip.deepfm_train import DeepFMTrainer, layout

U, I, F, E, n = 7176, 10729, 32, 16, int(sys.argv[1]) if len(sys.argv) > 1 else 2048
rng = np.random.RandomState(0)
init = {name: rng.normal(0, 0.05, shape).astype(np.float32) for name, shape in layout(U, I, F, E)}
init["embedding_dict.feat.weight"][0] = 0
steps = 50
N = n * steps
col = lambda v: np.asarray(v, np.float64)[:, None]
feats = lambda: np.where(np.arange(4)[None, :] < rng.randint(1, 5, N)[:, None], rng.randint(1, F, (N, 4)), 0)
u = rng.randint(0, U, N)
x = np.concatenate([col(u), col(rng.randint(0, I, N)), feats(), col(rng.uniform(2, 60, N)), col(u), col(rng.randint(0, I, N)), feats(), col(rng.uniform(2, 60, N))], axis=1)
y = rng.uniform(0, 5, (N, 1)); score = rng.gamma(1.0, 0.5, (N, 1))
tr = DeepFMTrainer(init, use_ab=True, lambda_ab=10.0)
xd, yd, sd = torch.as_tensor(x, dtype=torch.float32).cuda(), torch.as_tensor(y, dtype=torch.float32).cuda(), torch.as_tensor(score, dtype=torch.float32).cuda()
for st in range(5):
    tr.step(xd[st * n:(st + 1) * n], yd[st * n:(st + 1) * n], sd[st * n:(st + 1) * n])
torch.cuda.synchronize()
t0 = time.perf_counter()
for st in range(steps):
    tr.step(xd[st * n:(st + 1) * n], yd[st * n:(st + 1) * n], sd[st * n:(st + 1) * n])
torch.cuda.synchronize()
t = (time.perf_counter() - t0) / steps
out = dict(batch=n, us_per_step=1e6 * t, samples_per_s=n / t)
if "--cpu" in sys.argv:
    import nn_oracle
    torch.set_num_threads(16)
    t0 = time.perf_counter()
    nn_oracle.deepfm_train(init, x[:5 * n], y[:5 * n], score[:5 * n], n, 5, True, 10.0)
    tc = (time.perf_counter() - t0) / 5
    out.update(cpu_us_per_step=1e6 * tc, cpu_samples_per_s=n / tc, cpu_threads=16)
if "--epoch" in sys.argv:
    def med(fn, reps=5):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / steps)
        return 1e6 * float(np.median(ts))
    order = torch.randperm(N, device="cuda")

    def old_route():
        for s0 in range(0, N, n):
            idx = order[s0:s0 + n]
            tr.step(xd[idx], yd[idx], sd[idx])
    out["a_gather_step_us"] = med(old_route)
    tr.load(xd, yd, sd)
    out["b_epoch_pairwise_us"] = med(lambda: tr.epoch(order, n, check=False))
    no_ab = {k: v for k, v in init.items() if not k.startswith("ab_")}
    for kind in ("ips", "pd"):
        tk = DeepFMTrainer(no_ab, use_ab=False, loss_kind=kind)
        tk.load(xd, yd, sd.clamp(0.05, 1.0))
        out[f"c_epoch_{kind}_us"] = med(lambda: tk.epoch(order, n, check=False))
if "--scores" in sys.argv:
    import collections
    import pandas as pd
    from cirs_hip.dataprep import ips_scores, popularity_scores
    rows, items = 1_000_000, 10729
    photo = np.minimum(rng.zipf(1.2, rows) - 1, items - 1).astype(np.int64)
    ts = 1.6e9 + np.sort(rng.uniform(0, 5e6, rows))

    def host_ips():
        cnt = collections.Counter(photo.tolist())
        v = pd.Series(photo).map(lambda p: cnt[p])
        v[v < 1] = 1
        return (1.0 / v).to_numpy()[:, None]

    def host_pd(gamma=0.1, num_bin=5):
        t = pd.Series(ts); ph = pd.Series(photo)
        interval = (t.max() - t.min()) / num_bin
        pop = np.zeros((rows, 1))
        for i in range(num_bin):
            lo, hi = interval * i + t.min(), interval * (i + 1) + t.min()
            index = (lo <= t) & ((t < hi) if i < num_bin - 1 else (t <= hi))
            cnt = collections.Counter(ph[index].tolist()); total = sum(cnt.values())
            pop[index] = ph[index].map(lambda p: cnt[p] / total).to_frame()
        return pop ** gamma
    for name, dev_fn, host_fn in (("ips", lambda: ips_scores(photo), host_ips), ("pd", lambda: popularity_scores(photo, ts, 0.1), host_pd)):
        dev_fn(); torch.cuda.synchronize()
        t0 = time.perf_counter(); got = dev_fn(); torch.cuda.synchronize(); td = time.perf_counter() - t0
        t0 = time.perf_counter(); want = host_fn(); th = time.perf_counter() - t0
        out[f"scores_{name}_device_ms"] = 1e3 * td; out[f"scores_{name}_host_map_ms"] = 1e3 * th
        out[f"scores_{name}_equal"] = bool(np.array_equal(got, want))
if "--dice" in sys.argv:
    from cirs_hip import dice_host, dice_train
    dinit = {name: rng.normal(0, 0.05, shape).astype(np.float32) for name, shape in dice_train.layout(U, I, F, E)}
    dinit["embedding_dict.feat.weight"][0] = 0
    x16 = np.concatenate([col(rng.randint(0, U, N)), col(rng.randint(0, U, N)), col(rng.randint(0, I, N)), col(rng.randint(0, I, N)), feats(),
                          col(rng.uniform(2, 60, N)), col(rng.randint(0, I, N)), col(rng.randint(0, I, N)), feats(), col(rng.uniform(2, 60, N))], axis=1)
    s16 = np.where(rng.uniform(size=(N, 1)) < 0.5, 1.0, -1.0)
    x16d, s16d = torch.as_tensor(x16, dtype=torch.float32).cuda(), torch.as_tensor(s16, dtype=torch.float32).cuda()
    order = torch.randperm(N, device="cuda")
    td = dice_train.DiceTrainer(dinit)
    td.load(x16d, yd, s16d)
    # plain torch on the same GPU: parameters, torch.optim.Adam and the order live outside the timed region, like the device trainer's; the
    # timed pass is the statements of dice_host.torch_train's loop, the per-step losses kept on the device
    tp = {k: torch.as_tensor(v).cuda().requires_grad_(True) for k, v in dinit.items()}
    topt = torch.optim.Adam(list(tp.values()), lr=1e-3)
    y1, s1, feat = yd.reshape(-1), s16d.reshape(-1), "embedding_dict.feat.weight"

    def torch_fn():
        losses = []
        for s0 in range(0, N, n):
            idx = order[s0:s0 + n]
            terms = dice_host.get_loss(tp, x16d[idx], y1[idx], s1[idx])
            loss = terms[0] + terms[1] + terms[2] + terms[3]
            reg = dice_host.regulariser(tp)
            topt.zero_grad()
            (loss + reg).backward()
            tp[feat].grad[0] = 2 * (0.1 + 1e-5) * tp[feat].detach()[0]
            topt.step()
            losses.append(torch.stack([v.detach() for v in (loss,) + terms + (reg,)]))
        return torch.stack(losses)

    def med(fn, reps=5):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / steps)
        return 1e6 * float(np.median(ts))
    dev_fn = lambda: td.epoch(order, n, check=False)
    d1, t1 = med(dev_fn), med(torch_fn)
    d2, t2 = med(dev_fn), med(torch_fn)
    out.update(dice_epoch_us=min(d1, d2), dice_torch_us=min(t1, t2), dice_epoch_us_runs=[d1, d2], dice_torch_us_runs=[t1, t2],
               dice_speedup=min(t1, t2) / min(d1, d2))
if "--validate" in sys.argv:
    from cirs_hip import dice_train
    from cirs_hip.deepfm import DeviceDeepFM
    from cirs_hip.userval import ValSet
    NU, NI = 1411, 3327
    NV = NU * NI
    vu, vi = np.repeat(rng.randint(0, U, NU), NI), np.tile(rng.randint(0, I, NI), NU)
    vfeat = np.tile(np.where(np.arange(4)[None, :] < rng.randint(1, 5, NI)[:, None], rng.randint(1, F, (NI, 4)), 0), (NU, 1))
    xv = np.concatenate([col(vu), col(vi), vfeat, col(np.tile(rng.uniform(2, 60, NI), NU))], axis=1)
    yv = rng.uniform(0, 5, (NV, 1))
    dinit = {name: rng.normal(0, 0.05, shape).astype(np.float32) for name, shape in dice_train.layout(U, I, F, E)}
    dinit["embedding_dict.feat.weight"][0] = 0

    def wall(fn, reps):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts))
    for tag, dm in (("pairwise", DeviceDeepFM(init)), ("dice", dice_train.DeviceDice(dinit))):
        vs = ValSet(xv, yv, dm.cfg, dm.device)

        def per_row():
            e = dm.forward(vs.uid, vs.pid, vs.feats, vs.dur).double() - vs.y
            return float(e.abs().sum().cpu()) / NV, float((e * e).sum().cpu()) / NV

        def batched():
            preds = [dm.forward(vs.uid[s0:s0 + 2048], vs.pid[s0:s0 + 2048], vs.feats[s0:s0 + 2048], vs.dur[s0:s0 + 2048]).cpu().numpy()
                     for s0 in range(0, NV, 2048)]
            e = np.concatenate(preds).astype("float64") - yv[:, 0]
            return np.abs(e).mean(), (e * e).mean()

        def fused():
            s = dm.validate(vs)[1].cpu().numpy()
            return s[0] / NV, s[1] / NV
        a1, c1, b1 = wall(per_row, 5), wall(fused, 5), wall(batched, 3)
        a2, c2 = wall(per_row, 5), wall(fused, 5)
        ev = []
        for _ in range(21):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dm.validate(vs); e1.record(); torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        ra, rc = per_row(), fused()
        out[f"validate_{tag}"] = dict(rows=NV, a_per_row_ms=min(a1, a2), b_batched_loop_ms=b1, c_fused_ms=min(c1, c2), a_runs=[a1, a2], c_runs=[c1, c2],
                                      fused_kernel_ms=float(np.median(ev[1:])), speedup_vs_a=min(a1, a2) / min(c1, c2),
                                      metrics_agree=bool(np.allclose(ra, rc, rtol=1e-6)))
print(json.dumps(out))
