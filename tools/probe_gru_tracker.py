"""The recurrent state trackers (GRU, LSTM), the pooled-window one (Avg), the convolutional one (Caser), the dilated-convolution one (NextItNet), the
attention-pool one (STAMP), the GRU encoder with attention over its hidden states (NARM), the filter-MLP one (FMLP) and the linear-recurrence one
(LRU) against the Transformer one at the benchmark shapes:
    python tools/probe_gru_tracker.py [--workload c2|c3] [--reps 60]

Thirteen trackers over the same env, policy and learner (bench.py's engine at dropout 0): the Transformer (2 layers), the GRU and the LSTM with 1 and
with 2 layers, the Avg tracker with a window of 3 and of 10, the Caser tracker with a window of 10 and heights (2, 3, 4),
the NextItNet tracker with dilations (1, 2, 4), the STAMP tracker with a window of 10, the NARM tracker (one encoder layer, attention over the whole
session), the FMLP tracker with a window of 10 and 2 layers, the LRU tracker (one linear recurrent unit).  Per tracker, alternated inside every repetition so that drift of the machine hits all alike:
  step_us        one tracker step alone (one launch, all envs) at positions 1, 15 and 30 -- a device-event pair around the launch
  collect_ms     one DeviceRollout.collect (what Collector.collect runs on the device): the fused two-launch sequence for the Transformer,
                 cirs_rollout_collect_gru's / _lstm's / _avg's / _caser's / _nextitnet's / _stamp's / _narm's / _fmlp's / _lru's unfused sequence for the others -- device events around the call, enqueued behind a spin kernel (the host
                 ahead of the device, as in the training loop); collect_idle_ms: the same from an idle stream (the host's launch rate counts)
  bwd_adam_ms    the tracker backward + Adam step of one update (the learner's d loss / d obs as upstream gradient) -- device events
Medians over --reps repetitions after a warm-up, min and max alongside; lstm_over_gru: the ratios of those medians per layer count;
avg_over_gru: the Avg tracker's over the one-layer GRU's, per window; caser_over: the Caser tracker's over the one-layer GRU's and over the Avg tracker's at
the same window (the two step kernels share everything except the window arithmetic); nextitnet_over: the NextItNet tracker's over the Caser tracker's and
over the one-layer GRU's; stamp_over: the STAMP tracker's over the Avg tracker's and over the Caser tracker's at the same window (the yardsticks on either
side of it); narm_over: the NARM tracker's over the one-layer GRU's (its encoder alone) and over the STAMP tracker's, with the step at positions 1, 15
and 30 (its attention term grows with the position); fmlp_over: the FMLP tracker's over the NextItNet, the Caser and the Transformer tracker's (the
other dense-tile trackers and the model it is the ablation partner of), with the step at positions 1, 15 and 30; lru_over: the LRU tracker's over
the one-layer GRU's, the NARM and the Transformer tracker's (the carried-state trackers and the model whose KV cache it does without), with the step at
positions 1, 15 and 30 (its step should not depend on the position).  One JSON line.
--trace: no timing, a few collects and backwards per tracker -- the run to put under `rocprofv3 --kernel-trace --stats -- python ...` for kernel times
(tracing slows the host: never in the same run as the timings above)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from cirs_hip.avg_tracker import DeviceAvgTracker, avg_param_shapes, init_avg_tracker_params  # noqa: E402
from cirs_hip.caser_tracker import DeviceCaserTracker, caser_param_shapes, init_caser_tracker_params  # noqa: E402
from cirs_hip.fmlp_tracker import DeviceFmlpTracker, fmlp_param_shapes, init_fmlp_tracker_params  # noqa: E402
from cirs_hip.gru_tracker import DeviceGruTracker, gru_param_shapes, init_gru_tracker_params  # noqa: E402
from cirs_hip.lru_tracker import DeviceLruTracker, init_lru_tracker_params, lru_param_shapes  # noqa: E402
from cirs_hip.lstm_tracker import DeviceLstmTracker, init_lstm_tracker_params, lstm_param_shapes  # noqa: E402
from cirs_hip.narm_tracker import DeviceNarmTracker, init_narm_tracker_params, narm_param_shapes  # noqa: E402
from cirs_hip.nextitnet_tracker import DeviceNextItNetTracker, init_nextitnet_tracker_params, nextitnet_param_shapes  # noqa: E402
from cirs_hip.rollout import DeviceRollout  # noqa: E402
from cirs_hip.stamp_tracker import DeviceStampTracker, init_stamp_tracker_params, stamp_param_shapes  # noqa: E402
from cirs_hip.tracker import flat_tracker_params  # noqa: E402


CELLS = {"gru": (DeviceGruTracker, gru_param_shapes, init_gru_tracker_params), "lstm": (DeviceLstmTracker, lstm_param_shapes, init_lstm_tracker_params)}


def recurrent_engine(cell, wl, layers, device):
    engine, shapes, init = CELLS[cell]
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(shapes(U, I, 32, 20, layers), device=device, init=init(U, I, seed=2023, nlayers=layers))
    trk = engine(dict(views), U, I, B, T, nlayers=layers, device=device)
    trk.enable_training(flat)
    return trk


def avg_engine(wl, window, device):
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(avg_param_shapes(U, I, 32, 20), device=device, init=init_avg_tracker_params(U, I, seed=2023))
    trk = DeviceAvgTracker(dict(views), U, I, B, T, window_size=window, device=device)
    trk.enable_training(flat)
    return trk


def caser_engine(wl, window, heights, device):
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(caser_param_shapes(U, I, 32, 20, window, heights), device=device,
                                      init=init_caser_tracker_params(U, I, seed=2023, window_size=window, filter_sizes=heights))
    trk = DeviceCaserTracker(dict(views), U, I, B, T, window_size=window, filter_sizes=heights, device=device)
    trk.enable_training(flat)
    return trk


def nextitnet_engine(wl, dilations, device):
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(nextitnet_param_shapes(U, I, 32, 20, dilations), device=device,
                                      init=init_nextitnet_tracker_params(U, I, seed=2023, dilations=dilations))
    trk = DeviceNextItNetTracker(dict(views), U, I, B, T, dilations=dilations, device=device)
    trk.enable_training(flat)
    return trk


def stamp_engine(wl, window, device):
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(stamp_param_shapes(U, I, 32, 20), device=device, init=init_stamp_tracker_params(U, I, seed=2023))
    trk = DeviceStampTracker(dict(views), U, I, B, T, window_size=window, device=device)
    trk.enable_training(flat)
    return trk


def narm_engine(wl, device):
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(narm_param_shapes(U, I, 32, 20), device=device, init=init_narm_tracker_params(U, I, seed=2023))
    trk = DeviceNarmTracker(dict(views), U, I, B, T, device=device)
    trk.enable_training(flat)
    return trk


def fmlp_engine(wl, window, layers, device):
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(fmlp_param_shapes(U, I, 32, 20, window, layers), device=device,
                                      init=init_fmlp_tracker_params(U, I, seed=2023, window_size=window, nlayers=layers))
    trk = DeviceFmlpTracker(dict(views), U, I, B, T, window_size=window, nlayers=layers, device=device)
    trk.enable_training(flat)
    return trk


def lru_engine(wl, device):
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    flat, views = flat_tracker_params(lru_param_shapes(U, I, 32, 20), device=device, init=init_lru_tracker_params(U, I, seed=2023))
    trk = DeviceLruTracker(dict(views), U, I, B, T, device=device)
    trk.enable_training(flat)
    return trk


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


def timed(fn, queued=True):
    """device time of what fn enqueues.  queued: behind a spin kernel, so that the host has enqueued everything before the first event fires --
    the gaps between the launches are then the device's, not the host's (the state of the training loop, whose host runs an update ahead)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if queued:
        torch.cuda._sleep(1000000)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on an MI355X: no CPU fallback"
    assert args.trace or args.reps >= 50, "at least 50 repetitions"
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS[args.workload]
    U, I, B, T = wl["U"], wl["I"], wl["B"], wl["T"]
    eng, _ = bench.build_engine(wl, 0, 1, device, dropout=0.0)
    ln = eng.learner
    variants = {"transformer_l2": (eng.tracker, eng.rollout)}
    for cell in CELLS:
        for layers in (1, 2):
            trk = recurrent_engine(cell, wl, layers, device)
            variants[f"{cell}_l{layers}"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    for window in (3, 10):
        trk = avg_engine(wl, window, device)
        variants[f"avg_w{window}"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    trk = caser_engine(wl, 10, (2, 3, 4), device)
    variants["caser_w10"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    trk = nextitnet_engine(wl, (1, 2, 4), device)
    variants["nextitnet_d124"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    trk = stamp_engine(wl, 10, device)
    variants["stamp_w10"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    trk = narm_engine(wl, device)
    variants["narm"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    trk = fmlp_engine(wl, 10, 2, device)
    variants["fmlp_w10_l2"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    trk = lru_engine(wl, device)
    variants["lru"] = (trk, DeviceRollout(eng.env, trk, eng.policy))
    users = torch.as_tensor(np.random.RandomState(0).randint(0, U, B)).to(device, torch.int32)
    items = torch.as_tensor(np.random.RandomState(1).randint(0, I, B)).to(device)
    rews = torch.rand(B, dtype=torch.float64, device=device)
    state = torch.empty((B, 20), device=device)
    for trk, _ in variants.values():
        trk.reserve_backward(B * T)

    def collect(name):
        trk, ro = variants[name]
        return ro.collect(users, seed=2023 << 8, rng_base=0)

    def prepare_update(name):
        """the learner's pass over this tracker's buffer: leaves d loss / d obs in ln.dobs; the policy is restored so that every tracker meets the same one"""
        trk, ro = variants[name]
        lens = collect(name).cpu().numpy().astype(np.int32)
        keep = eng.policy_flat.clone()
        n = ln.prepare(ro.traj, lens)
        ln.learn(1024, 2, want_tracker_grad=True)
        eng.policy_flat.copy_(keep)
        offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
        return dict(lens=lens, n=n, offsets=torch.as_tensor(offsets).to(device), lens_d=torch.as_tensor(lens).to(device), dobs=ln.dobs.clone(),
                    b_env=ln.b_env.clone(), b_t=ln.b_t.clone(), params=trk.flat.clone())

    def bwd_adam(name, u):
        trk, ro = variants[name]
        trk.backward(users, ro.traj, u["b_env"], u["b_t"], u["offsets"], u["lens_d"], u["n"], u["dobs"])
        trk.adam_update()

    def step_at(name, pos):
        trk, _ = variants[name]
        trk.len.fill_(pos)
        return timed(lambda: trk.step(items, rews, out=state, out_stride=20)) * 1e3

    if args.trace:
        for name in variants:
            u = prepare_update(name)
            for _ in range(5):
                collect(name)
                bwd_adam(name, u)
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, "workload": args.workload, "trackers": list(variants)}), flush=True)
        return
    # the update inputs of every tracker: its own collect's buffer (the trajectories differ: different states -> different actions)
    ups = {name: prepare_update(name) for name in variants}
    out = {"workload": args.workload, "n_env": B, "n_users": U, "n_items": I, "max_turn": T, "reps": args.reps, "warmup": args.warmup, "trackers": {}}
    acc = {name: {"step_us": {p: [] for p in (1, 15, 30)}, "collect_ms": [], "collect_idle_ms": [], "bwd_adam_ms": []} for name in variants}
    for rep in range(args.warmup + args.reps):
        for name in variants:      # alternated: one measurement of every kind per tracker per repetition
            trk, ro = variants[name]
            row = {p: step_at(name, p) for p in (1, 15, 30)}
            c = timed(lambda: collect(name))
            ci = timed(lambda: collect(name), queued=False)      # from an idle stream: the host's launch rate counts
            # the collect overwrote the slots with the same episodes (same users, seed, parameters restored below): the stored update inputs still describe them
            b = timed(lambda: bwd_adam(name, ups[name]))
            trk.flat.copy_(ups[name]["params"])      # undo the Adam step: every repetition runs the same episodes
            if rep >= args.warmup:
                for p in row:
                    acc[name]["step_us"][p].append(row[p])
                acc[name]["collect_ms"].append(c)
                acc[name]["collect_idle_ms"].append(ci)
                acc[name]["bwd_adam_ms"].append(b)
    for name in variants:
        a = acc[name]
        out["trackers"][name] = {"rows": int(ups[name]["n"]), "mean_len": round(float(ups[name]["lens"].mean()), 2),
                                 "step_us": {str(p): stats(v) for p, v in a["step_us"].items()}, "collect_ms": stats(a["collect_ms"]), "collect_idle_ms": stats(a["collect_idle_ms"]),
                                 "bwd_adam_ms": stats(a["bwd_adam_ms"])}
    med = lambda name, key: out["trackers"][name][key]["median"]  # noqa: E731
    out["lstm_over_gru"] = {f"l{l}": {"step_us_30": round(out["trackers"][f"lstm_l{l}"]["step_us"]["30"]["median"] / out["trackers"][f"gru_l{l}"]["step_us"]["30"]["median"], 3),
                                      "collect_ms": round(med(f"lstm_l{l}", "collect_ms") / med(f"gru_l{l}", "collect_ms"), 3),
                                      "bwd_adam_ms": round(med(f"lstm_l{l}", "bwd_adam_ms") / med(f"gru_l{l}", "bwd_adam_ms"), 3)} for l in (1, 2)}
    out["avg_over_gru"] = {f"w{w}": {"step_us_30": round(out["trackers"][f"avg_w{w}"]["step_us"]["30"]["median"] / out["trackers"]["gru_l1"]["step_us"]["30"]["median"], 3),
                                     "collect_ms": round(med(f"avg_w{w}", "collect_ms") / med("gru_l1", "collect_ms"), 3),
                                     "bwd_adam_ms": round(med(f"avg_w{w}", "bwd_adam_ms") / med("gru_l1", "bwd_adam_ms"), 3)} for w in (3, 10)}
    out["caser_over"] = {base: {"step_us_30": round(out["trackers"]["caser_w10"]["step_us"]["30"]["median"] / out["trackers"][base]["step_us"]["30"]["median"], 3),
                                "collect_ms": round(med("caser_w10", "collect_ms") / med(base, "collect_ms"), 3),
                                "bwd_adam_ms": round(med("caser_w10", "bwd_adam_ms") / med(base, "bwd_adam_ms"), 3)} for base in ("gru_l1", "avg_w10")}
    out["nextitnet_over"] = {base: {"step_us_30": round(out["trackers"]["nextitnet_d124"]["step_us"]["30"]["median"] / out["trackers"][base]["step_us"]["30"]["median"], 3),
                                    "collect_ms": round(med("nextitnet_d124", "collect_ms") / med(base, "collect_ms"), 3),
                                    "bwd_adam_ms": round(med("nextitnet_d124", "bwd_adam_ms") / med(base, "bwd_adam_ms"), 3)} for base in ("caser_w10", "gru_l1")}
    out["stamp_over"] = {base: {"step_us_30": round(out["trackers"]["stamp_w10"]["step_us"]["30"]["median"] / out["trackers"][base]["step_us"]["30"]["median"], 3),
                                "collect_ms": round(med("stamp_w10", "collect_ms") / med(base, "collect_ms"), 3),
                                "bwd_adam_ms": round(med("stamp_w10", "bwd_adam_ms") / med(base, "bwd_adam_ms"), 3)} for base in ("avg_w10", "caser_w10")}
    out["narm_over"] = {base: {**{f"step_us_{p}": round(out["trackers"]["narm"]["step_us"][str(p)]["median"] / out["trackers"][base]["step_us"][str(p)]["median"], 3)
                                  for p in (1, 15, 30)},
                               "collect_ms": round(med("narm", "collect_ms") / med(base, "collect_ms"), 3),
                               "bwd_adam_ms": round(med("narm", "bwd_adam_ms") / med(base, "bwd_adam_ms"), 3)} for base in ("gru_l1", "stamp_w10")}
    out["fmlp_over"] = {base: {**{f"step_us_{p}": round(out["trackers"]["fmlp_w10_l2"]["step_us"][str(p)]["median"] / out["trackers"][base]["step_us"][str(p)]["median"], 3)
                                  for p in (1, 15, 30)},
                               "collect_ms": round(med("fmlp_w10_l2", "collect_ms") / med(base, "collect_ms"), 3),
                               "bwd_adam_ms": round(med("fmlp_w10_l2", "bwd_adam_ms") / med(base, "bwd_adam_ms"), 3)}
                        for base in ("nextitnet_d124", "caser_w10", "transformer_l2")}
    out["lru_over"] = {base: {**{f"step_us_{p}": round(out["trackers"]["lru"]["step_us"][str(p)]["median"] / out["trackers"][base]["step_us"][str(p)]["median"], 3)
                                 for p in (1, 15, 30)},
                              "collect_ms": round(med("lru", "collect_ms") / med(base, "collect_ms"), 3),
                              "bwd_adam_ms": round(med("lru", "bwd_adam_ms") / med(base, "bwd_adam_ms"), 3)}
                       for base in ("gru_l1", "narm", "transformer_l2")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
