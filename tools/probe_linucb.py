"""Time the four LinUCB device operations (csrc/linucb.hip) at the KuaishouEnv shape: 3327 arms, d = 7.

    python tools/probe_linucb.py [--rows 2000000] [--val_rows 4694000] [--users 200] [--repeat 20] [--out FILE.json]

A synthetic log (user ids below 7176, raw photo ids below 10728, rows per arm falling like a power law: skewed arm sizes are the normal
case and the longest arm sets the accumulation's time) is made resident once.  Every operation is warmed up three times and then timed
`repeat` times with device events around the call; the medians and the spread (min, max) go to stdout as one JSON line (and into
--out, if given).  What is timed: one epoch of update (the grouping plan built once, as linucb_trainer does), solve over all arms and
over one dirty arm, score for `users` trajectory users (test_kuaishou) and for one (recommend_k_item), predict over a validation set.
No GPU: the probe fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cirs-codes_amd"))


def timed(fn, repeat, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "repeat": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", type=int, default=3327)
    ap.add_argument("--d", type=int, default=7)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--val_rows", type=int, default=4_694_000)       # 1411 users x 3327 items
    ap.add_argument("--users", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe times the device: it needs a GPU"
    from cirs_hip.linucb import DeviceLinUCB
    K, d = args.arms, args.d
    rng = np.random.RandomState(0)
    w = 1.0 / np.arange(1, K + 1) ** 0.8
    arm = rng.choice(K, args.rows, p=w[rng.permutation(K)] / w.sum()).astype(np.int64)
    arm[rng.uniform(size=args.rows) < 0.3] = -1                       # rows of items outside the env
    classes = np.sort(rng.choice(10728, K, replace=False))
    feats = np.c_[rng.randint(0, 32, (K, d - 3)), rng.uniform(2, 60, K)].astype(np.float64)
    dev = torch.device("cuda")

    def log(n, arm_of_row):
        a = np.maximum(arm_of_row, 0)
        x = np.concatenate([rng.randint(0, 7176, (n, 1)).astype(np.float64), classes[a][:, None].astype(np.float64), feats[a]], axis=1)
        return torch.as_tensor(x).to(dev), torch.as_tensor(rng.uniform(0, 5, n)).to(dev), torch.as_tensor(arm_of_row).to(dev)
    x, y, arm_t = log(args.rows, arm)
    val_arm = rng.randint(-1, K, args.val_rows).astype(np.int64)
    vx, _, varm_t = log(args.val_rows, val_arm)
    state = DeviceLinUCB(K, d, 0.25)
    plan = state.plan(arm_t)
    count = np.bincount(arm[arm >= 0], minlength=K)
    users = torch.as_tensor(rng.randint(0, 7176, args.users).astype(np.float64)).to(dev)
    feats_t = torch.as_tensor(feats).to(dev)
    res = {"arms": K, "d": d, "rows": args.rows, "rows_with_an_arm": int(count.sum()), "longest_arm": int(count.max()),
           "median_arm": int(np.median(count)), "val_rows": args.val_rows, "users": args.users, "device": torch.cuda.get_device_name(0)}
    res["plan_ms (sort by arm, once per log)"] = timed(lambda: state.plan(arm_t), args.repeat)
    res["update_epoch"] = timed(lambda: state.update(x, y, plan=plan), args.repeat)

    def solve_all():
        state._dirty_all = True
        state.solve()

    def solve_one():
        state._dirty.add(17)
        state.solve()
    res["solve_all_arms"] = timed(solve_all, args.repeat)
    res["solve_one_dirty_arm"] = timed(solve_one, args.repeat)
    res[f"score_{args.users}_users"] = timed(lambda: state.score(users, feats_t), args.repeat)
    res["score_1_user"] = timed(lambda: state.score(users[:1], feats_t), args.repeat)
    res["score_1_user_full_outputs"] = timed(lambda: state.score(users[:1], feats_t, want_full=True), args.repeat)
    res["predict_val_rows"] = timed(lambda: state.predict(vx, varm_t), args.repeat)
    import time
    A = state.A.cpu().numpy()
    t0 = time.perf_counter()
    np.linalg.inv(A)
    res["host_numpy_batched_inv_all_arms_ms (one call, for scale)"] = (time.perf_counter() - t0) * 1e3
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
