"""Bits and launch sequences of the PPO minibatch-step paths under one library build, for A/B runs of two builds that must compute the same
(a change to the host code of csrc/ppo.hip; tools/build_rev.sh builds the library of a git revision, CIRS_HIP_LIB selects a build).

  CIRS_HIP_LIB=<lib> python tools/ab_step_bits.py run <out.pt>            every case below, each result tensor saved with torch.save
  CIRS_HIP_LIB=<lib> rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python tools/ab_step_bits.py run - --trace
                                                                          only the plain-learn and the first TP case, nothing saved
  python tools/ab_step_bits.py compare <a.pt> <b.pt> <trace dir a> <trace dir b> <out.txt>      exit status 1 on any difference

Cases (losses, parameters, adam_m, adam_v and d loss / d obs of every rank): learn_tp with two thread ranks at I = 512, B = 40, T = 12, batch 64, two
repeats, ent_coef 0 and 0.01, each also with CIRS_PPO_HEAD_RECOMPUTE=1; a two-rank learn_dp chain and a plain learn at I = 180, B = 24, T = 30,
batch 70 (a merged last minibatch, a partial last item tile), the chain also with CIRS_PPO_ROWS_KERNEL=0, the plain learn also with
CIRS_PPO_ROWS_KERNEL=0, CIRS_PPO_MERGE_KERNEL=1 and CIRS_PPO_LEARN_PREFETCH=0."""
import csv
import glob
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cirs-codes_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch

from cirs_hip import abi
from cirs_hip.rollout import Trajectory
from test_gpu_engine_dp import FakeCollectives                      # thread stand-ins of the collectives
from test_gpu_learn import _random_case, make_learner, rollout_time_value_logp, upload_traj

SWITCHES = ("CIRS_PPO_MERGE_KERNEL", "CIRS_PPO_HEAD_RECOMPUTE", "CIRS_PPO_ROWS_KERNEL", "CIRS_PPO_TEST_DROP_ARRIVAL", "CIRS_PPO_LEARN_PREFETCH")


def case_data(I, B, T, seed):
    pp, lens, acts, rews, dones, obs, n, rng = _random_case(I, B, T, seed)
    value, logp = rollout_time_value_logp(pp, obs, acts, lens)
    traj = Trajectory(B, T, 20, "cuda")
    upload_traj(traj, acts, rews, dones, lens, obs, value, logp)
    return pp, lens, [rng.permutation(n) for _ in range(2)], traj, n


def make(pp, I, B, T, ent):
    return make_learner(pp, I, B, T, [0.95, 0.95, 0.2, 0.25, ent, 0.5, 1e-3, 0, 0])[0]


def dump(out, tag, ln, losses):
    torch.cuda.synchronize()
    ln.check_handoffs()
    for k, t in (("losses", losses), ("params", ln.params), ("adam_m", ln.adam_m), ("adam_v", ln.adam_v), ("dobs", ln.dobs)):
        out[f"{tag}/{k}"] = t.detach().cpu().clone()


def set_env(**kw):
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in kw.items():
        os.environ[k] = v


def run_ranks(W, fn):
    fake = FakeCollectives(W)
    res = [None] * W

    def run(r):
        try:
            fake.local.rank = r
            res[r] = fn(r, fake)
        except Exception as exc:  # noqa: BLE001
            fake.errors.append(exc)
            fake.bar.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not fake.errors, fake.errors
    assert all(r is not None for r in res)
    return res


class Coll:     # what learn_tp uses of cirs_hip.distributed.Collectives
    def __init__(self, fake):
        self.fake = fake

    def all_gather(self, out, inp):
        self.fake.all_gather_into_tensor(out, inp)

    def all_reduce(self, t):
        self.fake.all_reduce(t)


def tp_case(out, tag, ent, **env):
    set_env(**env)
    W, I, B, T, bs = 2, 512, 40, 12, 64
    Is = I // W
    pp, lens, perms, traj, n = case_data(I, B, T, seed=19)
    lns = []
    for r in range(W):
        sp = dict(pp)
        sp["wa"], sp["ba"] = pp["wa"][r * Is:(r + 1) * Is].contiguous(), pp["ba"][r * Is:(r + 1) * Is].contiguous()
        lns.append(make(sp, Is, B, T, ent))

    def fn(r, fake):
        lns[r].prepare(traj, lens)
        return lns[r].learn_tp(bs, 2, perms, r, W, r * Is, Coll(fake))

    res = run_ranks(W, fn)
    for r in range(W):
        dump(out, f"{tag}/rank{r}", lns[r], res[r])


def dp_case(out, tag, **env):
    set_env(**env)
    W, I, B, T, bs = 2, 180, 24, 30, 70
    pp, lens, perms, traj, n = case_data(I, B, T, seed=23)
    lns = [make(pp, I, B, T, 0.01) for _ in range(W)]

    def fn(r, fake):
        lns[r].prepare(traj, lens)
        return lns[r].learn_dp(bs, 2, perms, r, W, fake.all_reduce)

    res = run_ranks(W, fn)
    for r in range(W):
        dump(out, f"{tag}/rank{r}", lns[r], res[r])


def learn_case(out, tag, **env):
    set_env(**env)
    I, B, T, bs = 180, 24, 30, 70
    pp, lens, perms, traj, n = case_data(I, B, T, seed=23)
    ln = make(pp, I, B, T, 0.01)
    ln.prepare(traj, lens)
    losses = ln.learn(bs, 2, perms=perms)
    dump(out, tag, ln, losses)
    print(tag, "rows", n, "steps", losses.shape[0], flush=True)


def run(out_path, trace):
    out = {}
    print("library:", abi.LIB_PATH, flush=True)
    learn_case(out, "learn")
    tp_case(out, "tp_ent0", 0.0)
    if not trace:
        tp_case(out, "tp_ent0.01", 0.01)
        tp_case(out, "tp_ent0_recompute", 0.0, CIRS_PPO_HEAD_RECOMPUTE="1")
        tp_case(out, "tp_ent0.01_recompute", 0.01, CIRS_PPO_HEAD_RECOMPUTE="1")
        dp_case(out, "dp_chain")
        dp_case(out, "dp_chain_rows0", CIRS_PPO_ROWS_KERNEL="0")
        learn_case(out, "learn_rows0", CIRS_PPO_ROWS_KERNEL="0")
        learn_case(out, "learn_merge1", CIRS_PPO_MERGE_KERNEL="1")
        learn_case(out, "learn_prefetch0", CIRS_PPO_LEARN_PREFETCH="0")
        for k, t in out.items():
            assert bool(torch.isfinite(t.float()).all()), k
        torch.save(out, out_path)
        print("saved", len(out), "tensors to", out_path, flush=True)
    torch.cuda.synchronize()
    print("done", flush=True)


def kernel_name(full):
    """The demangled name without its argument list (the last balanced parenthesis group)."""
    if not full.endswith(")"):
        return full
    depth = 0
    for i in range(len(full) - 1, -1, -1):
        depth += (full[i] == ")") - (full[i] == "(")
        if depth == 0:
            return full[:i]
    return full


def sequences(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (d, files)
    rows = list(csv.DictReader(open(files[0])))
    per = {}
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        per.setdefault(r["Thread_Id"], []).append((kernel_name(r["Kernel_Name"]), grid, wg))
    # the main thread first (it dispatches first), then the rank threads in the order of their content (their ids differ from run to run)
    first = min(per, key=lambda t: min(int(r["Dispatch_Id"]) for r in rows if r["Thread_Id"] == t))
    return [per[first]] + sorted(v for t, v in per.items() if t != first)


def compare(pa, ch, ta, tb, out_path):
    a, b = torch.load(pa), torch.load(ch)
    na, nb = (os.path.splitext(os.path.basename(f))[0] for f in (pa, ch))
    lines, bad = [], 0
    lines.append(f"## saved tensors: {na} library vs {nb} library (torch.equal, all finite)")
    lines.append(f"{'tensor':44s} {'shape':>14s} {'equal':>6s} {'finite':>7s} {'max |' + na + '|':>13s}")
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in sorted(a):
        eq = a[k].shape == b[k].shape and torch.equal(a[k], b[k])
        fin = bool(torch.isfinite(a[k].float()).all() and torch.isfinite(b[k].float()).all())
        bad += (not eq) + (not fin)
        lines.append(f"{k:44s} {str(tuple(a[k].shape)):>14s} {str(eq):>6s} {str(fin):>7s} {float(a[k].float().abs().max()):13.6g}")
    lines.append(f"{len(a)} tensors, {bad} differences or non-finite")
    sa, sb = sequences(ta), sequences(tb)
    lines.append("")
    lines.append("## kernel sequences (rocprofv3 --kernel-trace; per host thread, in dispatch order; every kernel of the process, torch's included)")
    legend = {}
    for seqs in (sa, sb):
        for s in seqs:
            for e in s:
                legend.setdefault(e, len(legend))
    for e, i in legend.items():
        lines.append(f"  k{i:<3d} {e[0]}  grid {e[1]}  workgroup {e[2]}")
    same = sa == sb
    bad += not same
    for name, seqs in ((na, sa), (nb, sb)):
        for t, s in enumerate(seqs):
            lines.append(f"{name} thread {t} ({len(s)} dispatches): " + " ".join(f"k{legend[e]}" for e in s))
    lines.append(f"sequences of (kernel name, grid, workgroup size) equal: {same}")
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[:60]))
    print("...", lines[-1])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], "--trace" in sys.argv)
    else:
        compare(*sys.argv[2:7])
