"""CPU: the conditions that tests/trackercase.py's cases have to meet, proved from the reference alone (no device): no ReLU branch point within reach of
float32 rounding, every case has the property its name claims, the dispatch limits in the case table are the ones csrc/tracker_bwd.hip's formula gives,
and the float64 restatement reproduces the states recorded from the reference."""
import os
import re

import numpy as np
import pytest
import torch

import nn_oracle
import trackercase as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(tc.CASES))
def test_no_relu_branch_point_within_the_margin(name):
    c = tc.CASES[name]
    p, users, acts, rews, G, g_last = tc.inputs(c)
    r = tc.restatement(c, p, users, acts, rews, G, g_last, torch.float64, want_grads=False)
    print(f"{name}: seed {c['seed']}, {int(c['lens'].sum())} rows, smallest |linear1 pre-activation| of a live row {r['margin']:.2e}")
    assert r["margin"] > tc.RELU_MARGIN


@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_has_the_property_its_name_claims(name):
    c = tc.CASES[name]
    lens, T, cl = c["lens"], c["T"], c["claims"]
    assert cl, "a case without a claim"
    assert lens.min() >= 0 and lens.max() <= T + 1 and lens.sum() > 0
    checks = dict(R=lambda v: lens.sum() == v, min_R=lambda v: lens.sum() >= v, B=lambda v: len(lens) == v, max_len=lambda v: T + 1 == v,
                  min_max_len=lambda v: T + 1 >= v, full=lambda v: (lens.max() == T + 1) == v, has=lambda v: set(v) <= set(lens.tolist()),
                  min_len=lambda v: lens.min() >= v, ep=lambda v: tc.takes_episode_kernels(c["nhead"], T + 1) == v,
                  nlayers=lambda v: c["nlayers"] == v, S=lambda v: c["S"] == v, pad=lambda v: c["pad"] == v, p=lambda v: c["p"] == v,
                  hot_rows=lambda v: sum(int((tc.inputs(c)[2][b, :max(lens[b] - 1, 0)] == 7).sum()) for b in range(len(lens))) >= v)
    for k, v in cl.items():
        assert checks[k](v), (name, k, v)
    if c["modes"]:
        assert lens.min() >= 1
    m = re.fullmatch(r"R(\d+)(-p.*)?", name)
    if m:
        assert lens.sum() == int(m.group(1))
    m = re.fullmatch(r"ep-nh(\d)-L(\d+)(-p.*)?", name)
    if m:
        nh, L = int(m.group(1)), int(m.group(2))
        assert c["nhead"] == nh and T + 1 == L and L in (tc.EP_LIMIT[nh], tc.EP_LIMIT[nh] + 1) and 3 <= len(lens) <= 4
        assert ("rows" in c["paths"]) == (L == tc.EP_LIMIT[nh]), "at the limit itself the per-row path is forced too"


def test_case_table_covers_what_it_is_for():
    C = tc.CASES
    for nh, lim in tc.EP_LIMIT.items():      # both sides of every head count's limit
        assert any(c["nhead"] == nh and c["T"] + 1 == lim and c["p"] == 0 for c in C.values())
        assert any(c["nhead"] == nh and c["T"] + 1 == lim + 1 for c in C.values())
    assert {c["nlayers"] for c in C.values()} >= {1, 2, 3} and {c["S"] for c in C.values()} >= {1, 7, 20, 32}
    assert sorted(c["p"] for c in C.values() if c["p"] > 0) == [0.1, 0.3]
    assert len(tc.MODE_CASES) == 2
    special_lens = {C[k]["T"] + 1 for k in tc.SPECIAL_CASES}
    assert {tc.PREFIX_ONE_LAUNCH_MAX_LEN, tc.PREFIX_ONE_LAUNCH_MAX_LEN + 1} <= special_lens
    assert any(C[k]["nlayers"] == 3 for k in tc.SPECIAL_CASES) and any(0 in C[k]["lens"] for k in tc.SPECIAL_CASES)
    from cirs_hip import abi
    with open(os.path.join(ROOT, "include", "cirs_hip.h")) as f:
        ceiling = int(re.search(r"#define\s+CIRS_MAX_TRACKER_LAYERS\s+(\d+)", f.read()).group(1))
    assert ceiling == abi.MAX_TRACKER_LAYERS and max(c["nlayers"] for c in C.values()) <= ceiling


def test_episode_limits_follow_from_the_library_formula():
    """EP_LIMIT against the restated formula, and the restated formula against the text of csrc/tracker_bwd.hip (so an edit of either shows)."""
    for nh, lim in tc.EP_LIMIT.items():
        fits = [L for L in range(1, 130) if tc.takes_episode_kernels(nh, L)]
        assert fits == list(range(1, lim + 1)), nh
    with open(os.path.join(ROOT, "cirs-codes_amd", "csrc", "tracker_bwd.hip")) as f:
        src = f.read()
    for piece in ("static constexpr int NW = NH < 4 ? NH : 4;", "static constexpr int HPL = NH / NW;", "return (HPL * Lp) | 1;",
                  "keep_words(int Lp) { return 2 * (size_t)NH * Lp; }",
                  "bwd_floats(int Lp) { return (size_t)Lp * 128 + (size_t)NW * (Lp + 1) * strip(Lp) + 2 * (size_t)NH * Lp + keep_words(Lp); }",
                  "const bool ep = L <= 64 && ep_bytes(true) <= 64 * 1024", "if (state_out && ep && L <= 32 &&"):
        assert piece in src, piece


def test_float64_restatement_reproduces_the_recorded_states(golden_dir):
    z = np.load(os.path.join(golden_dir, "tracker.npz"))
    p = {k: v.double() for k, v in nn_oracle.tracker_params(z).items()}
    with torch.no_grad():
        st = nn_oracle.tracker_states(p, z["users"], z["acts"], z["rews"])
    assert st.dtype == torch.float64
    got, want = st.float().numpy(), z["states"]
    m = np.isfinite(want)
    assert m.any()
    print(f"float64 restatement vs recorded states: max |err| {np.abs(got[m] - want[m]).max():.3e} (bar {tc.GOLDEN_BAR})")
    np.testing.assert_allclose(got[m], want[m], rtol=tc.GOLDEN_BAR, atol=tc.GOLDEN_BAR)


def test_float32_restatement_error_is_what_the_bar_assumes():
    """e32 is computed, never a constant; this only pins its order of magnitude, so that a broken restatement cannot open the bar: on every case the
    float32 restatement stays within 1e-5 of float64 in the states and 5e-5 in every gradient tensor (the key-bias gradient is ~1e-16 in float64)."""
    for name in ("R33", "len-edges", "ep-nh4-L47-p0.1"):
        ref = tc.reference(name)
        assert ref["s_e32"] < 1e-5 and max(ref["e32"].values()) < 5e-5, name
        for k, g in ref["g64"].items():
            if k.endswith("self_attn.in_proj_bias"):
                assert np.abs(g[32:64]).max() <= 1e-12 * np.abs(g).max()
