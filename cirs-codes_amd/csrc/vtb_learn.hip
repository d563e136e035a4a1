// vtb_learn.hip -- the VirtualTaobao PPO update (CIRS-RL-taobao.py, HostPPOPolicy.update of core/host_rl.py) on gfx950.
//
// One update over the buffer of one device collect:
//   vtb_learn_forward_kernel      one workgroup per episode: the teacher-forced causal pass of the tracker over positions 0..len
//                                 (cirs_hip/vtb_host.py tracker_states, position-keyed dropout regenerated from the collect's key);
//                                 writes the states and keeps every activation the backward needs in the episode's workspace
//   vtb_learn_values_kernel       one wave per sampled row: critic of obs / obs_next, logp_old of the stored raw action
//   vtb_learn_gae_kernel          one thread per GAE segment of the sample order, fp64 (lambda_returns)
//   vtb_learn_rms_kernel          the block's (n, mean, var) in a fixed order, merged into the running return statistics (fp64)
//   vtb_learn_minibatch_kernel    64 rows per workgroup: advantage whitening (recomputed per workgroup), the row objective, its
//                                 gradient through the heads and the Net trunk, per-workgroup gradient partials; dL/dstate per row
//                                 on the last pass
//   vtb_learn_adam_kernel         one workgroup: fixed-order reduction of the partials, clip_grad_norm_ (trunk counted twice), Adam
//                                 (two sub-steps for the trunk; bias corrections from the host), the minibatch's loss record
//   vtb_learn_tracker_bwd_kernel  one workgroup per episode: dL/dstate of the obs rows back through decoder, both encoder layers, PE
//                                 and the input slots into per-episode tracker gradient partials
//   vtb_learn_tracker_adam_kernel fixed-order reduction over episodes, one Adam step of the tracker
// Exact redraw (cirs_vtb_learn_*_redraw, the buffer of a dropout_redraw collect): the forward and the tracker backward run per CALL (c, e)
// instead of per episode -- positions 0..c with the masks of dropout env id drop_env_base + c * n_env + e, state and gradient on the last
// position -- in vtb_learn_forward_redraw_kernel / vtb_learn_tracker_redraw_kernel, built from the same two device functions.
// No float atomics: every sum has a fixed order, so two runs from the same snapshot are bit-identical.  fp32 FMA, fp64 for GAE,
// the return statistics, the advantage moments and the gradient norm.  Parameter images are in torch's [out][in] layout.
#include "common.h"
#include "optim.h"
#include "rng.h"
#include "vtb_model.h"

namespace cirs {
namespace {

constexpr int kA = CIRS_VTB_ACTION_DIM, kU = CIRS_VTB_USER_DIM, kObs = kA + 3, kObs0 = kU + 3;
constexpr int kT = 256;         // threads of the per-episode and per-tile kernels
constexpr int kRows = 64;       // rows per minibatch workgroup
constexpr int kMaxW = 128;      // trunk widths
constexpr int kAdamT = 1024;

struct TLay {   // tracker image offsets (floats)
    long user_w, user_b, gate_w, gate_b, dec_w, dec_b, total;
    long in_w[CIRS_VTB_RO_MAX_LAYERS], in_b[CIRS_VTB_RO_MAX_LAYERS], out_w[CIRS_VTB_RO_MAX_LAYERS], out_b[CIRS_VTB_RO_MAX_LAYERS];
    long l1_w[CIRS_VTB_RO_MAX_LAYERS], l1_b[CIRS_VTB_RO_MAX_LAYERS], l2_w[CIRS_VTB_RO_MAX_LAYERS], l2_b[CIRS_VTB_RO_MAX_LAYERS];
    long n1_w[CIRS_VTB_RO_MAX_LAYERS], n1_b[CIRS_VTB_RO_MAX_LAYERS], n2_w[CIRS_VTB_RO_MAX_LAYERS], n2_b[CIRS_VTB_RO_MAX_LAYERS];
};
struct PLay {   // policy image offsets (floats)
    long tw[CIRS_VTB_RO_MAX_HIDDEN], tb[CIRS_VTB_RO_MAX_HIDDEN], tin[CIRS_VTB_RO_MAX_HIDDEN];
    long mu_w, mu_b, sg_w, sg_b, sp, c_w, c_b, trunk_end, total;
    int width;  // last trunk width
};
struct ELay {   // per-episode workspace (floats); positions are strided by Lp = max_turn + 1
    long X, SIG, G, DU, DH, DS, DFF, DQKV, total;
    long QKV[CIRS_VTB_RO_MAX_LAYERS], P[CIRS_VTB_RO_MAX_LAYERS], PM[CIRS_VTB_RO_MAX_LAYERS], ATT[CIRS_VTB_RO_MAX_LAYERS];
    long XH1[CIRS_VTB_RO_MAX_LAYERS], H1[CIRS_VTB_RO_MAX_LAYERS], RS1[CIRS_VTB_RO_MAX_LAYERS], FF[CIRS_VTB_RO_MAX_LAYERS];
    long XH2[CIRS_VTB_RO_MAX_LAYERS], RS2[CIRS_VTB_RO_MAX_LAYERS];
};
struct WLay {   // workspace (floats)
    long states, dsrow, env, tslab, now, nxt, vs, adv, ret, logp_old, total64, rowbuf, pslab, lslab, total;
    long row_stride;      // rowbuf floats per minibatch row
    long max_wg;          // minibatch workgroups of the largest minibatch (n_rows rows)
};
struct Lay {
    TLay t;
    PLay p;
    ELay e;
    WLay w;
    int Lp;
    int n_wg;      // tracker workgroups = episode workspaces = gradient slabs: n_env, or n_env * groups in the exact-redraw mode
    int groups;    // exact-redraw mode: workgroups per env, group g runs the calls c = g, g + groups, ...
};

// redraw: the exact-redraw layout (cirs_vtb_learn_*_redraw with dropout_p > 0)
Lay make_layout(const cirs_vtb_learn_cfg& c, bool redraw = false) {
    Lay L{};
    const long D = c.model.dim_model, F = c.model.d_hid, S = c.model.dim_state, H = c.model.nhead;
    long o = 0;
    auto take = [&o](long n) { const long r = o; o += n; return r; };
    L.t.user_w = take(D * kU); L.t.user_b = take(D);
    L.t.gate_w = take(D * (1 + kA)); L.t.gate_b = take(D);
    for (int l = 0; l < c.model.nlayers; ++l) {
        L.t.in_w[l] = take(3 * D * D); L.t.in_b[l] = take(3 * D);
        L.t.out_w[l] = take(D * D); L.t.out_b[l] = take(D);
        L.t.l1_w[l] = take(F * D); L.t.l1_b[l] = take(F);
        L.t.l2_w[l] = take(D * F); L.t.l2_b[l] = take(D);
        L.t.n1_w[l] = take(D); L.t.n1_b[l] = take(D);
        L.t.n2_w[l] = take(D); L.t.n2_b[l] = take(D);
    }
    L.t.dec_w = take(S * D); L.t.dec_b = take(S);
    L.t.total = o;

    o = 0;
    long in = S;
    for (int i = 0; i < c.model.n_hidden; ++i) {
        L.p.tin[i] = in;
        L.p.tw[i] = take((long)c.model.hidden[i] * in);
        L.p.tb[i] = take(c.model.hidden[i]);
        in = c.model.hidden[i];
    }
    L.p.width = (int)in;
    L.p.trunk_end = o;
    L.p.mu_w = take(kA * in); L.p.mu_b = take(kA);
    if (c.model.conditioned_sigma) {
        L.p.sg_w = take(kA * in); L.p.sg_b = take(kA); L.p.sp = -1;
    } else {
        L.p.sg_w = L.p.sg_b = -1; L.p.sp = take(kA);
    }
    L.p.c_w = take(in); L.p.c_b = take(1);
    L.p.total = o;

    const long Lp = c.max_turn + 1;
    L.Lp = (int)Lp;
    o = 0;
    L.e.X = take((c.model.nlayers + 1) * Lp * D);
    for (int l = 0; l < c.model.nlayers; ++l) {
        L.e.QKV[l] = take(Lp * 3 * D);
        L.e.P[l] = take(H * Lp * Lp);
        L.e.PM[l] = take(H * Lp * Lp);
        L.e.ATT[l] = take(Lp * D);
        L.e.XH1[l] = take(Lp * D); L.e.H1[l] = take(Lp * D); L.e.RS1[l] = take(Lp);
        L.e.FF[l] = take(Lp * F);
        L.e.XH2[l] = take(Lp * D); L.e.RS2[l] = take(Lp);
    }
    L.e.SIG = take(Lp * D);
    L.e.G = take(Lp * D); L.e.DU = take(Lp * D); L.e.DH = take(Lp * D);
    L.e.DS = take(Lp * S);
    L.e.DFF = take(Lp * F); L.e.DQKV = take(Lp * 3 * D);
    L.e.total = (o + 3) / 4 * 4;

    long sumh = 0;
    for (int i = 0; i < c.model.n_hidden; ++i) sumh += c.model.hidden[i];
    const long n = c.n_rows, B = c.n_env;
    // a pseudo-episode's activations live only from its forward to its backward inside one workgroup, so the workspace grows with the
    // workgroups in flight, not with the sum of the prefix lengths: up to 8 per env while that keeps <= 1024 of them
    L.groups = redraw ? (int)(1024 / B < 1 ? 1 : 1024 / B > 8 ? 8 : 1024 / B) : 1;
    L.n_wg = (int)B * L.groups;
    o = 0;
    L.w.states = take(Lp * B * S);
    L.w.dsrow = take(n * S);
    L.w.env = take(L.n_wg * L.e.total);
    L.w.tslab = take(L.n_wg * L.t.total);
    L.w.vs = take(n); L.w.adv = take(n); L.w.ret = take(n); L.w.logp_old = take(n);   // the per-row block, in this order
    L.w.now = take(n); L.w.nxt = take(n);
    o = (o + 1) / 2 * 2;
    L.w.total64 = take(2 * n);
    L.w.row_stride = 2 * sumh + 2 * kA + 1 + 3;
    L.w.rowbuf = take(n * L.w.row_stride);
    L.w.max_wg = cdiv(n, kRows);
    L.w.pslab = take(L.w.max_wg * L.p.total);
    o = (o + 1) / 2 * 2;
    L.w.lslab = take(2 * 3 * L.w.max_wg);
    L.w.total = o;
    return L;
}

// keep decision of (position, layer, site, element) of this episode (csrc/rng.h; needs c, denv, thr in scope)
#define LEARN_KEEP(P, LAYER, SITE, ELEM) \
    dropout_keep(c.model.dropout_seed, denv, (uint32_t)(P), (uint32_t)(LAYER), (uint32_t)(SITE), (uint32_t)(ELEM), thr)

__device__ __forceinline__ float sigm(float g) { return 1.0f / (1.0f + expf(-g)); }

// ---- tracker forward: one workgroup per (pseudo-)episode ------------------------------------------------------------------------
// The teacher-forced causal pass over the slots 0..np-1 of env e with the masks of dropout env id denv; activations into the workspace w.
// LAST: only the state of position np - 1 is handed out (the state of call np - 1 in the exact-redraw mode).
template <bool DROP, bool LAST>
__device__ __forceinline__ void tracker_forward(const cirs_vtb_learn_cfg& c, const cirs_vtb_learn_bufs& b, const Lay& L, int e, int np,
                                                uint32_t denv, float* w) {
    const int tid = threadIdx.x;
    const int B = c.n_env, D = c.model.dim_model, H = c.model.nhead, HD = D / H, F = c.model.d_hid, S = c.model.dim_state;
    const int NL = c.model.nlayers, Lp = L.Lp;
    const float* tp = b.tparams;
    const uint32_t thr = DROP ? dropout_threshold(c.model.dropout_p) : 0u;
    const float inv = DROP ? 1.0f / (1.0f - c.model.dropout_p) : 1.0f;
    const float sqd = sqrtf((float)D);
    float* X0 = w + L.e.X;
    for (int i = tid; i < np * D; i += kT) {
        const int p = i / D, d = i % D;
        float x;
        if (p == 0) {
            const double* o0 = b.obs0 + (long)e * kObs0;
            float acc = tp[L.t.user_b + d];
            const float* W = tp + L.t.user_w + (long)d * kU;
            for (int u = 0; u < kU; ++u) acc = __builtin_fmaf(W[u], (float)o0[u], acc);
            x = acc;
        } else {
            const long row = (long)(p - 1) * B + e;
            const double* so = b.obs + row * kObs;
            const float* W = tp + L.t.gate_w + (long)d * (1 + kA);
            float acc = __builtin_fmaf(W[0], (float)b.rew[row], tp[L.t.gate_b + d]);
            for (int k = 0; k < kA; ++k) acc = __builtin_fmaf(W[1 + k], (float)so[k], acc);
            const float sg = sigm(acc);
            w[L.e.SIG + (long)p * D + d] = sg;
            x = sg * (float)so[d];
        }
        float h = x * sqd + b.pe[(long)p * D + d];
        if (DROP) h = LEARN_KEEP(p, 0, CIRS_DROP_POS, d) ? h * inv : 0.f;
        X0[(long)p * D + d] = h;
    }
    __syncthreads();
    const float qscale = 1.0f / sqrtf((float)HD);
    for (int l = 0; l < NL; ++l) {
        const float* X = w + L.e.X + (long)l * Lp * D;
        float* Xn = w + L.e.X + (long)(l + 1) * Lp * D;
        float* QKV = w + L.e.QKV[l];
        float* P = w + L.e.P[l];
        float* PM = w + L.e.PM[l];
        float* ATT = w + L.e.ATT[l];
        float* XH1 = w + L.e.XH1[l];
        float* H1 = w + L.e.H1[l];
        float* FF = w + L.e.FF[l];
        float* XH2 = w + L.e.XH2[l];
        for (int i = tid; i < np * 3 * D; i += kT) {
            const int p = i / (3 * D), o = i % (3 * D);
            const float* W = tp + L.t.in_w[l] + (long)o * D;
            float acc = tp[L.t.in_b[l] + o];
            for (int k = 0; k < D; ++k) acc = __builtin_fmaf(W[k], X[(long)p * D + k], acc);
            QKV[(long)p * 3 * D + o] = acc;
        }
        __syncthreads();
        for (int i = tid; i < np * H; i += kT) {
            const int p = i / H, h = i % H;
            float* pr = P + ((long)h * Lp + p) * Lp;
            float* pm = PM + ((long)h * Lp + p) * Lp;
            const float* q = QKV + (long)p * 3 * D + h * HD;
            float mx = -INFINITY;
            for (int j = 0; j <= p; ++j) {
                const float* k = QKV + (long)j * 3 * D + D + h * HD;
                float sc = 0.f;
                for (int d = 0; d < HD; ++d) sc = __builtin_fmaf(q[d] * qscale, k[d], sc);
                pr[j] = sc;
                mx = fmaxf(mx, sc);
            }
            float sm = 0.f;
            for (int j = 0; j <= p; ++j) {
                const float ex = expf(pr[j] - mx);
                pr[j] = ex;
                sm += ex;
            }
            const float r = 1.0f / sm;
            for (int j = 0; j <= p; ++j) {
                const float pv = pr[j] * r;
                pr[j] = pv;
                pm[j] = DROP ? (LEARN_KEEP(p, l, CIRS_DROP_ATTN, j * H + h) ? pv * inv : 0.f) : pv;
            }
        }
        __syncthreads();
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, d = i % D, h = d / HD;
            const float* pm = PM + ((long)h * Lp + p) * Lp;
            float acc = 0.f;
            for (int j = 0; j <= p; ++j) acc = __builtin_fmaf(pm[j], QKV[(long)j * 3 * D + 2 * D + d], acc);
            ATT[(long)p * D + d] = acc;
        }
        __syncthreads();
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, o = i % D;
            const float* W = tp + L.t.out_w[l] + (long)o * D;
            float sa = tp[L.t.out_b[l] + o];
            for (int k = 0; k < D; ++k) sa = __builtin_fmaf(W[k], ATT[(long)p * D + k], sa);
            if (DROP) sa = LEARN_KEEP(p, l, CIRS_DROP_RES1, o) ? sa * inv : 0.f;
            XH1[(long)p * D + o] = X[(long)p * D + o] + sa;
        }
        __syncthreads();
        for (int p = tid; p < np; p += kT) {      // LayerNorm 1 (biased variance, eps 1e-5)
            float* u = XH1 + (long)p * D;
            float m = 0.f;
            for (int d = 0; d < D; ++d) m += u[d];
            m /= (float)D;
            float v = 0.f;
            for (int d = 0; d < D; ++d) v = __builtin_fmaf(u[d] - m, u[d] - m, v);
            const float rs = 1.0f / sqrtf(v / (float)D + 1e-5f);
            for (int d = 0; d < D; ++d) {
                const float xh = (u[d] - m) * rs;
                u[d] = xh;
                H1[(long)p * D + d] = __builtin_fmaf(xh, tp[L.t.n1_w[l] + d], tp[L.t.n1_b[l] + d]);
            }
            w[L.e.RS1[l] + p] = rs;
        }
        __syncthreads();
        for (int i = tid; i < np * F; i += kT) {
            const int p = i / F, f = i % F;
            const float* W = tp + L.t.l1_w[l] + (long)f * D;
            float acc = tp[L.t.l1_b[l] + f];
            for (int k = 0; k < D; ++k) acc = __builtin_fmaf(W[k], H1[(long)p * D + k], acc);
            FF[(long)p * F + f] = fmaxf(acc, 0.f);
        }
        __syncthreads();
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, o = i % D;
            const float* W = tp + L.t.l2_w[l] + (long)o * F;
            float acc = tp[L.t.l2_b[l] + o];
            for (int f = 0; f < F; ++f) {
                float fv = FF[(long)p * F + f];
                if (DROP) fv = LEARN_KEEP(p, l, CIRS_DROP_FF, f) ? fv * inv : 0.f;
                acc = __builtin_fmaf(W[f], fv, acc);
            }
            if (DROP) acc = LEARN_KEEP(p, l, CIRS_DROP_RES2, o) ? acc * inv : 0.f;
            XH2[(long)p * D + o] = H1[(long)p * D + o] + acc;
        }
        __syncthreads();
        for (int p = tid; p < np; p += kT) {      // LayerNorm 2
            float* u = XH2 + (long)p * D;
            float m = 0.f;
            for (int d = 0; d < D; ++d) m += u[d];
            m /= (float)D;
            float v = 0.f;
            for (int d = 0; d < D; ++d) v = __builtin_fmaf(u[d] - m, u[d] - m, v);
            const float rs = 1.0f / sqrtf(v / (float)D + 1e-5f);
            for (int d = 0; d < D; ++d) {
                const float xh = (u[d] - m) * rs;
                u[d] = xh;
                Xn[(long)p * D + d] = __builtin_fmaf(xh, tp[L.t.n2_w[l] + d], tp[L.t.n2_b[l] + d]);
            }
            w[L.e.RS2[l] + p] = rs;
        }
        __syncthreads();
    }
    const float* XL = w + L.e.X + (long)NL * Lp * D;
    float* states = b.ws + L.w.states;
    for (int i = tid + (LAST ? (np - 1) * S : 0); i < np * S; i += kT) {
        const int p = i / S, s = i % S;
        const float* W = tp + L.t.dec_w + (long)s * D;
        float acc = tp[L.t.dec_b + s];
        for (int k = 0; k < D; ++k) acc = __builtin_fmaf(W[k], XL[(long)p * D + k], acc);
        states[((long)p * B + e) * S + s] = acc;
    }
}

// position-keyed mode: one pass per episode over positions 0..len (the last one is obs_next of the last row)
template <bool DROP>
__global__ __launch_bounds__(kT) void vtb_learn_forward_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L) {
    const int e = blockIdx.x;
    tracker_forward<DROP, false>(c, b, L, e, b.len[e] + 1, (uint32_t)(c.model.drop_env_base + e), b.ws + L.w.env + (long)e * L.e.total);
}

// exact-redraw mode: workgroup (e, g) runs the calls c = g, g + groups, ... <= len of env e, each a pass of its own over the slots 0..c
// with the masks of dropout env id drop_env_base + c * n_env + e; only the states leave (the update runs the passes again)
__global__ __launch_bounds__(kT) void vtb_learn_forward_redraw_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L) {
    const int e = blockIdx.x / L.groups, g = blockIdx.x % L.groups;
    float* w = b.ws + L.w.env + (long)blockIdx.x * L.e.total;
    const int len = b.len[e];
    for (int call = g; call <= len; call += L.groups) {
        tracker_forward<true, true>(c, b, L, e, call + 1, (uint32_t)(c.model.drop_env_base + call * c.n_env + e), w);
        __syncthreads();
    }
}

// ---- per-row networks (one wave per row) ------------------------------------------------------------------------------------
struct RowOut {
    float logp, ent, v;
};

// trunk forward from in[S] (wave LDS) into act (global, per layer) and the last activation in lds `last`; returns it
__device__ __forceinline__ const float* trunk_fwd(const cirs_vtb_learn_cfg& c, const Lay& L, const float* pp, float* buf0, float* buf1,
                                                  float* A, int lane) {
    float* in = buf0;
    float* out = buf1;
    long aoff = 0;
    for (int li = 0; li < c.model.n_hidden; ++li) {
        const int O = c.model.hidden[li], K = (int)L.p.tin[li];
        for (int o = lane; o < O; o += 64) {
            const float* W = pp + L.p.tw[li] + (long)o * K;
            float acc = pp[L.p.tb[li] + o];
            for (int k = 0; k < K; ++k) acc = __builtin_fmaf(W[k], in[k], acc);
            const float a = fmaxf(acc, 0.f);
            out[o] = a;
            if (A) A[aoff + o] = a;
        }
        __builtin_amdgcn_wave_barrier();
        aoff += O;
        float* t = in;
        in = out;
        out = t;
    }
    return in;
}

// heads over the last trunk activation h: logp of act, entropy, value; mu / sigma pieces left in lanes < 27
struct HeadLane {
    float pre, mu, sig, diff, hs;
};
__device__ __forceinline__ RowOut heads(const cirs_vtb_learn_cfg& c, const Lay& L, const float* pp, const float* h, const float* act, int lane,
                                        HeadLane& hl) {
    const int W = L.p.width;
    float lp = 0.f, en = 0.f;
    hl = HeadLane{0.f, 0.f, 1.f, 0.f, 0.f};
    if (lane < kA) {
        const float* Wm = pp + L.p.mu_w + (long)lane * W;
        float pre = pp[L.p.mu_b + lane];
        for (int k = 0; k < W; ++k) pre = __builtin_fmaf(Wm[k], h[k], pre);
        const float mu = c.model.unbounded ? pre : c.model.max_action * tanhf(pre);
        float sig;
        float hs = 0.f;
        if (c.model.conditioned_sigma) {
            const float* Ws = pp + L.p.sg_w + (long)lane * W;
            hs = pp[L.p.sg_b + lane];
            for (int k = 0; k < W; ++k) hs = __builtin_fmaf(Ws[k], h[k], hs);
            sig = expf(fminf(fmaxf(hs, -20.f), 2.f));
        } else {
            sig = expf(pp[L.p.sp + lane]);
        }
        const float ls = logf(sig);
        const float diff = act[lane] - mu;
        lp = -(diff * diff) / (2.0f * (sig * sig)) - ls - 0.91893853320467274f;
        en = 0.5f + 0.91893853320467274f + ls;
        hl = HeadLane{pre, mu, sig, diff, hs};
    }
    float vv = 0.f;
    for (int k = lane; k < W; k += 64) vv = __builtin_fmaf(pp[L.p.c_w + k], h[k], vv);
    RowOut r;
    r.logp = wave_sum_f32(lp);
    r.ent = wave_sum_f32(en);
    r.v = wave_sum_f32(vv) + pp[L.p.c_b];
    return r;
}

// ---- returns stage -------------------------------------------------------------------------------------------------------------
constexpr int kVW = 4;   // waves per values workgroup
__global__ __launch_bounds__(64 * kVW) void vtb_learn_values_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L, int want_logp) {
    __shared__ float sm[kVW][2][kMaxW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = blockIdx.x * kVW + wv;
    if (r >= c.n_rows) return;           // wave-uniform
    const int B = c.n_env, S = c.model.dim_state;
    const int t = b.rows[r], e = b.rows[c.n_rows + r];
    const float* states = b.ws + L.w.states;
    const float* pp = b.pparams;
    float* ws = b.ws;
    for (int which = 0; which < 2; ++which) {
        const float* s = states + ((long)(t + which) * B + e) * S;
        for (int k = lane; k < S; k += 64) sm[wv][0][k] = s[k];
        __builtin_amdgcn_wave_barrier();
        const float* h = trunk_fwd(c, L, pp, sm[wv][0], sm[wv][1], nullptr, lane);
        HeadLane hl;
        const RowOut o = heads(c, L, pp, h, b.act + ((long)t * B + e) * kA, lane, hl);
        if (lane == 0) {
            if (which == 0) {
                ws[L.w.now + r] = o.v;
                if (want_logp) ws[L.w.logp_old + r] = o.logp;
            } else {
                ws[L.w.nxt + r] = o.v;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(256) void vtb_learn_gae_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c.n_seg) return;
    const int B = c.n_env, n = c.n_rows;
    const int end = b.seg_end[k], beg = k == 0 ? 0 : b.seg_end[k - 1];
    float* ws = b.ws;
    double* tot = (double*)(ws + L.w.total64);
    const double unit = c.scale_returns ? sqrt(b.rms[1] + c.floor) : 1.0;
    double run = 0.0;
    for (int i = end - 1; i >= beg; --i) {
        const int t = b.rows[i], e = b.rows[n + i];
        const long te = (long)t * B + e;
        const double now = (double)ws[L.w.now + i] * unit;
        const double nxt = b.done[te] ? 0.0 : (double)ws[L.w.nxt + i] * unit;
        const double td = b.rew[te] + c.discount * nxt - now;
        const double carry = b.boundary[i] ? 0.0 : c.discount * c.lam;
        run = td + carry * run;
        const double total = run + now;
        tot[i] = total;
        ws[L.w.adv + i] = (float)run;
        ws[L.w.ret + i] = (float)(total / unit);
        ws[L.w.vs + i] = ws[L.w.now + i];
    }
}

__global__ __launch_bounds__(256) void vtb_learn_rms_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L) {
    __shared__ double red[256];
    const int n = c.n_rows, tid = threadIdx.x;
    const double* tot = (const double*)(b.ws + L.w.total64);
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += tot[i];
    const double mu = block_sum<256>(s, red) / n;
    double q = 0.0;
    for (int i = tid; i < n; i += 256) q += (tot[i] - mu) * (tot[i] - mu);
    const double s2 = block_sum<256>(q, red) / n;
    if (tid == 0) {   // ReturnScale.update: parallel-variance merge of one block
        const double w_old = b.rms[2], w_all = w_old + n, shift = mu - b.rms[0];
        const double var = (b.rms[1] * w_old + s2 * n + shift * shift * (w_old * n / w_all)) / w_all;
        b.rms[0] = b.rms[0] + shift * (n / w_all);
        b.rms[1] = var;
        b.rms[2] = w_all;
    }
}

// ---- minibatch: row objective and gradient ---------------------------------------------------------------------------------------
// rowbuf per minibatch row j: A [sum hidden] | DZ [sum hidden] | DPRE [27] | DSG [27] (dsigma_param or dL/dhead_sigma) | DV | terms [3]
__global__ __launch_bounds__(kT) void vtb_learn_minibatch_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L, const int32_t* perm,
                                                                 int m, int want_ds) {
    __shared__ double red[kT];
    __shared__ float sm[kT / 64][4][kMaxW];
    __shared__ float stat[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int B = c.n_env, S = c.model.dim_state, n = c.n_rows, W = L.p.width;
    float* ws = b.ws;
    const float* pp = b.pparams;
    const int j0 = blockIdx.x * kRows, j1 = min(j0 + kRows, m);
    // advantage moments of the whole minibatch (every workgroup recomputes them, fixed order)
    float amean = 0.f, astd = 1.f;
    if (c.whiten_adv) {
        double s = 0.0;
        for (int j = tid; j < m; j += kT) s += ws[L.w.adv + perm[j]];
        const double mu = block_sum<256>(s, red) / m;
        double q = 0.0;
        for (int j = tid; j < m; j += kT) {
            const double d = ws[L.w.adv + perm[j]] - mu;
            q += d * d;
        }
        const double var = block_sum<256>(q, red) / (m - 1);
        if (tid == 0) {
            stat[0] = (float)mu;
            stat[1] = (float)sqrt(var);
        }
        __syncthreads();
        amean = stat[0];
        astd = stat[1];
    }
    long sumh = 0;
    for (int i = 0; i < c.model.n_hidden; ++i) sumh += c.model.hidden[i];
    const long RS = L.w.row_stride;
    const float inv_m = 1.0f / (float)m;
    for (int j = j0 + wv; j < j1; j += kT / 64) {
        const int r = perm[j];
        const int t = b.rows[r], e = b.rows[n + r];
        float* rb = ws + L.w.rowbuf + (long)j * RS;
        const float* s = ws + L.w.states + ((long)t * B + e) * S;
        for (int k = lane; k < S; k += 64) sm[wv][0][k] = s[k];
        __builtin_amdgcn_wave_barrier();
        const float* h = trunk_fwd(c, L, pp, sm[wv][0], sm[wv][1], rb, lane);
        HeadLane hl;
        const RowOut o = heads(c, L, pp, h, b.act + ((long)t * B + e) * kA, lane, hl);
        // ---- the row's share of the objective
        const float adv = c.whiten_adv ? (ws[L.w.adv + r] - amean) / astd : ws[L.w.adv + r];
        const float w = expf(o.logp - ws[L.w.logp_old + r]);
        const float lo = 1.0f - c.clip, hi = 1.0f + c.clip;
        const float cw = fminf(fmaxf(w, lo), hi);
        const bool inr = w >= lo && w <= hi;
        const float s1 = w * adv, s2 = cw * adv;
        float gain = fminf(s1, s2);
        float dg = s1 < s2 ? adv : s1 > s2 ? (inr ? adv : 0.f) : 0.5f * adv + (inr ? 0.5f * adv : 0.f);   // torch.minimum ties split
        if (c.has_dual) {
            const float d2 = c.dual * adv;
            dg *= gain > d2 ? 1.f : gain < d2 ? 0.f : 0.5f;
            gain = fmaxf(gain, d2);
        }
        const float dlogp = -inv_m * dg * w;
        const float ret = ws[L.w.ret + r], vold = ws[L.w.vs + r];
        float err = (ret - o.v) * (ret - o.v);
        float derr = 2.0f * (o.v - ret);
        if (c.clip_value) {
            const float dv0 = o.v - vold;
            const float vb = vold + fminf(fmaxf(dv0, -c.clip), c.clip);
            const float e2 = (ret - vb) * (ret - vb);
            const float de2 = (dv0 >= -c.clip && dv0 <= c.clip) ? 2.0f * (vb - ret) : 0.f;
            derr = err > e2 ? derr : err < e2 ? de2 : 0.5f * derr + 0.5f * de2;
            err = fmaxf(err, e2);
        }
        const float dv = c.c_value * inv_m * derr;
        const float dent = -c.c_entropy * inv_m;
        // ---- heads backward (lanes < 27)
        float* A_last = rb + (sumh - W);
        float* DZ = rb + sumh;
        float* DPRE = rb + 2 * sumh;
        float* DSG = DPRE + kA;
        if (lane < kA) {
            const float var = hl.sig * hl.sig;
            const float dmu = dlogp * hl.diff / var;
            const float dpre = c.model.unbounded ? dmu : dmu * c.model.max_action * (1.0f - tanhf(hl.pre) * tanhf(hl.pre));
            DPRE[lane] = dpre;
            sm[wv][2][lane] = dpre;
            float dsg;
            if (c.model.conditioned_sigma) {
                const float dsig = dlogp * (hl.diff * hl.diff / (var * hl.sig) - 1.0f / hl.sig) + dent / hl.sig;
                dsg = (hl.hs >= -20.f && hl.hs <= 2.f) ? dsig * hl.sig : 0.f;
            } else {
                dsg = dlogp * (hl.diff * hl.diff / var - 1.0f) + dent;
            }
            DSG[lane] = dsg;
            sm[wv][3][lane] = dsg;
        }
        if (lane == 0) {
            rb[2 * sumh + 2 * kA] = dv;
            rb[2 * sumh + 2 * kA + 1] = gain;
            rb[2 * sumh + 2 * kA + 2] = err;
            rb[2 * sumh + 2 * kA + 3] = o.ent;
        }
        __builtin_amdgcn_wave_barrier();
        // dL/d(last activation)
        float* da = sm[wv][0];
        for (int k = lane; k < W; k += 64) {
            float acc = pp[L.p.c_w + k] * dv;
            for (int d = 0; d < kA; ++d) acc = __builtin_fmaf(pp[L.p.mu_w + (long)d * W + k], sm[wv][2][d], acc);
            if (c.model.conditioned_sigma)
                for (int d = 0; d < kA; ++d) acc = __builtin_fmaf(pp[L.p.sg_w + (long)d * W + k], sm[wv][3][d], acc);
            da[k] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        // trunk backward
        long aoff = sumh;
        for (int li = c.model.n_hidden - 1; li >= 0; --li) {
            const int O = c.model.hidden[li], K = (int)L.p.tin[li];
            aoff -= O;
            for (int q = lane; q < O; q += 64) {
                const float dz = rb[aoff + q] > 0.f ? da[q] : 0.f;
                DZ[aoff + q] = dz;
                sm[wv][1][q] = dz;
            }
            __builtin_amdgcn_wave_barrier();
            for (int k = lane; k < K; k += 64) {
                float acc = 0.f;
                for (int q = 0; q < O; ++q) acc = __builtin_fmaf(pp[L.p.tw[li] + (long)q * K + k], sm[wv][1][q], acc);
                da[k] = acc;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (want_ds)
            for (int k = lane; k < S; k += 64) ws[L.w.dsrow + (long)r * S + k] = da[k];
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // ---- this workgroup's gradient partial, rows in order
    float* slab = ws + L.w.pslab + (long)blockIdx.x * L.p.total;
    const float* rb0 = ws + L.w.rowbuf;
    for (long q = tid; q < L.p.total; q += kT) {
        float acc = 0.f;
        if (q < L.p.trunk_end) {
            int li = 0;
            while (li + 1 < c.model.n_hidden && q >= L.p.tw[li + 1]) ++li;
            long aoff = 0;
            for (int i = 0; i < li; ++i) aoff += c.model.hidden[i];
            const int K = (int)L.p.tin[li];
            if (q < L.p.tb[li]) {
                const long o = (q - L.p.tw[li]) / K, k = (q - L.p.tw[li]) % K;
                for (int j = j0; j < j1; ++j) {
                    const float* rb = rb0 + (long)j * RS;
                    float x;
                    if (li == 0) {
                        const int r = perm[j];
                        x = ws[L.w.states + ((long)b.rows[r] * B + b.rows[n + r]) * S + k];
                    } else {
                        x = rb[aoff - K + k];
                    }
                    acc = __builtin_fmaf(rb[sumh + aoff + o], x, acc);
                }
            } else {
                const long o = q - L.p.tb[li];
                for (int j = j0; j < j1; ++j) acc += rb0[(long)j * RS + sumh + aoff + o];
            }
        } else if (q < L.p.mu_b) {
            const long d = (q - L.p.mu_w) / W, k = (q - L.p.mu_w) % W;
            for (int j = j0; j < j1; ++j) acc = __builtin_fmaf(rb0[(long)j * RS + 2 * sumh + d], rb0[(long)j * RS + sumh - W + k], acc);
        } else if (q < L.p.mu_b + kA) {
            const long d = q - L.p.mu_b;
            for (int j = j0; j < j1; ++j) acc += rb0[(long)j * RS + 2 * sumh + d];
        } else if (q < L.p.c_w) {   // sigma: head or free parameter
            if (c.model.conditioned_sigma && q < L.p.sg_b) {
                const long d = (q - L.p.sg_w) / W, k = (q - L.p.sg_w) % W;
                for (int j = j0; j < j1; ++j) acc = __builtin_fmaf(rb0[(long)j * RS + 2 * sumh + kA + d], rb0[(long)j * RS + sumh - W + k], acc);
            } else {
                const long d = q - (c.model.conditioned_sigma ? L.p.sg_b : L.p.sp);
                for (int j = j0; j < j1; ++j) acc += rb0[(long)j * RS + 2 * sumh + kA + d];
            }
        } else if (q < L.p.c_b) {
            const long k = q - L.p.c_w;
            for (int j = j0; j < j1; ++j) acc = __builtin_fmaf(rb0[(long)j * RS + 2 * sumh + 2 * kA], rb0[(long)j * RS + sumh - W + k], acc);
        } else {
            for (int j = j0; j < j1; ++j) acc += rb0[(long)j * RS + 2 * sumh + 2 * kA];
        }
        slab[q] = acc;
    }
    if (tid < 3) {
        double s = 0.0;
        for (int j = j0; j < j1; ++j) s += rb0[(long)j * RS + 2 * sumh + 2 * kA + 1 + tid];
        ((double*)(ws + L.w.lslab))[(long)blockIdx.x * 3 + tid] = s;
    }
}

// one Adam step of torch.optim.Adam (single-tensor path) with the step's bias corrections from the host (optim.h: adam_bias).  The second
// moment is ONE fused multiply-add here, which rounds differently from optim.h's adam_update (a product and a sum): this learner keeps its
// own three statements so that its results stay what they were.
__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, const AdamBias& ab, float b1, float b2, float eps) {
    m = m + (1.0f - b1) * (g - m);
    v = __builtin_fmaf(v, b2, (1.0f - b2) * g * g);
    const float denom = sqrtf(v) / ab.bc2s + eps;
    p = p + (-ab.step_size) * (m / denom);
}

// trunk0 / trunk1: the trunk's two sub-steps (the parameter list holds it twice), head: the heads' one
struct PolicyBias { AdamBias trunk0, trunk1, head; };

__global__ __launch_bounds__(kAdamT) void vtb_learn_adam_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L, int m, int mb,
                                                                PolicyBias ab) {
    __shared__ double red[kAdamT];
    __shared__ float coef_s;
    const int tid = threadIdx.x;
    const int nwg = (m + kRows - 1) / kRows;
    float* ws = b.ws;
    const float* slab = ws + L.w.pslab;
    const long P = L.p.total;
    double sq = 0.0;
    for (long q = tid; q < P; q += kAdamT) {
        float g = 0.f;
        for (int k = 0; k < nwg; ++k) g += slab[(long)k * P + q];
        const double gd = g;
        sq += (q < L.p.trunk_end ? 2.0 : 1.0) * gd * gd;
    }
    sq = block_sum<kAdamT>(sq, red);
    if (tid == 0) {
        const float tn = (float)sqrt(sq);
        coef_s = c.has_max_norm ? clip_coef(tn, c.max_norm) : 1.0f;
        const double* ls = (const double*)(ws + L.w.lslab);
        double sg = 0.0, se = 0.0, sn = 0.0;
        for (int k = 0; k < nwg; ++k) {
            sg += ls[k * 3];
            se += ls[k * 3 + 1];
            sn += ls[k * 3 + 2];
        }
        const float pt = -(float)(sg / m), vt = (float)(se / m), et = (float)(sn / m);
        float* lo = b.losses + (long)mb * 4;
        lo[0] = pt + c.c_value * vt - c.c_entropy * et;
        lo[1] = pt;
        lo[2] = vt;
        lo[3] = et;
    }
    __syncthreads();
    const float coef = coef_s;
    for (long q = tid; q < P; q += kAdamT) {
        float g = 0.f;
        for (int k = 0; k < nwg; ++k) g += slab[(long)k * P + q];
        float p = b.pparams[q], mm = b.p_m[q], vv = b.p_v[q];
        if (q < L.p.trunk_end) {
            if (c.has_max_norm) g = (g * coef) * coef;
            adam_one(p, mm, vv, g, ab.trunk0, c.beta1, c.beta2, c.eps);
            adam_one(p, mm, vv, g, ab.trunk1, c.beta1, c.beta2, c.eps);
        } else {
            if (c.has_max_norm) g = g * coef;
            adam_one(p, mm, vv, g, ab.head, c.beta1, c.beta2, c.eps);
        }
        b.pparams[q] = p;
        b.p_m[q] = mm;
        b.p_v[q] = vv;
    }
}

// ---- tracker backward: one workgroup per episode -----------------------------------------------------------------------------------
// dW[o][k] += sum_p dY[p][o] X[p][k] and db[o] += sum_p dY[p][o] for a [O][K] linear over positions 0..np-1 (written, not added)
// ADD (exact-redraw mode): the pseudo-episodes of a workgroup add into its slab one after the other
template <bool ADD>
__device__ __forceinline__ void put_grad(float* g, long i, float v) {
    g[i] = ADD ? g[i] + v : v;
}

template <bool ADD>
__device__ __forceinline__ void lin_grads(float* g, long ow, long ob, const float* dY, int ldy, const float* X, int ldx, int O, int K, int np,
                                          int tid) {
    for (int i = tid; i < O * K; i += kT) {
        const int o = i / K, k = i % K;
        float acc = 0.f;
        for (int p = 0; p < np; ++p) acc = __builtin_fmaf(dY[(long)p * ldy + o], X[(long)p * ldx + k], acc);
        put_grad<ADD>(g, ow + i, acc);
    }
    for (int o = tid; o < O; o += kT) {
        float acc = 0.f;
        for (int p = 0; p < np; ++p) acc += dY[(long)p * ldy + o];
        put_grad<ADD>(g, ob + o, acc);
    }
}

// LayerNorm backward per position: dU = rs * (dy*w - mean(dy*w) - xh * mean(dy*w*xh)); dY [np][D] in, dU out
__device__ __forceinline__ void ln_bwd(const float* dY, const float* XH, const float* RS, const float* w, float* dU, int D, int np, int tid) {
    for (int p = tid; p < np; p += kT) {
        float a = 0.f, bb = 0.f;
        for (int d = 0; d < D; ++d) {
            const float g = dY[(long)p * D + d] * w[d];
            a += g;
            bb = __builtin_fmaf(g, XH[(long)p * D + d], bb);
        }
        a /= (float)D;
        bb /= (float)D;
        for (int d = 0; d < D; ++d) {
            const float g = dY[(long)p * D + d] * w[d];
            dU[(long)p * D + d] = RS[p] * (g - a - XH[(long)p * D + d] * bb);
        }
    }
}

// The backward of tracker_forward's pass over positions 0..np-1 (activations in w, masks regenerated) into the gradient slab g.
// LAST (exact-redraw mode): the upstream gradient sits on position np - 1 only, the rows whose obs is call np - 1, and g is added to.
template <bool DROP, bool LAST>
__device__ __forceinline__ void tracker_backward(const cirs_vtb_learn_cfg& c, const cirs_vtb_learn_bufs& b, const Lay& L, int e, int np,
                                                 uint32_t denv, float* w, float* g) {
    const int tid = threadIdx.x;
    const int B = c.n_env, D = c.model.dim_model, H = c.model.nhead, HD = D / H, F = c.model.d_hid, S = c.model.dim_state;
    const int NL = c.model.nlayers, Lp = L.Lp, T = c.max_turn;
    const float* tp = b.tparams;
    const uint32_t thr = DROP ? dropout_threshold(c.model.dropout_p) : 0u;
    const float inv = DROP ? 1.0f / (1.0f - c.model.dropout_p) : 1.0f;
    float* G = w + L.e.G;
    float* DU = w + L.e.DU;
    float* DH = w + L.e.DH;
    float* DFF = w + L.e.DFF;
    float* DQKV = w + L.e.DQKV;
    float* DS = w + L.e.DS;
    // dstate of each position: the sum over the sampled rows of (t = p, env e), in sample order
    for (int i = tid; i < np * S; i += kT) {
        const int p = i / S, s = i % S;
        const long key = (long)e * T + p;
        float acc = 0.f;
        if (!LAST || p == np - 1)
            for (int k = b.grad_start[key]; k < b.grad_start[key + 1]; ++k) acc += b.ws[L.w.dsrow + (long)b.grad_rows[k] * S + s];
        DS[(long)p * S + s] = acc;
    }
    __syncthreads();
    const float* XL = w + L.e.X + (long)NL * Lp * D;
    lin_grads<LAST>(g, L.t.dec_w, L.t.dec_b, DS, S, XL, D, S, D, np, tid);
    for (int i = tid; i < np * D; i += kT) {
        const int p = i / D, k = i % D;
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc = __builtin_fmaf(tp[L.t.dec_w + (long)s * D + k], DS[(long)p * S + s], acc);
        G[(long)p * D + k] = acc;
    }
    __syncthreads();
    const float qscale = 1.0f / sqrtf((float)HD);
    for (int l = NL - 1; l >= 0; --l) {
        const float* X = w + L.e.X + (long)l * Lp * D;
        const float* QKV = w + L.e.QKV[l];
        float* P = w + L.e.P[l];
        const float* PM = w + L.e.PM[l];
        const float* ATT = w + L.e.ATT[l];
        const float* XH1 = w + L.e.XH1[l];
        const float* H1 = w + L.e.H1[l];
        const float* FF = w + L.e.FF[l];
        const float* XH2 = w + L.e.XH2[l];
        // LayerNorm 2
        for (int d = tid; d < D; d += kT) {
            float a = 0.f, bb = 0.f;
            for (int p = 0; p < np; ++p) {
                a = __builtin_fmaf(G[(long)p * D + d], XH2[(long)p * D + d], a);
                bb += G[(long)p * D + d];
            }
            put_grad<LAST>(g, L.t.n2_w[l] + d, a);
            put_grad<LAST>(g, L.t.n2_b[l] + d, bb);
        }
        ln_bwd(G, XH2, w + L.e.RS2[l], tp + L.t.n2_w[l], DU, D, np, tid);
        __syncthreads();
        // DU = du2; df2 = du2 * m_res2 (staged in G, which is free now)
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, o = i % D;
            float v = DU[i];
            if (DROP) v = LEARN_KEEP(p, l, CIRS_DROP_RES2, o) ? v * inv : 0.f;
            G[i] = v;
        }
        __syncthreads();
        // dFF (pre-ReLU, through the FF mask), linear2 grads use the masked FF
        for (int i = tid; i < np * F; i += kT) {
            const int p = i / F, f = i % F;
            float acc = 0.f;
            for (int o = 0; o < D; ++o) acc = __builtin_fmaf(tp[L.t.l2_w[l] + (long)o * F + f], G[(long)p * D + o], acc);
            const float msk = DROP ? (LEARN_KEEP(p, l, CIRS_DROP_FF, f) ? inv : 0.f) : 1.0f;
            DFF[i] = FF[i] > 0.f ? acc * msk : 0.f;
        }
        for (int i = tid; i < D * F; i += kT) {
            const int o = i / F, f = i % F;
            float acc = 0.f;
            for (int p = 0; p < np; ++p) {
                float fv = FF[(long)p * F + f];
                if (DROP) fv = LEARN_KEEP(p, l, CIRS_DROP_FF, f) ? fv * inv : 0.f;
                acc = __builtin_fmaf(G[(long)p * D + o], fv, acc);
            }
            put_grad<LAST>(g, L.t.l2_w[l] + i, acc);
        }
        for (int o = tid; o < D; o += kT) {
            float acc = 0.f;
            for (int p = 0; p < np; ++p) acc += G[(long)p * D + o];
            put_grad<LAST>(g, L.t.l2_b[l] + o, acc);
        }
        __syncthreads();
        lin_grads<LAST>(g, L.t.l1_w[l], L.t.l1_b[l], DFF, F, H1, D, F, D, np, tid);
        // dH1 = du2 + W1^T dFF
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, k = i % D;
            float acc = DU[i];
            for (int f = 0; f < F; ++f) acc = __builtin_fmaf(tp[L.t.l1_w[l] + (long)f * D + k], DFF[(long)p * F + f], acc);
            DH[i] = acc;
        }
        __syncthreads();
        // LayerNorm 1
        for (int d = tid; d < D; d += kT) {
            float a = 0.f, bb = 0.f;
            for (int p = 0; p < np; ++p) {
                a = __builtin_fmaf(DH[(long)p * D + d], XH1[(long)p * D + d], a);
                bb += DH[(long)p * D + d];
            }
            put_grad<LAST>(g, L.t.n1_w[l] + d, a);
            put_grad<LAST>(g, L.t.n1_b[l] + d, bb);
        }
        ln_bwd(DH, XH1, w + L.e.RS1[l], tp + L.t.n1_w[l], DU, D, np, tid);
        __syncthreads();
        // DU = du1 (also the residual gradient of X); dsa = du1 * m_res1 -> G
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, o = i % D;
            float v = DU[i];
            if (DROP) v = LEARN_KEEP(p, l, CIRS_DROP_RES1, o) ? v * inv : 0.f;
            G[i] = v;
        }
        __syncthreads();
        lin_grads<LAST>(g, L.t.out_w[l], L.t.out_b[l], G, D, ATT, D, D, D, np, tid);
        // dATT -> DH
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, k = i % D;
            float acc = 0.f;
            for (int o = 0; o < D; ++o) acc = __builtin_fmaf(tp[L.t.out_w[l] + (long)o * D + k], G[(long)p * D + o], acc);
            DH[i] = acc;
        }
        __syncthreads();
        // dV_j = sum_{i >= j} PM_ij dATT_i
        for (int i = tid; i < np * D; i += kT) {
            const int j = i / D, d = i % D, h = d / HD;
            float acc = 0.f;
            for (int q = j; q < np; ++q) acc = __builtin_fmaf(PM[((long)h * Lp + q) * Lp + j], DH[(long)q * D + d], acc);
            DQKV[(long)j * 3 * D + 2 * D + d] = acc;
        }
        // dS_ij = P_ij (dP_ij - sum_k P_ik dP_ik), dP_ij = (dATT_i . V_j) * mask_ij; overwrites P
        for (int i = tid; i < np * H; i += kT) {
            const int q = i / H, h = i % H;
            float* pr = P + ((long)h * Lp + q) * Lp;
            float dot = 0.f;
            for (int j = 0; j <= q; ++j) {
                float dp = 0.f;
                for (int d = 0; d < HD; ++d) dp = __builtin_fmaf(DH[(long)q * D + h * HD + d], QKV[(long)j * 3 * D + 2 * D + h * HD + d], dp);
                if (DROP) dp = LEARN_KEEP(q, l, CIRS_DROP_ATTN, j * H + h) ? dp * inv : 0.f;
                dot = __builtin_fmaf(pr[j], dp, dot);
            }
            // second sweep: recompute dp (cheap) and write dS
            for (int j = 0; j <= q; ++j) {
                float dp = 0.f;
                for (int d = 0; d < HD; ++d) dp = __builtin_fmaf(DH[(long)q * D + h * HD + d], QKV[(long)j * 3 * D + 2 * D + h * HD + d], dp);
                if (DROP) dp = LEARN_KEEP(q, l, CIRS_DROP_ATTN, j * H + h) ? dp * inv : 0.f;
                pr[j] = pr[j] * (dp - dot);
            }
        }
        __syncthreads();
        // dQ_i = scale * sum_j dS_ij K_j ; dK_j = scale * sum_{i >= j} dS_ij Q_i
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, d = i % D, h = d / HD;
            float aq = 0.f, ak = 0.f;
            for (int j = 0; j <= p; ++j) aq = __builtin_fmaf(P[((long)h * Lp + p) * Lp + j], QKV[(long)j * 3 * D + D + d], aq);
            for (int q = p; q < np; ++q) ak = __builtin_fmaf(P[((long)h * Lp + q) * Lp + p], QKV[(long)q * 3 * D + d], ak);
            DQKV[(long)p * 3 * D + d] = aq * qscale;
            DQKV[(long)p * 3 * D + D + d] = ak * qscale;
        }
        __syncthreads();
        lin_grads<LAST>(g, L.t.in_w[l], L.t.in_b[l], DQKV, 3 * D, X, D, 3 * D, D, np, tid);
        // dX = du1 + W_in^T dQKV -> G (the next layer down's output gradient)
        for (int i = tid; i < np * D; i += kT) {
            const int p = i / D, k = i % D;
            float acc = DU[i];
            for (int o = 0; o < 3 * D; ++o) acc = __builtin_fmaf(tp[L.t.in_w[l] + (long)o * D + k], DQKV[(long)p * 3 * D + o], acc);
            DH[i] = acc;
        }
        __syncthreads();
        for (int i = tid; i < np * D; i += kT) G[i] = DH[i];
        __syncthreads();
    }
    // PE dropout and the sqrt(D) scale -> d slot (DH)
    const float sqd = sqrtf((float)D);
    for (int i = tid; i < np * D; i += kT) {
        const int p = i / D, d = i % D;
        float v = G[i];
        if (DROP) v = LEARN_KEEP(p, 0, CIRS_DROP_POS, d) ? v * inv : 0.f;
        DH[i] = v * sqd;
    }
    __syncthreads();
    // slot 0: ffn_user
    const double* o0 = b.obs0 + (long)e * kObs0;
    for (int i = tid; i < D * kU; i += kT) put_grad<LAST>(g, L.t.user_w + i, DH[i / kU] * (float)o0[i % kU]);
    for (int d = tid; d < D; d += kT) put_grad<LAST>(g, L.t.user_b + d, DH[d]);
    // slots 1..np-1: x = sigmoid(gate) * a; dgate = dx * a * s (1 - s) -> DU
    const float* SIG = w + L.e.SIG;
    for (int i = tid; i < np * D; i += kT) {
        const int p = i / D, d = i % D;
        if (p == 0) {
            DU[i] = 0.f;
            continue;
        }
        const float a = (float)b.obs[((long)(p - 1) * B + e) * kObs + d];
        const float s = SIG[i];
        DU[i] = DH[i] * a * (s * (1.0f - s));
    }
    __syncthreads();
    for (int i = tid; i < D * (1 + kA); i += kT) {
        const int o = i / (1 + kA), k = i % (1 + kA);
        float acc = 0.f;
        for (int p = 1; p < np; ++p) {
            const long row = (long)(p - 1) * B + e;
            const float x = k == 0 ? (float)b.rew[row] : (float)b.obs[row * kObs + k - 1];
            acc = __builtin_fmaf(DU[(long)p * D + o], x, acc);
        }
        put_grad<LAST>(g, L.t.gate_w + i, acc);
    }
    for (int o = tid; o < D; o += kT) {
        float acc = 0.f;
        for (int p = 1; p < np; ++p) acc += DU[(long)p * D + o];
        put_grad<LAST>(g, L.t.gate_b + o, acc);
    }
}

// position-keyed mode: one workgroup per episode; the obs positions 0..len-1 carry gradient
template <bool DROP>
__global__ __launch_bounds__(kT) void vtb_learn_tracker_bwd_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L) {
    const int e = blockIdx.x;
    tracker_backward<DROP, false>(c, b, L, e, b.len[e], (uint32_t)(c.model.drop_env_base + e), b.ws + L.w.env + (long)e * L.e.total,
                                  b.ws + L.w.tslab + (long)e * L.t.total);
}

// exact-redraw mode: workgroup (e, g) runs forward and backward of the calls c = g, g + groups, ... < len of env e that have sampled rows
// (call len is only ever an obs_next), in this fixed order, adding into its own slab (zeroed by the caller)
__global__ __launch_bounds__(kT) void vtb_learn_tracker_redraw_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L) {
    const int e = blockIdx.x / L.groups, g = blockIdx.x % L.groups;
    float* w = b.ws + L.w.env + (long)blockIdx.x * L.e.total;
    float* slab = b.ws + L.w.tslab + (long)blockIdx.x * L.t.total;
    const int len = b.len[e];
    for (int call = g; call < len; call += L.groups) {
        const long key = (long)e * c.max_turn + call;
        if (b.grad_start[key] == b.grad_start[key + 1]) continue;      // workgroup-uniform
        const uint32_t denv = (uint32_t)(c.model.drop_env_base + call * c.n_env + e);
        tracker_forward<true, true>(c, b, L, e, call + 1, denv, w);
        __syncthreads();
        tracker_backward<true, true>(c, b, L, e, call + 1, denv, w, slab);
        __syncthreads();
    }
}
#undef LEARN_KEEP

__global__ __launch_bounds__(256) void vtb_learn_tracker_adam_kernel(cirs_vtb_learn_cfg c, cirs_vtb_learn_bufs b, Lay L, AdamBias ab) {
    const long P = L.t.total;
    const float* slab = b.ws + L.w.tslab;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < P; q += (long)gridDim.x * blockDim.x) {
        float g = 0.f;
        for (int e = 0; e < L.n_wg; ++e) g += slab[(long)e * P + q];
        float p = b.tparams[q], m = b.t_m[q], v = b.t_v[q];
        adam_one(p, m, v, g, ab, c.t_beta1, c.t_beta2, c.t_eps);
        b.tparams[q] = p;
        b.t_m[q] = m;
        b.t_v[q] = v;
    }
}

int validate(const cirs_vtb_learn_cfg* c) {
    CIRS_REQUIRE(c != nullptr, "null learn cfg");
    CIRS_REQUIRE(c->n_env >= 1 && c->max_turn >= 1, "n_env and max_turn must be >= 1");
    if (int rc = vtb_validate_model(&c->model, c->max_turn)) return rc;
    CIRS_REQUIRE(c->model.d_hid >= 1 && c->model.d_hid <= 1024, "d_hid must lie in [1, 1024]");
    CIRS_REQUIRE(c->model.dim_state >= 1 && c->model.dim_state <= kMaxW, "dim_state must lie in [1, 128]");
    CIRS_REQUIRE(c->n_rows >= 1, "n_rows must be >= 1");
    CIRS_REQUIRE(c->n_seg >= 1 && c->n_seg <= c->n_rows, "n_seg must lie in [1, n_rows]");
    return CIRS_OK;
}

int validate_bufs(const cirs_vtb_learn_bufs* b) {
    CIRS_REQUIRE(b && b->tparams && b->t_m && b->t_v && b->pparams && b->p_m && b->p_v && b->pe && b->obs0 && b->obs && b->rew && b->done &&
                     b->act && b->len && b->rows && b->boundary && b->seg_end && b->grad_rows && b->grad_start && b->rms && b->ws,
                 "null learn buffer");
    return CIRS_OK;
}

int returns_stage(const cirs_vtb_learn_cfg& c, const cirs_vtb_learn_bufs& b, const Lay& L, int want_logp, hipStream_t s) {
    hipLaunchKernelGGL(vtb_learn_values_kernel, dim3(cdiv(c.n_rows, kVW)), dim3(64 * kVW), 0, s, c, b, L, want_logp);
    CIRS_CHECK_LAUNCH("vtb_learn_values_kernel");
    hipLaunchKernelGGL(vtb_learn_gae_kernel, dim3(cdiv(c.n_seg, 256)), dim3(256), 0, s, c, b, L);
    CIRS_CHECK_LAUNCH("vtb_learn_gae_kernel");
    if (c.scale_returns) {
        hipLaunchKernelGGL(vtb_learn_rms_kernel, dim3(1), dim3(256), 0, s, c, b, L);
        CIRS_CHECK_LAUNCH("vtb_learn_rms_kernel");
    }
    return CIRS_OK;
}

// what the exact-redraw mode adds to validate
int validate_redraw(const cirs_vtb_learn_cfg* c) {
    CIRS_REQUIRE((long)c->model.drop_env_base + ((long)c->max_turn + 1) * c->n_env < (1L << 31),
                 "dropout_redraw: drop_env_base + (max_turn + 1) * n_env must be < 2^31 (call c of env e draws dropout env id "
                 "drop_env_base + c * n_env + e)");
    return CIRS_OK;
}

int sizes(const cirs_vtb_learn_cfg* cfg, bool redraw, int64_t* out) {
    CIRS_REQUIRE(out != nullptr, "null output");
    const Lay L = make_layout(*cfg, redraw);
    out[0] = L.t.total;
    out[1] = L.p.total;
    out[2] = L.w.total;
    out[3] = L.w.states;
    out[4] = L.w.vs;
    return CIRS_OK;
}

int prepare(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, bool redraw, hipStream_t s) {
    const Lay L = make_layout(*cfg, redraw);
    if (redraw) hipLaunchKernelGGL(vtb_learn_forward_redraw_kernel, dim3(L.n_wg), dim3(kT), 0, s, *cfg, *b, L);
    else if (cfg->model.dropout_p > 0.f) hipLaunchKernelGGL(vtb_learn_forward_kernel<true>, dim3(cfg->n_env), dim3(kT), 0, s, *cfg, *b, L);
    else hipLaunchKernelGGL(vtb_learn_forward_kernel<false>, dim3(cfg->n_env), dim3(kT), 0, s, *cfg, *b, L);
    CIRS_CHECK_LAUNCH("vtb_learn_forward_kernel");
    return returns_stage(*cfg, *b, L, 1, s);
}

int update(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, bool redraw, const int32_t* perms, int32_t repeat, int32_t batch_size,
           int32_t recompute_adv, int64_t p_step0, int64_t t_step0, hipStream_t s) {
    CIRS_REQUIRE(perms != nullptr && b->losses != nullptr, "null permutations / losses");
    CIRS_REQUIRE(repeat >= 1 && batch_size >= 1, "repeat and batch_size must be >= 1");
    CIRS_REQUIRE(p_step0 >= 0 && t_step0 >= 0, "step counts must be >= 0");
    const cirs_vtb_learn_cfg c = *cfg;
    const Lay L = make_layout(c, redraw);
    const int n = c.n_rows;
    // row_ranges(n, batch_size): a short tail joins the range before it
    const int full = n / batch_size;
    const int n_mb = (full >= 1 && n % batch_size) ? full : (n + batch_size - 1) / batch_size;
    int mb = 0;
    for (int pass = 0; pass < repeat; ++pass) {
        if (recompute_adv && pass > 0)
            if (int rc = returns_stage(c, *b, L, 0, s)) return rc;
        const int32_t* perm = perms + (long)pass * n;
        for (int k = 0; k < n_mb; ++k, ++mb) {
            const int a = k * batch_size, e = k == n_mb - 1 ? n : a + batch_size;
            const int m = e - a;
            hipLaunchKernelGGL(vtb_learn_minibatch_kernel, dim3(cdiv(m, kRows)), dim3(kT), 0, s, c, *b, L, perm + a, m, pass == repeat - 1 ? 1 : 0);
            CIRS_CHECK_LAUNCH("vtb_learn_minibatch_kernel");
            const PolicyBias ab = {adam_bias(c.lr, c.beta1, c.beta2, 2 * p_step0 + 2 * mb + 1), adam_bias(c.lr, c.beta1, c.beta2, 2 * p_step0 + 2 * mb + 2),
                                   adam_bias(c.lr, c.beta1, c.beta2, p_step0 + mb + 1)};
            hipLaunchKernelGGL(vtb_learn_adam_kernel, dim3(1), dim3(kAdamT), 0, s, c, *b, L, m, mb, ab);
            CIRS_CHECK_LAUNCH("vtb_learn_adam_kernel");
        }
    }
    if (redraw) {
        CIRS_HIP(hipMemsetAsync(b->ws + L.w.tslab, 0, (size_t)L.n_wg * L.t.total * sizeof(float), s));
        hipLaunchKernelGGL(vtb_learn_tracker_redraw_kernel, dim3(L.n_wg), dim3(kT), 0, s, c, *b, L);
    } else if (c.model.dropout_p > 0.f) {
        hipLaunchKernelGGL(vtb_learn_tracker_bwd_kernel<true>, dim3(c.n_env), dim3(kT), 0, s, c, *b, L);
    } else {
        hipLaunchKernelGGL(vtb_learn_tracker_bwd_kernel<false>, dim3(c.n_env), dim3(kT), 0, s, c, *b, L);
    }
    CIRS_CHECK_LAUNCH("vtb_learn_tracker_bwd_kernel");
    const int g = cdiv(L.t.total, 256);
    hipLaunchKernelGGL(vtb_learn_tracker_adam_kernel, dim3(g < 1024 ? g : 1024), dim3(256), 0, s, c, *b, L,
                       adam_bias(c.t_lr, c.t_beta1, c.t_beta2, t_step0 + 1));
    CIRS_CHECK_LAUNCH("vtb_learn_tracker_adam_kernel");
    return CIRS_OK;
}

}  // namespace
}  // namespace cirs

extern "C" int cirs_vtb_learn_sizes(const cirs_vtb_learn_cfg* cfg, int64_t* out) {
    using namespace cirs;
    if (int rc = validate(cfg)) return rc;
    return sizes(cfg, false, out);
}

// replaces core/host_rl.py HostPPOPolicy._returns_stage + process_fn (:255-283) and the graph of vtb_host.tracker_states
extern "C" int cirs_vtb_learn_prepare(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, void* stream) {
    using namespace cirs;
    if (int rc = validate(cfg)) return rc;
    if (int rc = validate_bufs(b)) return rc;
    return prepare(cfg, b, false, (hipStream_t)stream);
}

// replaces core/host_rl.py HostPPOPolicy.learn (:286-316): ppo_objective + backward + clip_grad_norm_ + optim_RL.step per minibatch,
// optim_state.step once at the end on the last pass's tracker gradient
extern "C" int cirs_vtb_learn_update(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, const int32_t* perms, int32_t repeat,
                                     int32_t batch_size, int32_t recompute_adv, int64_t p_step0, int64_t t_step0, void* stream) {
    using namespace cirs;
    if (int rc = validate(cfg)) return rc;
    if (int rc = validate_bufs(b)) return rc;
    return update(cfg, b, false, perms, repeat, batch_size, recompute_adv, p_step0, t_step0, (hipStream_t)stream);
}

// ---- exact-redraw mode ---------------------------------------------------------------------------------------------------------
// The three calls above for a buffer of cirs_vtb_rollout_collect_redraw: the state of row (t, e) is call t's, of its obs_next call
// t + 1's, and the tracker gradient goes through each call's own graph (reference core/state_tracker.py:170-250: one build_state call,
// one retained graph; vtb_host.redraw_states).  Without dropout the calls coincide with the single causal pass: that one runs.
extern "C" int cirs_vtb_learn_redraw_sizes(const cirs_vtb_learn_cfg* cfg, int64_t* out) {
    using namespace cirs;
    if (int rc = validate(cfg)) return rc;
    if (int rc = validate_redraw(cfg)) return rc;
    return sizes(cfg, cfg->model.dropout_p > 0.f, out);
}

extern "C" int cirs_vtb_learn_prepare_redraw(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, void* stream) {
    using namespace cirs;
    if (int rc = validate(cfg)) return rc;
    if (int rc = validate_redraw(cfg)) return rc;
    if (int rc = validate_bufs(b)) return rc;
    return prepare(cfg, b, cfg->model.dropout_p > 0.f, (hipStream_t)stream);
}

extern "C" int cirs_vtb_learn_update_redraw(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, const int32_t* perms, int32_t repeat,
                                            int32_t batch_size, int32_t recompute_adv, int64_t p_step0, int64_t t_step0, void* stream) {
    using namespace cirs;
    if (int rc = validate(cfg)) return rc;
    if (int rc = validate_redraw(cfg)) return rc;
    if (int rc = validate_bufs(b)) return rc;
    return update(cfg, b, cfg->model.dropout_p > 0.f, perms, repeat, batch_size, recompute_adv, p_step0, t_step0, (hipStream_t)stream);
}
