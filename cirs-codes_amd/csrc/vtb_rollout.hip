// vtb_rollout.hip -- the policy side of the VirtualTaobao PPO rollout (CIRS-RL-taobao.py) on gfx950.
//
// Per vector step t, vtb_policy_step_kernel runs one 64-lane wavefront per env of the previous step's active list:
//   record      the env step t-1 of this env (obs, reward, done, CTR) into the trajectory; force_length overrides done
//   input slot  t = 0: x = ffn_user(obs0[:88]); t > 0: x = sigmoid(fnn_gate([r, a])) * a, a = the 27 action columns of obs
//               (core/host_rl.py HostStateTracker.build_state, same order of operations)
//   decode      h = x * sqrt(D) + pe[t]; nlayers post-norm TransformerEncoderLayers with per-layer K/V caches (causal attention of
//               position t over 0..t), decoder -> state s_t (traj.state[t])
//   actor       envs that are not done: Net trunk (ReLU), mu = max_action * tanh(head) (or the head when unbounded), sigma = exp(param)
//               or exp(clamp(head, -20, 2)); act = mu + sigma * z, z ~ N(0, 1) (Box-Muller on Philox, see gauss_z); the raw act goes
//               to traj.act, the mapped action (HostPPOPolicy.map_action: clip / tanh, then scaled to the box) to the env's action
//               buffer at a compacted position of the next active list (one atomic per env)
// and then vtb_step_kernel (csrc/virtualtb.hip) steps the envs of that list.  The rows of an env do not depend on its position in the
// list, so the order the atomics produce changes no result.
//
// Dropout (DROP): the production mode of csrc/rng.h, position-keyed masks at the five sites of tracker.hip with its element
// convention (ATTN: key_pos * nhead + head); a cached position keeps its masks for the rest of the episode.
// Exact redraw (cirs_vtb_rollout_collect_redraw): call t runs the prefix 0..t again with masks of its own, as the reference's tracker in
// train() does; vtb_policy_step_redraw_kernel below, built from the same row functions, so call 0 equals the decode's bit for bit.
// fp32 throughout; matrices are [in][out] so that the lanes of a mat-vec read consecutive floats; the weights stay in L2.
#include "common.h"
#include "rng.h"
#include "vtb_model.h"

#define CIRS_RNG_STREAM_GAUSS 0x47415553u /* 'GAUS' */

namespace cirs {
namespace {

constexpr int kWaves = 4;
constexpr int kMaxD = 64, kMaxHid = 256, kMaxW = 128, kMaxAttn = 2048;
constexpr int kA = CIRS_VTB_ACTION_DIM, kU = CIRS_VTB_USER_DIM, kObs = kA + 3, kObs0 = kU + 3;
// per-wave LDS: xs, qs, ks, vs, att, h1 [64 each] | ff [256] | hb, hc [128 each] | head norms [64] | scores [nhead * max_len]
constexpr int kFixed = 6 * kMaxD + kMaxHid + 2 * kMaxW + kMaxD;

// ---- Gaussian noise ---------------------------------------------------------------------------------------------------
// sin / cos of x in [0, pi/2): Taylor polynomials in x^2 (truncation < 6e-8 at pi/2), fixed fmaf order
__host__ __device__ __forceinline__ float det_sin_q(float x) {
    const float z = x * x;
    float p = -2.5052108385e-8f;
    p = __builtin_fmaf(p, z, 2.7557319224e-6f);
    p = __builtin_fmaf(p, z, -1.9841269841e-4f);
    p = __builtin_fmaf(p, z, 8.3333333333e-3f);
    p = __builtin_fmaf(p, z, -1.6666666667e-1f);
    p = __builtin_fmaf(p, z, 1.0f);
    return x * p;
}
__host__ __device__ __forceinline__ float det_cos_q(float x) {
    const float z = x * x;
    float p = 2.0876756988e-9f;
    p = __builtin_fmaf(p, z, -2.7557319224e-7f);
    p = __builtin_fmaf(p, z, 2.4801587302e-5f);
    p = __builtin_fmaf(p, z, -1.3888888889e-3f);
    p = __builtin_fmaf(p, z, 4.1666666667e-2f);
    p = __builtin_fmaf(p, z, -0.5f);
    p = __builtin_fmaf(p, z, 1.0f);
    return p;
}

// z of (env, t, dim): see include/cirs_hip.h cirs_vtb_rollout_noise
__device__ __forceinline__ float gauss_z(uint64_t seed, uint32_t collect_id, uint32_t env, uint32_t t, uint32_t dim) {
    const u32x4 r = philox4x32_10(dim >> 2, env, t, collect_id, (uint32_t)seed ^ CIRS_RNG_STREAM_GAUSS, (uint32_t)(seed >> 32));
    const bool hi = (dim & 2u) != 0;
    const float u1 = u01_from_bits(hi ? r.z : r.x), u2 = u01_from_bits(hi ? r.w : r.y);
    const float rad = sqrtf(-2.0f * det_logf(u1));
    const float v = u2 * 4.0f;                     // exact
    const int q = (int)v;                          // quadrant 0..3
    const float x = (v - (float)q) * 1.5707963267948966f;
    const float s = det_sin_q(x), c = det_cos_q(x);
    const float cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;   // cos(2 pi u2)
    const float sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;   // sin(2 pi u2)
    return rad * ((dim & 1u) ? sn : cs);
}

// ---- wave helpers -------------------------------------------------------------------------------------------------------
// b[o] + sum_k W[k][o] x[k] for the output o of this lane (o < O is the caller's business)
__device__ __forceinline__ float mv(const float* __restrict__ W, const float* __restrict__ b, const float* x, int K, int O, int o) {
    float acc = b ? b[o] : 0.f;
#pragma unroll 8
    for (int k = 0; k < K; ++k) acc = __builtin_fmaf(W[(size_t)k * O + o], x[k], acc);
    return acc;
}

// LayerNorm over the D values of lanes 0..D-1 (torch: biased variance, eps 1e-5); other lanes get 0
__device__ __forceinline__ float layer_norm(float v, int lane, int D, const float* __restrict__ w, const float* __restrict__ b) {
    const bool on = lane < D;
    const float mean = wave_sum_f32(on ? v : 0.f) / (float)D;
    const float d = v - mean;
    const float var = wave_sum_f32(on ? d * d : 0.f) / (float)D;
    return on ? d / sqrtf(var + 1e-5f) * w[lane] + b[lane] : 0.f;
}

__device__ __forceinline__ void wbar() { __builtin_amdgcn_wave_barrier(); }

// the LDS of one wave
struct WaveLds {
    float *xs, *qs, *ks, *vs, *att, *h1s, *ffs, *hb, *hc, *hinv, *ps;
};
__device__ __forceinline__ WaveLds wave_lds(float* smem, int wv, int H, int L) {
    float* base = smem + (size_t)wv * (kFixed + H * L);
    WaveLds s;
    s.xs = base;
    s.qs = base + kMaxD;
    s.ks = base + 2 * kMaxD;
    s.vs = base + 3 * kMaxD;
    s.att = base + 4 * kMaxD;
    s.h1s = base + 5 * kMaxD;
    s.ffs = base + 6 * kMaxD;
    s.hb = s.ffs + kMaxHid;
    s.hc = s.hb + kMaxW;
    s.hinv = s.hc + kMaxW;
    s.ps = s.hinv + kMaxD;
    return s;
}

// the dropout key of one pass: the masks of (dropout env id, position, layer, site, element) under the collect's key
struct DropKey {
    uint64_t seed;
    uint32_t env, thr;
    float inv;
};
__device__ __forceinline__ DropKey drop_key(const cirs_vtb_model_cfg& m, uint32_t env, bool on) {
    DropKey k;
    k.seed = m.dropout_seed;
    k.env = env;
    k.thr = on ? dropout_threshold(m.dropout_p) : 0u;
    k.inv = on ? 1.0f / (1.0f - m.dropout_p) : 1.0f;
    return k;
}
#define VTB_DROP(V, LAYER, SITE, ELEM) \
    (dropout_keep(dk.seed, dk.env, (uint32_t)pos, (uint32_t)(LAYER), (uint32_t)(SITE), (uint32_t)(ELEM), dk.thr) ? (V) * dk.inv : 0.f)

// ---- record the env step t-1 of env e (list position j) and build the input slot t (lanes < D) ---------------------------
__device__ __forceinline__ float record_and_slot(const cirs_vtb_rollout_cfg& cfg, const cirs_vtb_policy_weights& w, const cirs_vtb_traj& tr,
                                                 const WaveLds& s, int t, int steps, int j, int e, int lane, bool& finished) {
    const int B = cfg.n_env, D = cfg.model.dim_model;
    float* hc = s.hc;
    finished = false;
    float x = 0.f;
    if (t == 0) {
        const double* o0 = tr.obs0 + (size_t)e * kObs0;
        if (lane < kU) hc[lane] = (float)o0[lane];                 // the last 3 entries are not user features
        if (lane + 64 < kU) hc[64 + lane] = (float)o0[64 + lane];
        wbar();
        if (lane < D) x = mv(w.user_w, w.user_b, hc, kU, D, lane);
    } else {
        const size_t row = (size_t)(t - 1) * B + e;
        const double* so = tr.step_obs + (size_t)j * kObs;
        if (lane < kObs) tr.obs[row * kObs + lane] = so[lane];
        const double r64 = tr.step_rew[j];
        const bool done = cfg.force_length > 0 ? t >= cfg.force_length : tr.step_done[j] != 0;
        finished = done || t >= steps;
        if (lane == 0) {
            tr.rew[row] = r64;
            tr.ctr[row] = tr.step_ctr[j];
            tr.done[row] = (uint8_t)done;
            if (finished) tr.len[e] = t;
        }
        // gate input [r, a_0..a_26]: hc[0] = r (the fp64 reward rounded once), hc[1 + k] = a_k
        if (lane < kA) hc[1 + lane] = (float)so[lane];
        if (lane == 0) hc[0] = (float)r64;
        wbar();
        if (lane < D) {
            const float g = mv(w.gate_w, w.gate_b, hc, 1 + kA, D, lane);
            x = (1.0f / (1.0f + expf(-g))) * hc[1 + lane];     // sigmoid(gate) * a_t, feature-wise (D == 27)
        }
    }
    wbar();
    return x;
}

// the encoder's input row at position pos from the slot x: x * sqrt(D) + pe[pos], PE-output dropout
template <bool DROP>
__device__ __forceinline__ float embed_row(const cirs_vtb_policy_weights& w, const DropKey& dk, float x, int pos, int D, int lane) {
    float h = 0.f;
    if (lane < D) {
        h = x * sqrtf((float)D) + w.pe[(size_t)pos * D + lane];
        if (DROP) h = VTB_DROP(h, 0, CIRS_DROP_POS, lane);
    }
    return h;
}

// ---- one post-norm TransformerEncoderLayer for the row at position pos ----------------------------------------------------
// h (lanes < D) in, the layer's output back.  Causal attention of pos over 0..pos: the row's own K/V from LDS, rows 0..pos-1 from
// kc / vc [max_len][D]; STORE_KV also writes the row's K/V there (the decode's cache).
template <bool DROP, bool STORE_KV>
__device__ __forceinline__ float encoder_row(const cirs_vtb_model_cfg& m, const cirs_vtb_policy_layer& ly, const WaveLds& s, const DropKey& dk,
                                             int l, int pos, float h, float* kc, float* vc, int lane) {
    const int D = m.dim_model, H = m.nhead, HD = D / H, L = m.max_len;
    float *xs = s.xs, *qs = s.qs, *ks = s.ks, *vs = s.vs, *att = s.att, *h1s = s.h1s, *ffs = s.ffs, *hinv = s.hinv, *ps = s.ps;
    const float qscale = 1.0f / sqrtf((float)HD);
    if (lane < D) xs[lane] = h;
    wbar();
    if (lane < D) {
        const float q = mv(ly.in_w, ly.in_b, xs, D, 3 * D, lane);
        const float k = mv(ly.in_w, ly.in_b, xs, D, 3 * D, D + lane);
        const float v = mv(ly.in_w, ly.in_b, xs, D, 3 * D, 2 * D + lane);
        qs[lane] = q * qscale;
        ks[lane] = k;
        vs[lane] = v;
        if (STORE_KV) {
            kc[(size_t)pos * D + lane] = k;
            vc[(size_t)pos * D + lane] = v;
        }
    }
    wbar();
    // causal attention of position pos over 0..pos, one head after the other; lanes stride over the key positions
    for (int hh = 0; hh < H; ++hh) {
        float mx = -INFINITY;
        for (int jp = lane; jp <= pos; jp += 64) {
            const float* kr = jp == pos ? ks : kc + (size_t)jp * D;
            float sc = 0.f;
            for (int d = 0; d < HD; ++d) sc = __builtin_fmaf(qs[hh * HD + d], kr[hh * HD + d], sc);
            ps[hh * L + jp] = sc;
            mx = fmaxf(mx, sc);
        }
        mx = wave_max_f32(mx);
        float sm = 0.f;
        for (int jp = lane; jp <= pos; jp += 64) {
            const float ex = expf(ps[hh * L + jp] - mx);
            sm += ex;
            // attention-probability dropout acts after the softmax: the normaliser sums the unmasked terms
            ps[hh * L + jp] = DROP ? VTB_DROP(ex, l, CIRS_DROP_ATTN, jp * H + hh) : ex;
        }
        sm = wave_sum_f32(sm);
        if (lane == 0) hinv[hh] = 1.0f / sm;
    }
    wbar();
    if (lane < D) {
        const int hh = lane / HD;
        const float* pr = ps + hh * L;
        float acc = 0.f;
#pragma unroll 4
        for (int jp = 0; jp < pos; ++jp) acc = __builtin_fmaf(pr[jp], vc[(size_t)jp * D + lane], acc);
        acc = __builtin_fmaf(pr[pos], vs[lane], acc);
        att[lane] = acc * hinv[hh];
    }
    wbar();
    // out_proj + residual + LayerNorm 1
    float sa = lane < D ? mv(ly.out_w, ly.out_b, att, D, D, lane) : 0.f;
    if (DROP && lane < D) sa = VTB_DROP(sa, l, CIRS_DROP_RES1, lane);
    const float h1 = layer_norm(h + sa, lane, D, ly.norm1_w, ly.norm1_b);
    if (lane < D) h1s[lane] = h1;
    wbar();
    // feed-forward (ReLU) + residual + LayerNorm 2
    for (int i = lane; i < m.d_hid; i += 64) {
        float f = fmaxf(mv(ly.lin1_w, ly.lin1_b, h1s, D, m.d_hid, i), 0.f);
        if (DROP) f = VTB_DROP(f, l, CIRS_DROP_FF, i);
        ffs[i] = f;
    }
    wbar();
    float f2 = lane < D ? mv(ly.lin2_w, ly.lin2_b, ffs, m.d_hid, D, lane) : 0.f;
    if (DROP && lane < D) f2 = VTB_DROP(f2, l, CIRS_DROP_RES2, lane);
    const float out = layer_norm(h1 + f2, lane, D, ly.norm2_w, ly.norm2_b);
    wbar();
    return out;
}
#undef VTB_DROP

// ---- decoder on the encoder's output row h of position t, then the actor ---------------------------------------------------
// state s_t -> traj.state; unless the env has finished: Net trunk, mu / sigma, act = mu + sigma * z, the mapped action at a compacted
// position of the next active list
// GREEDY (deterministic_eval in eval mode, reference core/policy/ppo.py:152-153): act = mu, no z is drawn
template <bool GREEDY>
__device__ __forceinline__ void decode_and_act(const cirs_vtb_rollout_cfg& cfg, const cirs_vtb_policy_weights& w, const cirs_vtb_traj& tr,
                                               const WaveLds& sl, float h, int t, int e, int lane, bool finished, uint64_t seed,
                                               uint32_t collect_id) {
    const int B = cfg.n_env, D = cfg.model.dim_model, S = cfg.model.dim_state;
    float *xs = sl.xs, *hb = sl.hb, *hc = sl.hc;
    if (lane < D) xs[lane] = h;
    wbar();
    float s = 0.f;
    if (lane < S) {
        s = mv(w.dec_w, w.dec_b, xs, D, S, lane);
        tr.state[((size_t)t * B + e) * S + lane] = s;
    }
    if (finished) return;      // wave-uniform

    if (lane < S) hb[lane] = s;
    wbar();
    float* in = hb;
    float* out = hc;
    int width = S;
    for (int li = 0; li < cfg.model.n_hidden; ++li) {
        const int O = cfg.model.hidden[li];
        for (int o = lane; o < O; o += 64) out[o] = fmaxf(mv(w.trunk_w[li], w.trunk_b[li], in, width, O, o), 0.f);
        wbar();
        float* tmp = in;
        in = out;
        out = tmp;
        width = O;
    }
    if (lane < kA) {
        const float pre = mv(w.mu_w, w.mu_b, in, width, kA, lane);
        const float mu = cfg.model.unbounded ? pre : cfg.model.max_action * tanhf(pre);
        float sigma;
        if (cfg.model.conditioned_sigma) sigma = expf(fminf(fmaxf(mv(w.sigma_w, w.sigma_b, in, width, kA, lane), -20.f), 2.f));
        else sigma = expf(w.sigma_param[lane]);
        float act = mu;
        if constexpr (!GREEDY) {
            const float z = gauss_z(seed, collect_id, (uint32_t)e, (uint32_t)t, (uint32_t)lane);
            act = mu + sigma * z;
        }
        float u = act;
        if (cfg.bound_method == 1) u = fminf(fmaxf(act, -1.0f), 1.0f);
        else if (cfg.bound_method == 2) u = tanhf(act);
        float m = u;
        if (cfg.action_scaling) {
            const float lo = w.act_low[lane], hi = w.act_high[lane];
            m = lo + ((hi - lo) * (u + 1.0f)) / 2.0f;   // numpy's order: low + (high - low) * (unit + 1.0) / 2.0
        }
        const size_t row = ((size_t)t * B + e) * kA + lane;
        tr.act[row] = act;
        tr.act_mapped[row] = m;
        xs[lane] = m;
    }
    int p = 0;
    if (lane == 0) p = atomicAdd(&tr.counts[t], 1);
    p = __shfl(p, 0, CIRS_WAVE);
    wbar();
    if (lane < kA) tr.act_buf[(size_t)p * kA + lane] = xs[lane];
    if (lane == 0) tr.lists[(size_t)t * B + p] = e;
}

// ---- position-keyed mode: one wave per env, K/V-cached decode of position t ------------------------------------------------
template <bool DROP, bool GREEDY>
__global__ __launch_bounds__(64 * kWaves) void vtb_policy_step_kernel(cirs_vtb_rollout_cfg cfg, cirs_vtb_policy_weights w, cirs_vtb_traj tr,
                                                                       int t, int steps, uint64_t seed, uint32_t collect_id) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * kWaves + wv;
    const int B = cfg.n_env;
    if (j >= B) return;
    const int e = t == 0 ? j : tr.lists[(size_t)(t - 1) * B + j];
    if (e < 0 || e >= B) return;      // wave-uniform: past the end of the previous step's active list
    const int D = cfg.model.dim_model, L = cfg.model.max_len;
    const WaveLds s = wave_lds(smem, wv, cfg.model.nhead, L);
    bool finished;
    const float x = record_and_slot(cfg, w, tr, s, t, steps, j, e, lane, finished);
    const DropKey dk = drop_key(cfg.model, (uint32_t)(cfg.model.drop_env_base + e), DROP);
    float h = embed_row<DROP>(w, dk, x, t, D, lane);
    for (int l = 0; l < cfg.model.nlayers; ++l) {
        float* kc = tr.kcache + (((size_t)l * B + e) * L) * D;
        float* vc = tr.vcache + (((size_t)l * B + e) * L) * D;
        h = encoder_row<DROP, true>(cfg.model, w.layer[l], s, dk, l, t, h, kc, vc, lane);
    }
    decode_and_act<GREEDY>(cfg, w, tr, s, h, t, e, lane, finished, seed, collect_id);
}

// ---- exact-redraw mode (dropout_redraw): one workgroup per env, the whole prefix 0..t again with the masks of call t ----------
// Call t of env e draws the masks of dropout env id drop_env_base + t * n_env + e at every position 0..t, so nothing of an earlier call
// can be kept: per layer, phase A writes the K/V of every row of the layer's input (rows dealt to the waves), phase B runs the layer's
// rows -- all of them below the top layer, whose outputs are the next layer's input, the last row only in the top layer.  The slots
// x_0..x_t are kept (they carry no mask).  ws: slots [max_len][n_env][D] | layer outputs [nlayers - 1][n_env][max_len][D].
constexpr int kRedrawWaves = 8;
template <bool GREEDY>
__global__ __launch_bounds__(64 * kRedrawWaves) void vtb_policy_step_redraw_kernel(cirs_vtb_rollout_cfg cfg, cirs_vtb_policy_weights w,
                                                                                   cirs_vtb_traj tr, float* ws, int t, int steps, uint64_t seed,
                                                                                   uint32_t collect_id) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x;
    const int B = cfg.n_env;
    const int e = t == 0 ? j : tr.lists[(size_t)(t - 1) * B + j];
    if (e < 0 || e >= B) return;      // workgroup-uniform: past the end of the previous step's active list
    const int D = cfg.model.dim_model, L = cfg.model.max_len, NL = cfg.model.nlayers;
    const WaveLds s = wave_lds(smem, wv, cfg.model.nhead, L);
    float* slot = ws;
    float* rows = ws + (size_t)L * B * D;
    bool finished = false;
    if (wv == 0) {
        const float x = record_and_slot(cfg, w, tr, s, t, steps, j, e, lane, finished);
        if (lane < D) slot[((size_t)t * B + e) * D + lane] = x;
    }
    __syncthreads();
    const DropKey dk = drop_key(cfg.model, (uint32_t)(cfg.model.drop_env_base + t * B + e), true);
    float h_top = 0.f;
    for (int l = 0; l < NL; ++l) {
        const cirs_vtb_policy_layer& ly = w.layer[l];
        float* kc = tr.kcache + (((size_t)l * B + e) * L) * D;
        float* vc = tr.vcache + (((size_t)l * B + e) * L) * D;
        const float* in = l == 0 ? nullptr : rows + (((size_t)(l - 1) * B + e) * L) * D;
        float* out = rows + (((size_t)l * B + e) * L) * D;      // not written by the top layer
        const bool top = l == NL - 1;
        auto row_in = [&](int p) {
            if (l > 0) return lane < D ? in[(size_t)p * D + lane] : 0.f;
            return embed_row<true>(w, dk, lane < D ? slot[((size_t)p * B + e) * D + lane] : 0.f, p, D, lane);
        };
        for (int p = wv; p <= t; p += kRedrawWaves) {      // phase A
            const float h = row_in(p);
            if (lane < D) s.xs[lane] = h;
            wbar();
            if (lane < D) {
                kc[(size_t)p * D + lane] = mv(ly.in_w, ly.in_b, s.xs, D, 3 * D, D + lane);
                vc[(size_t)p * D + lane] = mv(ly.in_w, ly.in_b, s.xs, D, 3 * D, 2 * D + lane);
            }
            wbar();
        }
        __syncthreads();
        if (top) {                                           // phase B
            if (wv == 0) h_top = encoder_row<true, false>(cfg.model, ly, s, dk, l, t, row_in(t), kc, vc, lane);
        } else {
            for (int p = wv; p <= t; p += kRedrawWaves) {
                const float o = encoder_row<true, false>(cfg.model, ly, s, dk, l, p, row_in(p), kc, vc, lane);
                if (lane < D) out[(size_t)p * D + lane] = o;
            }
        }
        __syncthreads();
    }
    if (wv == 0) decode_and_act<GREEDY>(cfg, w, tr, s, h_top, t, e, lane, finished, seed, collect_id);
}

__global__ __launch_bounds__(256) void vtb_gauss_kernel(uint64_t seed, uint32_t collect_id, const int32_t* __restrict__ ids,
                                                        const int32_t* __restrict__ ts, int n, int dims, float* __restrict__ out) {
    const long total = (long)n * dims;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / dims), c = (int)(i % dims);
        out[i] = gauss_z(seed, collect_id, (uint32_t)ids[r], (uint32_t)ts[r], (uint32_t)c);
    }
}

__global__ __launch_bounds__(256) void vtb_mask_kernel(uint64_t dseed, float p, int env0, int n_env, int pos0, int n_pos, int layer, int site,
                                                       int n_elem, float* __restrict__ out) {
    const long total = (long)n_env * n_pos * n_elem;
    const uint32_t thr = dropout_threshold(p);
    const float inv = 1.0f / (1.0f - p);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int el = (int)(i % n_elem);
        const long rest = i / n_elem;
        const int q = (int)(rest % n_pos), ev = (int)(rest / n_pos);
        out[i] = dropout_keep(dseed, (uint32_t)(env0 + ev), (uint32_t)(pos0 + q), (uint32_t)layer, (uint32_t)site, (uint32_t)el, thr) ? inv : 0.f;
    }
}

int grid_of(long total) {
    const int g = cdiv(total, 256);
    return g < 4096 ? g : 4096;
}

int validate_rollout(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* w, const cirs_vtb_cfg* vc, const cirs_vtb_traj* tr) {
    CIRS_REQUIRE(cfg && w && vc && tr, "null rollout argument");
    const cirs_vtb_model_cfg* m = &cfg->model;
    CIRS_REQUIRE(cfg->n_env >= 1, "n_env must be >= 1");
    CIRS_REQUIRE(cfg->n_env == vc->n_env, "rollout n_env must equal the env's n_env");
    CIRS_REQUIRE(cfg->max_turn >= 1, "max_turn must be >= 1");
    CIRS_REQUIRE(!vc->simulated || cfg->max_turn == vc->max_turn, "rollout max_turn must equal the simulated env's max_turn");
    CIRS_REQUIRE(vc->simulated || cfg->max_turn >= vc->max_turn, "rollout max_turn must be >= the raw env's max_turn (it ends every episode there)");
    CIRS_REQUIRE(cfg->force_length >= 0 && cfg->force_length <= cfg->max_turn, "force_length must lie in [0, max_turn]");
    CIRS_REQUIRE(cfg->bound_method >= 0 && cfg->bound_method <= 2, "bound_method must be 0 (none), 1 (clip) or 2 (tanh)");
    if (int rc = vtb_validate_model(m, cfg->max_turn)) return rc;
    CIRS_REQUIRE(m->dim_model <= kMaxD, "dim_model must lie in [1, 64]");      // this and the next three: what a wave holds in LDS
    CIRS_REQUIRE((long)m->nhead * m->max_len <= kMaxAttn, "nhead * max_len must be <= 2048");
    CIRS_REQUIRE(m->d_hid >= 1 && m->d_hid <= kMaxHid, "d_hid must lie in [1, 256]");
    CIRS_REQUIRE(m->dim_state >= 1 && m->dim_state <= kMaxD, "dim_state must lie in [1, 64]");
    CIRS_REQUIRE(w->user_w && w->user_b && w->gate_w && w->gate_b && w->pe && w->dec_w && w->dec_b && w->mu_w && w->mu_b,
                 "tracker / actor weight is null");
    for (int l = 0; l < m->nlayers; ++l) {
        const cirs_vtb_policy_layer& y = w->layer[l];
        CIRS_REQUIRE(y.in_w && y.in_b && y.out_w && y.out_b && y.lin1_w && y.lin1_b && y.lin2_w && y.lin2_b && y.norm1_w && y.norm1_b &&
                         y.norm2_w && y.norm2_b,
                     "encoder layer weight is null");
    }
    for (int i = 0; i < m->n_hidden; ++i) CIRS_REQUIRE(w->trunk_w[i] && w->trunk_b[i], "actor trunk weight is null");
    CIRS_REQUIRE(m->conditioned_sigma ? (w->sigma_w && w->sigma_b) : (w->sigma_param != nullptr), "sigma weight is null");
    CIRS_REQUIRE(!cfg->action_scaling || (w->act_low && w->act_high), "action box is null");
    CIRS_REQUIRE(tr->state && tr->act && tr->act_mapped && tr->obs0 && tr->obs && tr->rew && tr->done && tr->ctr && tr->len && tr->kcache &&
                     tr->vcache && tr->lists && tr->counts && tr->act_buf && tr->step_obs && tr->step_rew && tr->step_ctr && tr->step_done,
                 "trajectory buffer is null");
    return CIRS_OK;
}

}  // namespace
}  // namespace cirs

namespace cirs {
namespace {

// what the exact-redraw mode adds to validate_rollout
int validate_redraw(const cirs_vtb_rollout_cfg* cfg) {
    CIRS_REQUIRE(cfg != nullptr, "null rollout argument");
    const cirs_vtb_model_cfg* m = &cfg->model;
    CIRS_REQUIRE((long)m->drop_env_base + ((long)cfg->max_turn + 1) * cfg->n_env < (1L << 31),
                 "dropout_redraw: drop_env_base + (max_turn + 1) * n_env must be < 2^31 (call c of env e draws dropout env id "
                 "drop_env_base + c * n_env + e)");
    CIRS_REQUIRE((size_t)kRedrawWaves * (kFixed + (size_t)m->nhead * m->max_len) * sizeof(float) <= 65536,
                 "dropout_redraw: nhead * max_len must be <= 1088 (8 waves per env in 64 KB of LDS)");
    return CIRS_OK;
}

// redraw_ws == nullptr: the position-keyed mode
int collect(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* pw, const cirs_vtb_cfg* vtb_cfg, const cirs_vtb_weights* vtb_w,
            cirs_vtb_state* vtb_st, cirs_vtb_traj* traj, float* redraw_ws, uint64_t seed, uint32_t collect_id, void* stream, bool greedy = false) {
    const hipStream_t s = (hipStream_t)stream;
    const cirs_vtb_rollout_cfg c = *cfg;
    const cirs_vtb_traj tr = *traj;
    const int B = c.n_env;
    const int steps = c.force_length > 0 ? c.force_length : (vtb_cfg->simulated ? c.max_turn : vtb_cfg->max_turn);
    const size_t T = (size_t)c.max_turn;
    CIRS_HIP(hipMemsetAsync(tr.lists, 0xFF, (T + 1) * B * sizeof(int32_t), s));
    CIRS_HIP(hipMemsetAsync(tr.counts, 0, (T + 1) * sizeof(int32_t), s));
    CIRS_HIP(hipMemsetAsync(tr.len, 0, (size_t)B * sizeof(int32_t), s));
    CIRS_HIP(hipMemsetAsync(tr.state, 0, (T + 1) * B * c.model.dim_state * sizeof(float), s));
    CIRS_HIP(hipMemsetAsync(tr.act, 0, T * B * kA * sizeof(float), s));
    CIRS_HIP(hipMemsetAsync(tr.act_mapped, 0, T * B * kA * sizeof(float), s));
    CIRS_HIP(hipMemsetAsync(tr.obs, 0, T * B * kObs * sizeof(double), s));
    CIRS_HIP(hipMemsetAsync(tr.rew, 0, T * B * sizeof(double), s));
    CIRS_HIP(hipMemsetAsync(tr.ctr, 0, T * B * sizeof(double), s));
    CIRS_HIP(hipMemsetAsync(tr.done, 0, T * B, s));
    if (int rc = cirs_vtb_reset(vtb_cfg, vtb_w, vtb_st, c.env_seed, nullptr, B, tr.obs0, stream)) return rc;
    const size_t wave_lds_bytes = (kFixed + (size_t)c.model.nhead * c.model.max_len) * sizeof(float);
    const dim3 grid(cdiv(B, kWaves)), block(64 * kWaves);
    const bool drop = c.model.dropout_p > 0.f;
    for (int t = 0; t <= steps; ++t) {
        if (redraw_ws) {
            const auto kern = greedy ? vtb_policy_step_redraw_kernel<true> : vtb_policy_step_redraw_kernel<false>;
            hipLaunchKernelGGL(kern, dim3(B), dim3(64 * kRedrawWaves), kRedrawWaves * wave_lds_bytes, s, c, *pw, tr, redraw_ws, t, steps, seed,
                               collect_id);
            CIRS_CHECK_LAUNCH("vtb_policy_step_redraw_kernel");
        } else {
            const auto kern = drop ? (greedy ? vtb_policy_step_kernel<true, true> : vtb_policy_step_kernel<true, false>)
                                   : (greedy ? vtb_policy_step_kernel<false, true> : vtb_policy_step_kernel<false, false>);
            hipLaunchKernelGGL(kern, grid, block, kWaves * wave_lds_bytes, s, c, *pw, tr, t, steps, seed, collect_id);
            CIRS_CHECK_LAUNCH("vtb_policy_step_kernel");
        }
        if (t == steps) break;
        // the env step of list t (ids past the active count are -1: empty slots)
        if (int rc = cirs_vtb_step(vtb_cfg, vtb_w, vtb_st, c.env_seed, tr.act_buf, tr.lists + (size_t)t * B, B, tr.step_obs, tr.step_rew,
                                   tr.step_done, tr.step_ctr, nullptr, stream))
            return rc;
    }
    return CIRS_OK;
}

}  // namespace
}  // namespace cirs

extern "C" int cirs_vtb_rollout_collect(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* pw, const cirs_vtb_cfg* vtb_cfg,
                                        const cirs_vtb_weights* vtb_w, cirs_vtb_state* vtb_st, cirs_vtb_traj* traj, uint64_t seed,
                                        uint32_t collect_id, void* stream) {
    using namespace cirs;
    if (int rc = validate_rollout(cfg, pw, vtb_cfg, traj)) return rc;
    CIRS_REQUIRE(vtb_w && vtb_st, "null env weights / state");
    return collect(cfg, pw, vtb_cfg, vtb_w, vtb_st, traj, nullptr, seed, collect_id, stream);
}

// replaces the per-call dropout of core/state_tracker.py:170-250 (the tracker stays in train(): build_state runs the whole prefix through
// the encoder again and nn.Dropout draws fresh masks at every call)
extern "C" int cirs_vtb_rollout_collect_redraw(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* pw, const cirs_vtb_cfg* vtb_cfg,
                                               const cirs_vtb_weights* vtb_w, cirs_vtb_state* vtb_st, cirs_vtb_traj* traj, float* redraw_ws,
                                               uint64_t seed, uint32_t collect_id, void* stream) {
    using namespace cirs;
    if (int rc = validate_redraw(cfg)) return rc;
    if (int rc = validate_rollout(cfg, pw, vtb_cfg, traj)) return rc;
    CIRS_REQUIRE(vtb_w && vtb_st, "null env weights / state");
    CIRS_REQUIRE(redraw_ws != nullptr, "dropout_redraw: null workspace (max_len * n_env * dim_model * nlayers floats)");
    // without dropout every call's prefix pass equals the cached decode: run that
    return collect(cfg, pw, vtb_cfg, vtb_w, vtb_st, traj, cfg->model.dropout_p > 0.f ? redraw_ws : nullptr, seed, collect_id, stream);
}

// deterministic_eval in eval mode (reference core/policy/ppo.py:152-153: act = logits[0], the mean): either collect without the Gaussian draw
extern "C" int cirs_vtb_rollout_collect_greedy(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* pw, const cirs_vtb_cfg* vtb_cfg,
                                               const cirs_vtb_weights* vtb_w, cirs_vtb_state* vtb_st, cirs_vtb_traj* traj, float* redraw_ws,
                                               void* stream) {
    using namespace cirs;
    if (redraw_ws) { if (int rc = validate_redraw(cfg)) return rc; }
    if (int rc = validate_rollout(cfg, pw, vtb_cfg, traj)) return rc;
    CIRS_REQUIRE(vtb_w && vtb_st, "null env weights / state");
    return collect(cfg, pw, vtb_cfg, vtb_w, vtb_st, traj, (redraw_ws && cfg->model.dropout_p > 0.f) ? redraw_ws : nullptr, 0, 0, stream, true);
}

extern "C" int cirs_vtb_rollout_noise(uint64_t seed, uint32_t collect_id, const int32_t* env_ids, const int32_t* ts, int32_t n, int32_t dims,
                                      float* out, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(n >= 0 && dims >= 0, "n and dims must be >= 0");
    if (n == 0 || dims == 0) return CIRS_OK;
    CIRS_REQUIRE(env_ids && ts && out, "null argument");
    hipLaunchKernelGGL(vtb_gauss_kernel, dim3(grid_of((long)n * dims)), dim3(256), 0, (hipStream_t)stream, seed, collect_id, env_ids, ts, n, dims,
                       out);
    CIRS_CHECK_LAUNCH("vtb_gauss_kernel");
    return CIRS_OK;
}

extern "C" int cirs_vtb_rollout_masks(uint64_t dropout_seed, float p, int32_t env0, int32_t n_env, int32_t pos0, int32_t n_pos, int32_t layer,
                                      int32_t site, int32_t n_elem, float* out, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(p >= 0.f && p < 1.f, "p must lie in [0, 1)");
    CIRS_REQUIRE(n_env >= 0 && n_pos >= 0 && n_elem >= 0, "sizes must be >= 0");
    CIRS_REQUIRE(env0 >= 0 && pos0 >= 0 && pos0 + (long)n_pos <= 4096, "env0 / positions out of range (positions < 4096)");
    CIRS_REQUIRE(layer >= 0 && layer < CIRS_VTB_RO_MAX_LAYERS, "layer out of range");
    CIRS_REQUIRE(site >= CIRS_DROP_POS && site <= CIRS_DROP_RES2, "site out of range");
    const long total = (long)n_env * n_pos * n_elem;
    if (total == 0) return CIRS_OK;
    CIRS_REQUIRE(out != nullptr, "null output");
    hipLaunchKernelGGL(vtb_mask_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, dropout_seed, p, env0, n_env, pos0, n_pos, layer,
                       site, n_elem, out);
    CIRS_CHECK_LAUNCH("vtb_mask_kernel");
    return CIRS_OK;
}
