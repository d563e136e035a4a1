// virtualtb.hip -- batched VirtualTaobao env step for gfx950: VirtualTB-v0 (raw kind, reward = clicks) and
// SimulatedEnv(VirtualTB-v0) (simulated kind, UserModel_MMOE reward discounted by the exposure effect).
//
// Reference order of effects per env (environments/VirtualTaobao/virtualTB/envs/virtualTB.py, the VirtualTB branch of
// core/env/simulatedEnv/simulated_env.py), all inside ONE launch per vector step:
//   exit rule   done iff one of the last min(t, N-1) actions lies within leave_threshold (L2, fp64) or t >= max_turn - 1
//   exposure    gamma * sum_{j<t} exp(-(t-j) d_j / tau) over the stored actions (fp64; simulated kind only)
//   action      [task user 88 | t | action 27] -> 128 -> 256 -> 21 (LeakyReLU 0.01); clicks a = Gumbel-max over logits
//               0..10, b = Gumbel-max over logits 11..20
//   reward      simulated: MMoE([sim user 88 | prev reward, 0, t | action 27]) clamped to [0, 10], then v1 r/(1+e) or
//               v2 r - e; raw: a
//   redraw      a done env draws its next task user in the same launch: generator 128 -> 128 -> 88 on z ~ U(0,1)^128,
//               one Gumbel-max per group.  The turn counter, the history and the simulated kind's sim user are kept, as
//               in the reference; only reset() clears them.
// The reference's LEAVE MODEL is not evaluated: its draw is recorded there (_leave_page) but affects no observable output.
//
// Layout: a tile of 16 envs per 256-thread workgroup.  The dense layers read their weights ([in][out], coalesced over the
// output column, ~0.5 MB in all and L2-resident) once per tile and keep the 16 activation rows in LDS; each thread owns
// (output column, 4 envs) units, so one weight load feeds 4 FMAs and the activation reads are LDS broadcasts.  The layers
// are fp32 VALU FMAs, not MFMA: at ~180 kFLOP per env a 1024-env step is 0.18 GFLOP, and the step is bound by the
// dependent layer chain (five to ten layers, each a barrier), not by the FMA rate.  The fp64 scalar parts (exit rule,
// exposure, CTR) run one wavefront per env, lanes over the history rows.
//
// Noise (INTEGRATION.md "Sampler noise"): Philox4x32-10, key = seed, counter = (env id, event, block, tag); tag 0 = the 21
// Gumbels of a step, tag 1 = a user draw (128 uniforms, then 88 Gumbels).  cirs_vtb_noise writes exactly those values.
#include "vtb_tile.h"

namespace cirs {
namespace {

constexpr int kMmIn = kUser + 3 + kAct, kMmH = 128, kExperts = 4, kExpertDim = 8;

// noise column c of (env, ev) as cirs_vtb_noise lays it out: 0..20 step Gumbels, 21..148 z, 149..236 user Gumbels
__device__ __forceinline__ float noise_value(uint64_t seed, uint32_t env, uint32_t ev, int c) {
    if (c < kStepWords) return gumbel_from_bits(noise_word(seed, env, ev, 0, c));
    const int w = c - kStepWords;
    const uint32_t x = noise_word(seed, env, ev, 1, w);
    return w < kZ ? u01_from_bits(x) : gumbel_from_bits(x);
}

// shared memory of one tile
struct Tile {
    static constexpr int kRows = kTile;
    float xa[kTile * kLd];
    float xb[kTile * kLd];
    float act[kTile][kAct];
    float gum[kTile][kUser];      // user-draw Gumbels
    float sg[kTile][kStepWords];  // step Gumbels
    double lin[kTile];
    float y[kTile];
    double expo[kTile];
    int env[kTile];               // -1: empty slot
    int turn[kTile];
    uint32_t ev[kTile];
    int need[kTile];              // user draw wanted for this slot
    int user[kTile][kGroups];     // one-hot positions
    int ab[kTile][2];
    int any;
};

// UserModel_MMOE.forward on the tile's inputs in T.xa[s][0..118) -> T.y[s] (unclamped).  Clobbers xa / xb.
__device__ void mmoe_tile(Tile& T, const cirs_vtb_weights& w) {
    if (threadIdx.x < kTile) {   // linear_model_task(X) before the input is overwritten
        const int s = threadIdx.x;
        double acc = 0.0;
        for (int k = 0; k < kMmIn; ++k) acc = fma((double)T.xa[s * kLd + k], (double)w.mm_wlin[k], acc);
        T.lin[s] = acc;
    }
    dense_tile<kActRelu, double>(w.mm_w1, w.mm_b1, T.xa, kMmIn, kMmH, T.xb);
    dense_tile<kActRelu, double>(w.mm_w2, w.mm_b2, T.xb, kMmH, kMmH, T.xa);
    dense_tile<kActNone, double>(w.mm_we, w.mm_be, T.xa, kMmH, kExperts * kExpertDim, T.xb);
    dense_tile<kActNone, double>(w.mm_wg, nullptr, T.xa, kMmH, kExperts, T.xb + kExperts * kExpertDim);
    if (threadIdx.x < kTile) {
        const int s = threadIdx.x;
        const float* ex = T.xb + s * kLd;
        const float* gl = ex + kExperts * kExpertDim;
        float m = gl[0];
        for (int e = 1; e < kExperts; ++e) m = fmaxf(m, gl[e]);
        double p[kExperts], sum = 0.0;
        for (int e = 0; e < kExperts; ++e) { p[e] = exp((double)(gl[e] - m)); sum += p[e]; }
        double tower = 0.0;
        for (int d = 0; d < kExpertDim; ++d) {
            double md = 0.0;
            for (int e = 0; e < kExperts; ++e) md = fma((double)ex[d * kExperts + e], p[e] / sum, md);
            tower = fma(md, (double)w.mm_wt[d], tower);
        }
        T.y[s] = (float)((T.lin[s] + tower) + (double)w.mm_bias[0]);
    }
    __syncthreads();
}

// slot bookkeeping shared by both kernels: env id, turn, event of slot s = threadIdx.x
__device__ __forceinline__ void load_slots(Tile& T, const cirs_vtb_cfg& cfg, const cirs_vtb_state& st, const int32_t* ids, int n) {
    if (threadIdx.x < kTile) {
        const int s = threadIdx.x, j = blockIdx.x * kTile + s;
        int e = -1;
        if (j < n) e = ids ? ids[j] : j;
        if (e < 0 || e >= cfg.n_env) e = -1;     // the host validates ids; never touch memory outside the state
        T.env[s] = e;
        T.turn[s] = e >= 0 ? st.turn[e] : 0;
        T.ev[s] = e >= 0 ? st.event[e] : 0u;
        T.need[s] = 0;
    }
    if (threadIdx.x == 0) T.any = 0;
    __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(kThreads) void vtb_reset_kernel(cirs_vtb_cfg cfg, cirs_vtb_weights w, cirs_vtb_state st, uint64_t seed,
                                                             const int32_t* __restrict__ ids, int n, double* __restrict__ obs) {
    __shared__ Tile T;
    load_slots(T, cfg, st, ids, n);
    if (threadIdx.x < kTile) T.need[threadIdx.x] = T.env[threadIdx.x] >= 0;
    __syncthreads();
    draw_users(T, w, seed, st.task_user, st.sim_user);
    if (threadIdx.x < kTile) {
        const int e = T.env[threadIdx.x];
        if (e >= 0) {
            st.turn[e] = 0;
            st.event[e] = T.ev[threadIdx.x] + 1u;
            st.prev_reward[e] = 0.0;
            st.cum_reward[e] = 0.0;
            st.lst_action[2 * e] = 0;
            st.lst_action[2 * e + 1] = 0;
        }
    }
    const long hrow = (long)cfg.max_turn * kAct;
    for (int s = 0; s < kTile; ++s) {
        const int e = T.env[s];
        if (e < 0) continue;
        for (long i = threadIdx.x; i < hrow; i += kThreads) st.hist[(long)e * hrow + i] = 0.f;
    }
    if (obs) {
        for (int i = threadIdx.x; i < kTile * (kUser + 3); i += kThreads) {
            const int s = i / (kUser + 3), c = i % (kUser + 3);
            const int j = blockIdx.x * kTile + s;
            if (T.env[s] < 0) continue;
            obs[(long)j * (kUser + 3) + c] = c < kUser && T.user[s][group_of(c)] == c ? 1.0 : 0.0;
        }
    }
}

__global__ __launch_bounds__(kThreads) void vtb_step_kernel(cirs_vtb_cfg cfg, cirs_vtb_weights w, cirs_vtb_state st, uint64_t seed,
                                                            const float* __restrict__ actions, const int32_t* __restrict__ ids, int n,
                                                            double* __restrict__ obs, double* __restrict__ rew,
                                                            uint8_t* __restrict__ done_out, double* __restrict__ ctr,
                                                            double* __restrict__ expo_out) {
    __shared__ Tile T;
    const int j0 = blockIdx.x * kTile;
    load_slots(T, cfg, st, ids, n);
    for (int i = threadIdx.x; i < kTile * kAct; i += kThreads) {
        const int s = i / kAct, c = i % kAct;
        T.act[s][c] = T.env[s] >= 0 ? actions[(long)(j0 + s) * kAct + c] : 0.f;
    }
    for (int i = threadIdx.x; i < kTile * kGroups; i += kThreads) {
        const int s = i / kGroups, g = i % kGroups;
        T.user[s][g] = T.env[s] >= 0 ? st.task_user[(long)T.env[s] * kGroups + g] : -1;
    }
    for (int i = threadIdx.x; i < kTile * 6; i += kThreads) {   // the 21 step Gumbels: 6 Philox blocks, tag 0
        const int s = i / 6, blk = i % 6;
        const u32x4 r = T.env[s] >= 0 ? philox4x32_10((uint32_t)T.env[s], T.ev[s], blk, 0u, (uint32_t)seed, (uint32_t)(seed >> 32))
                                      : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * blk + q < kStepWords) T.sg[s][4 * blk + q] = gumbel_from_bits(block_word(r, q));
    }
    __syncthreads();

    // ---- exit rule + exposure: one wavefront per env, lanes over the stored actions (fp64) ------------------------------
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < kTile; s += kThreads / 64) {
        const int e = T.env[s];
        if (e < 0) continue;   // wave-uniform
        const int t = T.turn[s];
        const int rows = t < cfg.max_turn ? t : cfg.max_turn;
        const bool want_expo = cfg.simulated && cfg.use_exposure && cfg.tau > 0.0;
        const float* h = st.hist + (long)e * cfg.max_turn * kAct;
        bool leave = false;
        double ex = 0.0;
        for (int r = lane; r < rows; r += 64) {
            double ss = 0.0;
            for (int c = 0; c < kAct; ++c) {
                const double d = (double)T.act[s][c] - (double)h[(long)r * kAct + c];
                ss = fma(d, d, ss);
            }
            const double dist = sqrt(ss);
            if (r >= t - cfg.num_leave_compute + 1 && dist <= cfg.leave_threshold) leave = true;
            if (want_expo) ex += exp((double)(-(t - r)) * dist / cfg.tau);
        }
        leave = __any(leave);
        ex = wave_sum_f64(ex);
        if (lane == 0) {
            const bool done = leave || t >= cfg.max_turn - 1;
            T.need[s] = done;
            if (done) T.any = 1;
            T.expo[s] = want_expo && t > 0 ? ex * cfg.gamma_exposure : 0.0;
        }
        if (t < cfg.max_turn && lane < kAct) st.hist[((long)e * cfg.max_turn + t) * kAct + lane] = T.act[s][lane];
    }

    // ---- action model on [task user | t | action] ------------------------------------------------------------------------
    for (int i = threadIdx.x; i < kTile * kActIn; i += kThreads) {
        const int s = i / kActIn, c = i % kActIn;
        float v;
        if (c < kUser) v = T.user[s][group_of(c)] == c ? 1.f : 0.f;
        else if (c == kUser) v = (float)T.turn[s];
        else v = T.act[s][c - kUser - 1];
        T.xa[s * kLd + c] = v;
    }
    __syncthreads();
    action_draw(T, w);

    // ---- user model (simulated kind) ---------------------------------------------------------------------------------------
    if (cfg.simulated) {
        for (int i = threadIdx.x; i < kTile * kMmIn; i += kThreads) {
            const int s = i / kMmIn, c = i % kMmIn, e = T.env[s];
            float v = 0.f;
            if (e >= 0) {
                if (c < kUser) v = st.sim_user[(long)e * kGroups + group_of(c)] == c ? 1.f : 0.f;
                else if (c == kUser) v = (float)st.prev_reward[e];
                else if (c == kUser + 2) v = (float)T.turn[s];
                else if (c > kUser + 2) v = T.act[s][c - kUser - 3];
            }
            T.xa[s * kLd + c] = v;
        }
        __syncthreads();
        mmoe_tile(T, w);
    }

    // ---- outputs and state -----------------------------------------------------------------------------------------------
    if (threadIdx.x < kTile) {
        const int s = threadIdx.x, e = T.env[s], j = j0 + s;
        if (e >= 0) {
            const int t = T.turn[s];
            const bool done = T.need[s] != 0;
            double r;
            if (cfg.simulated) {
                const double p = (double)fminf(fmaxf(T.y[s], 0.f), 10.f);
                r = cfg.version == 1 ? p / (1.0 + T.expo[s]) : p - T.expo[s];
                st.prev_reward[e] = r;
            } else {
                r = (double)T.ab[s][0];
            }
            const double cum = st.cum_reward[e] + r;
            st.cum_reward[e] = cum;
            st.turn[e] = t + 1;
            st.event[e] = T.ev[s] + 1u;
            st.lst_action[2 * e] = done ? 0 : T.ab[s][0];
            st.lst_action[2 * e + 1] = done ? 0 : T.ab[s][1];
            rew[j] = r;
            done_out[j] = done;
            ctr[j] = cum / (double)(t + 1) / 10.0;
            if (expo_out) expo_out[j] = T.expo[s];
            double* o = obs + (long)j * (kAct + 3);
            if (cfg.simulated) {
                o[kAct] = r;
                o[kAct + 1] = 0.0;
            } else {
                o[kAct] = done ? 0.0 : (double)T.ab[s][0];
                o[kAct + 1] = done ? 0.0 : (double)T.ab[s][1];
            }
            o[kAct + 2] = (double)(t + 1);
        }
    }
    for (int i = threadIdx.x; i < kTile * kAct; i += kThreads) {
        const int s = i / kAct, c = i % kAct;
        if (T.env[s] >= 0) obs[(long)(j0 + s) * (kAct + 3) + c] = (double)T.act[s][c];
    }

    // ---- next task user for the envs that finished (same event, tag 1) ------------------------------------------------------
    __syncthreads();
    if (T.any) draw_users(T, w, seed, st.task_user, nullptr);   // block-uniform
}

__global__ __launch_bounds__(kThreads) void vtb_mmoe_kernel(cirs_vtb_weights w, const float* __restrict__ x, int n, float* __restrict__ y) {
    __shared__ Tile T;
    const int j0 = blockIdx.x * kTile;
    for (int i = threadIdx.x; i < kTile * kMmIn; i += kThreads) {
        const int s = i / kMmIn, c = i % kMmIn;
        T.xa[s * kLd + c] = j0 + s < n ? x[(long)(j0 + s) * kMmIn + c] : 0.f;
    }
    __syncthreads();
    mmoe_tile(T, w);
    if (threadIdx.x < kTile && j0 + (int)threadIdx.x < n) y[j0 + threadIdx.x] = T.y[threadIdx.x];
}

__global__ __launch_bounds__(256) void vtb_noise_kernel(uint64_t seed, const int32_t* __restrict__ ids, const uint32_t* __restrict__ events,
                                                        int n, float* __restrict__ out) {
    const long total = (long)n * CIRS_VTB_NOISE_COLS;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / CIRS_VTB_NOISE_COLS), c = (int)(i % CIRS_VTB_NOISE_COLS);
        out[i] = noise_value(seed, (uint32_t)ids[j], events[j], c);
    }
}

static int validate(const cirs_vtb_cfg* cfg, const cirs_vtb_weights* w, bool need_env) {
    CIRS_REQUIRE(cfg != nullptr, "vtb cfg is null");
    CIRS_REQUIRE(w != nullptr, "vtb weights is null");
    if (need_env) {
        CIRS_REQUIRE(cfg->n_env > 0, "n_env must be positive");
        CIRS_REQUIRE(cfg->max_turn > 0 && cfg->max_turn <= 16383, "max_turn out of range (1..16383)");
        CIRS_REQUIRE(cfg->num_leave_compute >= 0, "num_leave_compute must be >= 0");
        CIRS_REQUIRE(cfg->simulated == 0 || cfg->simulated == 1, "simulated must be 0 or 1");
        CIRS_REQUIRE(w->gen_w1 && w->gen_b1 && w->gen_w2 && w->gen_b2, "generator weight is null");
        CIRS_REQUIRE(w->act_w1 && w->act_b1 && w->act_w2 && w->act_b2 && w->act_w3 && w->act_b3, "action-model weight is null");
    }
    if (!need_env || cfg->simulated) {
        if (need_env) {
            CIRS_REQUIRE(cfg->version == 1 || cfg->version == 2, "version must be 1 (v1) or 2 (v2)");
            CIRS_REQUIRE(cfg->use_exposure == 0 || cfg->use_exposure == 1, "use_exposure must be 0 or 1");
        }
        CIRS_REQUIRE(cfg->mmoe_d_in == kMmIn && cfg->mmoe_dnn_layers == 2 && cfg->mmoe_h1 == kMmH && cfg->mmoe_h2 == kMmH &&
                         cfg->mmoe_experts == kExperts && cfg->mmoe_expert_dim == kExpertDim && cfg->mmoe_tasks == 1 &&
                         cfg->mmoe_task_dim == 1,
                     "unsupported MMoE shape: only d_in 118, dnn (128, 128), 4 experts x 8, one task of dim 1");
        CIRS_REQUIRE(w->mm_w1 && w->mm_b1 && w->mm_w2 && w->mm_b2 && w->mm_we && w->mm_be && w->mm_wg && w->mm_wt && w->mm_wlin &&
                         w->mm_bias,
                     "MMoE weight is null");
    }
    return CIRS_OK;
}

static int validate_state(const cirs_vtb_state* st) {
    CIRS_REQUIRE(st && st->task_user && st->sim_user && st->turn && st->event && st->prev_reward && st->cum_reward &&
                     st->lst_action && st->hist,
                 "vtb state has a null field");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_vtb_reset(const cirs_vtb_cfg* cfg, const cirs_vtb_weights* w, cirs_vtb_state* st, uint64_t seed,
                              const int32_t* env_ids, int32_t n, double* obs_out, void* stream) {
    using namespace cirs;
    if (int rc = validate(cfg, w, true)) return rc;
    CIRS_REQUIRE(n >= 0 && n <= cfg->n_env, "n out of range (0..n_env)");
    if (n == 0) return CIRS_OK;
    if (int rc = validate_state(st)) return rc;
    hipLaunchKernelGGL(vtb_reset_kernel, dim3(cdiv(n, kTile)), dim3(kThreads), 0, (hipStream_t)stream, *cfg, *w, *st, seed, env_ids,
                       n, obs_out);
    CIRS_CHECK_LAUNCH("vtb_reset_kernel");
    return CIRS_OK;
}

extern "C" int cirs_vtb_step(const cirs_vtb_cfg* cfg, const cirs_vtb_weights* w, cirs_vtb_state* st, uint64_t seed,
                             const float* actions, const int32_t* env_ids, int32_t n, double* obs_out, double* rew_out,
                             uint8_t* done_out, double* ctr_out, double* expo_out, void* stream) {
    using namespace cirs;
    if (int rc = validate(cfg, w, true)) return rc;
    CIRS_REQUIRE(n >= 0 && n <= cfg->n_env, "n out of range (0..n_env)");
    if (n == 0) return CIRS_OK;
    if (int rc = validate_state(st)) return rc;
    CIRS_REQUIRE(actions && obs_out && rew_out && done_out && ctr_out, "null action/output pointer");
    hipLaunchKernelGGL(vtb_step_kernel, dim3(cdiv(n, kTile)), dim3(kThreads), 0, (hipStream_t)stream, *cfg, *w, *st, seed, actions,
                       env_ids, n, obs_out, rew_out, done_out, ctr_out, expo_out);
    CIRS_CHECK_LAUNCH("vtb_step_kernel");
    return CIRS_OK;
}

extern "C" int cirs_vtb_noise(uint64_t seed, const int32_t* env_ids, const uint32_t* events, int32_t n, float* out, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(n >= 0, "n must be >= 0");
    if (n == 0) return CIRS_OK;
    CIRS_REQUIRE(env_ids && events && out, "null argument");
    const long total = (long)n * CIRS_VTB_NOISE_COLS;
    const int grid = cdiv(total, 256) < 4096 ? cdiv(total, 256) : 4096;
    hipLaunchKernelGGL(vtb_noise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, seed, env_ids, events, n, out);
    CIRS_CHECK_LAUNCH("vtb_noise_kernel");
    return CIRS_OK;
}

extern "C" int cirs_vtb_mmoe_forward(const cirs_vtb_cfg* cfg, const cirs_vtb_weights* w, const float* x, int32_t n, float* y_out,
                                     void* stream) {
    using namespace cirs;
    if (int rc = validate(cfg, w, false)) return rc;
    CIRS_REQUIRE(n >= 0, "n must be >= 0");
    if (n == 0) return CIRS_OK;
    CIRS_REQUIRE(x && y_out, "null argument");
    hipLaunchKernelGGL(vtb_mmoe_kernel, dim3(cdiv(n, kTile)), dim3(kThreads), 0, (hipStream_t)stream, *w, x, n, y_out);
    CIRS_CHECK_LAUNCH("vtb_mmoe_kernel");
    return CIRS_OK;
}
