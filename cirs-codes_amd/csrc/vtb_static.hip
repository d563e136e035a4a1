// vtb_static.hip -- evaluation of the VirtualTaobao static baselines for gfx950: evaluation.py:238-282 (test_taobao) with the
// trajectories in lock step and the whole evaluation in ONE launch.
//
// The reference plays num_trajectory trajectories one env step at a time: a batch-1 forward of the two-task UserModel_MMOE on the
// static state [user 88 | last clicks, last second draw | turn], epsilon-greedy on the 27 predicted item features, VirtualTB.step.
// The work is a latency chain (about 12 small dense layers per turn, at most max_turn turns) and the trajectories never meet, so a
// workgroup takes 4 trajectories (100 trajectories -> 25 workgroups on 25 CUs) and runs their turns in a loop of its own; a finished
// trajectory idles until its three neighbours are done.  No grid-wide synchronisation, no host round trip, no float atomics.
// Per turn:
//   state    user one-hot, last (clicks, second draw), turn                                         -> out.state
//   policy   mmoe_forward_tile (vtb_mmoe.h): fp64 sums, one fp32 rounding per layer                 -> 27 features + reward_pred
//   epsilon  u < epsilon (only when epsilon > 0): the action is 27 uniforms of [0, 1) instead       -> out.action, out.explore
//   exit     done iff one of the last min(t, N-1) actions lies within leave_threshold (L2, fp64) or t >= max_turn - 1
//   action   the env's action model and Gumbel-max draws (vtb_tile.h, the code of vtb_step_kernel)  -> reward = clicks
// then vtb_static_reduce_kernel (one workgroup) adds the per-trajectory integers and fp64 sums in trajectory order.
// The action is not clipped to the env's action box and the user VirtualTB.step redraws on done is skipped (test_taobao resets).
#include "vtb_mmoe.h"

namespace cirs {
namespace {

constexpr int kSRows = 4;                      // trajectories per workgroup
constexpr int kStLd = CIRS_VTB_STATIC_STATE_DIM + 1;
constexpr int kEpsWords = 1 + kAct;            // 28 words = 7 Philox blocks
static_assert(kSRows * 64 == kThreads, "the exit rule runs one wavefront per trajectory");

struct STile {
    static constexpr int kRows = kSRows;
    float xa[kSRows * kLd];
    float xb[kSRows * kLd];
    float st[kSRows][kStLd];        // the static state of the turn
    float out[kSRows][kMmOut];      // policy output: 27 item features | reward_pred
    float act[kSRows][kAct];
    float gum[kSRows][kUser];
    float sg[kSRows][kStepWords];
    float eu[kSRows][kEpsWords];    // epsilon uniform | 27 exploration uniforms
    MmoeScratch<kSRows> mm;
    double closs[kSRows];
    int env[kSRows];                // trajectory id, -1: empty slot
    uint32_t ev[kSRows];
    int need[kSRows];
    int user[kSRows][kGroups];
    int ab[kSRows][2];
    int lst[kSRows][2];
    int fin[kSRows];                // the trajectory has ended (or the slot is empty)
    int dn[kSRows];                 // this turn's done
    int expl[kSRows];
    int clicks[kSRows];
    int len[kSRows];
    int n_live;
};

}  // namespace

__global__ __launch_bounds__(kThreads) void vtb_static_eval_kernel(cirs_vtb_static_cfg cfg, cirs_vtb_weights ew, cirs_vtb_mmoe_weights pw,
                                                                   uint64_t seed, cirs_vtb_static_out out, double* __restrict__ ws_closs,
                                                                   int32_t* __restrict__ ws_clicks) {
    __shared__ STile T;
    const int tid = threadIdx.x, j0 = blockIdx.x * kSRows;
    const int MT = cfg.max_turn;
    if (tid < kSRows) {
        const int j = j0 + tid;
        const bool ok = j < cfg.n_traj;
        T.env[tid] = ok ? j : -1;
        T.ev[tid] = 0u;
        T.need[tid] = ok;
        T.fin[tid] = !ok;
        T.lst[tid][0] = T.lst[tid][1] = 0;
        T.clicks[tid] = 0;
        T.len[tid] = 0;
        T.closs[tid] = 0.0;
    }
    for (int i = tid; i < kSRows * kGroups; i += kThreads) T.user[i / kGroups][i % kGroups] = -1;
    __syncthreads();
    draw_users(T, ew, seed, out.user, nullptr);

    for (int t = 0; t < MT; ++t) {
        if (tid == 0) {
            int n = 0;
            for (int s = 0; s < kSRows; ++s) n += !T.fin[s];
            T.n_live = n;
        }
        __syncthreads();
        if (T.n_live == 0) break;   // block-uniform

        // ---- static state, step Gumbels (tag 0) and the epsilon draw (tag 2) of event 1 + t ------------------------------
        for (int i = tid; i < kSRows * CIRS_VTB_STATIC_STATE_DIM; i += kThreads) {
            const int s = i / CIRS_VTB_STATIC_STATE_DIM, c = i % CIRS_VTB_STATIC_STATE_DIM;
            float v;
            if (c < kUser) v = T.user[s][group_of(c)] == c ? 1.f : 0.f;
            else if (c < kUser + 2) v = (float)T.lst[s][c - kUser];
            else v = (float)t;
            T.st[s][c] = v;
            if (!T.fin[s]) out.state[((long)T.env[s] * MT + t) * CIRS_VTB_STATIC_STATE_DIM + c] = v;
        }
        for (int i = tid; i < kSRows * 13; i += kThreads) {   // 6 blocks of tag 0, 7 blocks of tag 2
            const int s = i / 13, b = i % 13;
            const bool step = b < 6;
            const uint32_t blk = step ? b : b - 6;
            const u32x4 r = T.env[s] >= 0 ? philox4x32_10((uint32_t)T.env[s], 1u + (uint32_t)t, blk, step ? kTagStep : kTagEps,
                                                          (uint32_t)seed, (uint32_t)(seed >> 32))
                                          : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int wd = 4 * blk + q;
                if (step) { if (wd < kStepWords) T.sg[s][wd] = gumbel_from_bits(block_word(r, q)); }
                else T.eu[s][wd] = u01_from_bits(block_word(r, q));
            }
        }
        __syncthreads();

        // ---- the policy: both tasks of the MMoE ----------------------------------------------------------------------------
        mmoe_forward_tile<kSRows>(cfg.policy, pw, &T.st[0][0], kStLd, T.xa, T.xb, T.mm, &T.out[0][0], kMmOut);

        // ---- epsilon-greedy (evaluation.py:253-255) --------------------------------------------------------------------------
        for (int i = tid; i < kSRows * kAct; i += kThreads) {
            const int s = i / kAct, c = i % kAct;
            const bool ex = cfg.epsilon > 0.0 && (double)T.eu[s][0] < cfg.epsilon;
            T.act[s][c] = ex ? T.eu[s][1 + c] : T.out[s][c];
            if (c == 0) T.expl[s] = ex;
        }
        __syncthreads();

        // ---- exit rule: one wavefront per trajectory, lanes over the window's stored actions (fp64) --------------------------
        {
            const int s = tid >> 6, lane = tid & 63;
            if (!T.fin[s]) {   // wave-uniform
                const float* h = out.action + (long)T.env[s] * MT * kAct;
                bool leave = false;
                const int r0 = t - cfg.num_leave_compute + 1 > 0 ? t - cfg.num_leave_compute + 1 : 0;
                for (int r = r0 + lane; r < t; r += 64) {
                    double ss = 0.0;
                    for (int c = 0; c < kAct; ++c) {
                        const double d = (double)T.act[s][c] - (double)h[(long)r * kAct + c];
                        ss = fma(d, d, ss);
                    }
                    if (sqrt(ss) <= cfg.leave_threshold) leave = true;
                }
                leave = __any(leave);
                if (lane == 0) T.dn[s] = leave || t >= MT - 1;
                if (lane < kAct) out.action[((long)T.env[s] * MT + t) * kAct + lane] = T.act[s][lane];
            }
        }

        // ---- the env's action model on [user | t | action] and its two draws -------------------------------------------------
        for (int i = tid; i < kSRows * kActIn; i += kThreads) {
            const int s = i / kActIn, c = i % kActIn;
            float v;
            if (c < kUser) v = T.user[s][group_of(c)] == c ? 1.f : 0.f;
            else if (c == kUser) v = (float)t;
            else v = T.act[s][c - kUser - 1];
            T.xa[s * kLd + c] = v;
        }
        __syncthreads();
        action_draw(T, ew);

        // ---- bookkeeping ---------------------------------------------------------------------------------------------------
        if (tid < kSRows && !T.fin[tid]) {
            const int s = tid, a = T.ab[s][0];
            const long row = (long)T.env[s] * MT + t;
            const float pred = T.out[s][kAct];
            const bool done = T.dn[s] != 0;
            out.reward[row] = a;
            out.reward_pred[row] = pred;
            out.done[row] = done;
            out.explore[row] = T.expl[s] != 0;
            T.clicks[s] += a;
            T.closs[s] += fabs((double)pred - (double)a);
            T.lst[s][0] = done ? 0 : a;
            T.lst[s][1] = done ? 0 : T.ab[s][1];
            if (done) { T.fin[s] = 1; T.len[s] = t + 1; }
        }
        __syncthreads();
    }
    if (tid < kSRows && T.env[tid] >= 0) {
        int32_t* lens = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(out.metrics) + 48);
        lens[T.env[tid]] = T.len[tid];
        ws_clicks[T.env[tid]] = T.clicks[tid];
        ws_closs[T.env[tid]] = T.closs[tid];
    }
}

// {ctr, click_loss, len_tra, R_tra} from the per-trajectory results, added in trajectory order by one thread (chunks of 256
// staged through LDS so that the loads are not a dependent chain)
__global__ __launch_bounds__(256) void vtb_static_reduce_kernel(int n, const double* __restrict__ ws_closs, const int32_t* __restrict__ ws_clicks,
                                                                void* metrics) {
    __shared__ double s_closs[256];
    __shared__ int s_clicks[256], s_len[256];
    const int32_t* lens = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(metrics) + 48);
    long long clicks = 0, turns = 0;
    double closs = 0.0;
    for (int base = 0; base < n; base += 256) {
        const int j = base + threadIdx.x;
        if (j < n) { s_closs[threadIdx.x] = ws_closs[j]; s_clicks[threadIdx.x] = ws_clicks[j]; s_len[threadIdx.x] = lens[j]; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = n - base < 256 ? n - base : 256;
            for (int i = 0; i < m; ++i) { clicks += s_clicks[i]; turns += s_len[i]; closs += s_closs[i]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* m = reinterpret_cast<double*>(metrics);
        m[0] = (double)clicks / (double)turns;
        m[1] = closs / (double)turns;
        m[2] = (double)turns / (double)n;
        m[3] = (double)clicks / (double)n;
        long long* q = reinterpret_cast<long long*>(m + 4);
        q[0] = clicks;
        q[1] = turns;
    }
}

__global__ __launch_bounds__(256) void vtb_static_noise_kernel(uint64_t seed, const int32_t* __restrict__ ids, const int32_t* __restrict__ turns,
                                                               int n, float* __restrict__ out) {
    const long total = (long)n * CIRS_VTB_STATIC_NOISE_COLS;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / CIRS_VTB_STATIC_NOISE_COLS), c = (int)(i % CIRS_VTB_STATIC_NOISE_COLS);
        const uint32_t id = (uint32_t)ids[j], ev = 1u + (uint32_t)turns[j];
        float v;
        if (c < kStepWords) v = gumbel_from_bits(noise_word(seed, id, ev, kTagStep, c));
        else if (c < kStepWords + kZ) v = u01_from_bits(noise_word(seed, id, 0u, kTagUser, c - kStepWords));
        else if (c < CIRS_VTB_NOISE_COLS) v = gumbel_from_bits(noise_word(seed, id, 0u, kTagUser, c - kStepWords));
        else v = u01_from_bits(noise_word(seed, id, ev, kTagEps, c - CIRS_VTB_NOISE_COLS));
        out[i] = v;
    }
}

static int validate_static(const cirs_vtb_static_cfg* cfg) {
    CIRS_REQUIRE(cfg != nullptr, "vtb static cfg is null");
    CIRS_REQUIRE(cfg->n_traj > 0 && cfg->n_traj <= (1 << 20), "n_traj out of range (1..1048576)");
    CIRS_REQUIRE(cfg->max_turn > 0 && cfg->max_turn <= 16383, "max_turn out of range (1..16383)");
    CIRS_REQUIRE(cfg->num_leave_compute >= 0, "num_leave_compute must be >= 0");
    CIRS_REQUIRE(cfg->epsilon >= 0.0 && cfg->epsilon <= 1.0, "epsilon out of range (0..1)");
    CIRS_REQUIRE(cfg->leave_threshold == cfg->leave_threshold, "leave_threshold is NaN");
    const cirs_vtb_mmoe_shape& p = cfg->policy;
    CIRS_REQUIRE(p.d_in == CIRS_VTB_STATIC_STATE_DIM, "unsupported policy shape: d_in must be 91 (the static state)");
    CIRS_REQUIRE(p.n_dnn >= 1 && p.n_dnn <= CIRS_VTB_STATIC_MAX_DNN, "unsupported policy shape: 1..3 hidden layers");
    for (int l = 0; l < p.n_dnn; ++l)
        CIRS_REQUIRE(p.hidden[l] >= 1 && p.hidden[l] <= kMmMaxHidden, "unsupported policy shape: hidden widths must lie in 1..256");
    CIRS_REQUIRE(p.experts >= 1 && p.expert_dim >= 1 && (long)p.experts * p.expert_dim <= kMmMaxED,
                 "unsupported policy shape: experts * expert_dim must lie in 1..64");
    CIRS_REQUIRE(p.n_tasks == 2 && p.task_dim[0] == kAct && p.task_dim[1] == 1,
                 "unsupported policy shape: exactly two tasks of logit dims (27, 1)");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int64_t cirs_vtb_static_workspace_bytes(const cirs_vtb_static_cfg* cfg) {
    using namespace cirs;
    if (validate_static(cfg) != CIRS_OK) return -1;
    return 12 * (int64_t)cfg->n_traj;   // double closs[n] | int32 clicks[n]
}

extern "C" int cirs_vtb_static_eval(const cirs_vtb_static_cfg* cfg, const cirs_vtb_weights* w, const cirs_vtb_mmoe_weights* pw, uint64_t seed,
                                    const cirs_vtb_static_out* out, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_static(cfg)) return rc;
    CIRS_REQUIRE(w != nullptr, "vtb weights is null");
    CIRS_REQUIRE(pw != nullptr, "policy weights is null");
    CIRS_REQUIRE(out != nullptr, "vtb static out is null");
    CIRS_REQUIRE(w->gen_w1 && w->gen_b1 && w->gen_w2 && w->gen_b2, "generator weight is null");
    CIRS_REQUIRE(w->act_w1 && w->act_b1 && w->act_w2 && w->act_b2 && w->act_w3 && w->act_b3, "action-model weight is null");
    for (int l = 0; l < cfg->policy.n_dnn; ++l) CIRS_REQUIRE(pw->dnn_w[l] && pw->dnn_b[l], "policy weight is null");
    CIRS_REQUIRE(pw->expert_w && pw->expert_b && pw->gate_w[0] && pw->gate_w[1] && pw->tower_w[0] && pw->tower_w[1] && pw->lin_w &&
                     pw->bias[0] && pw->bias[1],
                 "policy weight is null");
    CIRS_REQUIRE(out->user && out->state && out->action && out->reward_pred && out->reward && out->done && out->explore && out->metrics,
                 "vtb static out has a null field");
    CIRS_REQUIRE(workspace != nullptr, "workspace is null");
    CIRS_REQUIRE(workspace_bytes >= 12 * (int64_t)cfg->n_traj, "workspace too small (cirs_vtb_static_workspace_bytes)");
    CIRS_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out->metrics & 7) == 0, "workspace / metrics must be 8-byte aligned");
    double* ws_closs = static_cast<double*>(workspace);
    int32_t* ws_clicks = reinterpret_cast<int32_t*>(ws_closs + cfg->n_traj);
    hipLaunchKernelGGL(vtb_static_eval_kernel, dim3(cdiv(cfg->n_traj, kSRows)), dim3(kThreads), 0, (hipStream_t)stream, *cfg, *w, *pw, seed,
                       *out, ws_closs, ws_clicks);
    CIRS_CHECK_LAUNCH("vtb_static_eval_kernel");
    hipLaunchKernelGGL(vtb_static_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, cfg->n_traj, ws_closs, ws_clicks, out->metrics);
    CIRS_CHECK_LAUNCH("vtb_static_reduce_kernel");
    return CIRS_OK;
}

extern "C" int cirs_vtb_static_noise(uint64_t seed, const int32_t* traj_ids, const int32_t* turns, int32_t n, float* out, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(n >= 0, "n must be >= 0");
    if (n == 0) return CIRS_OK;
    CIRS_REQUIRE(traj_ids && turns && out, "null argument");
    const long blocks = ((long)n * CIRS_VTB_STATIC_NOISE_COLS + 255) / 256;   // 64-bit: n * 265 passes 2^31 for n > 8.1 M
    const int grid = blocks < 4096 ? (int)blocks : 4096;
    hipLaunchKernelGGL(vtb_static_noise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, seed, traj_ids, turns, n, out);
    CIRS_CHECK_LAUNCH("vtb_static_noise_kernel");
    return CIRS_OK;
}
