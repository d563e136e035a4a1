// rollout.hip -- the Collector hot loop as a stream of launches with no host synchronisation (reference:
// core/collector.py:219-317).  Per vector step: policy trunk + MFMA actor head + merge (policy.hip), env step
// (env.hip), tracker decode step (tracker.hip); finished envs propagate as act = -1 so no compaction is needed and
// every env keeps its row (RNG keyed by env id -> results independent of which other envs are still alive).
#include "env_kernels.h"
#include "internal.h"
#include "policy_kernels.h"

namespace cirs {

__global__ __launch_bounds__(256) void mark_visited_kernel(const int64_t* __restrict__ act, int n, int n_items,
                                                           uint32_t* __restrict__ visited) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long a = act[j];
    if (a < 0) return;
    const int words = (n_items + 31) / 32;
    atomicOr(&visited[(size_t)j * words + (a >> 5)], 1u << (a & 31));
}

// core/collector.py:253-258: with force_length every env's done flag is replaced by (cnt_loop >= force_length)
__global__ __launch_bounds__(256) void force_done_kernel(uint8_t* __restrict__ st_done, uint8_t* __restrict__ done_row,
                                                         const int64_t* __restrict__ act, int n, int force_done) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (act[j] < 0) return;
    st_done[j] = (uint8_t)force_done;
    done_row[j] = (uint8_t)force_done;
}

// rows -> (raw uid, raw pid, feats, duration) of the chosen pair; finished rows (act < 0) score item 0 and are ignored
__global__ __launch_bounds__(256) void online_pairs_kernel(const int32_t* __restrict__ env_user, const int64_t* __restrict__ act, int n,
                                                           cirs_online_reward o) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long a = act[j] < 0 ? 0 : act[j];
    o.uid_buf[j] = o.raw_uid[env_user[j]];
    o.pid_buf[j] = o.raw_pid[a];
#pragma unroll
    for (int q = 0; q < 4; ++q) o.feat_buf[(size_t)j * 4 + q] = o.item_feats[(size_t)a * 4 + q];
    o.dur_buf[j] = o.item_dur[a];
}

// sampler scratch (cirs_policy_workspace_bytes without its slack): the logit store sits behind it
static inline int64_t sampler_ws_bytes(const cirs_policy_cfg* cfg, int n) {
    return (int64_t)(ws_h2_floats(n) + 5 * ws_partial_elems(n, cfg->n_items)) * 4;
}

}  // namespace cirs

static int rollout_impl(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                        const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                        const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                        int32_t t_begin, int32_t t_end, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                        const cirs_online_reward* online, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream,
                        const cirs_redraw* redraw = nullptr, const int32_t* init_users = nullptr, bool greedy = false);

// Collector.reset_env + collect(n_episode = n_env) from ONE call (core/collector.py:123-134,147-367): env reset, the tracker's first position (from the packed
// weight image, the first step's trunk in its launch), the max_turn vector steps.  Every trajectory entry [t][env] is written (finished envs: act -1, done 1,
// rew / ctr 0), so the caller clears nothing; the tracker lengths restart at 1.
extern "C" int cirs_rollout_collect(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                    const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                                    const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                    const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    CIRS_REQUIRE(env_cfg && env_st && users && workspace && n_env > 0, "cirs_rollout_collect: null argument");
    CIRS_REQUIRE(workspace_bytes >= (int64_t)sizeof(int64_t) * n_env, "workspace too small");
    // (env.reset rides in the setup launch of rollout_impl; its obs ids -- the users -- land in the head of the workspace: scratch nobody reads)
    CIRS_REQUIRE(env_st->user && env_st->turn && env_st->done && env_st->hist_action && env_st->cum_reward, "env state has null field");
    return rollout_impl(env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj, n_env, 0, env_cfg->max_turn, seed, rng_base, visited, force_length,
                        nullptr, nullptr, workspace, workspace_bytes, stream, nullptr, users);
}

extern "C" int cirs_rollout_steps_redraw(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                         const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                                         const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                         int32_t t_begin, int32_t t_end, uint64_t seed, uint32_t rng_base, const cirs_redraw* redraw,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
    CIRS_REQUIRE(redraw && redraw->row_env && redraw->row_t && redraw->offsets && redraw->lens && redraw->workspace, "cirs_rollout_steps_redraw: null field");
    return rollout_impl(env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj, n_env, t_begin, t_end, seed, rng_base, nullptr, 0,
                        nullptr, nullptr, workspace, workspace_bytes, stream, redraw);
}

extern "C" int cirs_rollout_steps_noise(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                        const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                                        const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                                        int32_t n_env, int32_t t_begin, int32_t t_end, const float* gumbel, uint32_t* visited,
                                        int32_t force_length, void* workspace, int64_t workspace_bytes, void* stream) {
    CIRS_REQUIRE(gumbel, "cirs_rollout_steps_noise: gumbel is null (use cirs_rollout_steps for the counter-based sampler)");
    return rollout_impl(env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj, n_env, t_begin, t_end, 0, 0, visited,
                        force_length, nullptr, gumbel, workspace, workspace_bytes, stream);
}

// deterministic_eval (reference core/policy/ppo.py:149-151: act = logits_masked.argmax(-1) in eval mode): the fused two-launch sequence with the no-noise
// head kernel in place of the sampler and the step kernel's tail merging its partials -- the form the harness-noise rollout runs.  visited, force_length,
// env step, tracker decode and trunk are the sampled rollout's.  No noise is drawn: there is no seed / rng_base.
extern "C" int cirs_rollout_steps_greedy(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                         const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                                         const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                         int32_t t_begin, int32_t t_end, uint32_t* visited, int32_t force_length, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
    CIRS_REQUIRE(env_tab != nullptr, "cirs_rollout_steps_greedy: null argument");
    CIRS_REQUIRE(env_tab->pred_online == nullptr, "greedy rollout: the online-reward loop has no greedy mode (tables with pred_online are refused)");
    return rollout_impl(env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj, n_env, t_begin, t_end, 0, 0, visited, force_length,
                        nullptr, nullptr, workspace, workspace_bytes, stream, nullptr, nullptr, true);
}

// cirs_rollout_collect with the arg-max action of core/policy/ppo.py:149-151 (see cirs_rollout_steps_greedy)
extern "C" int cirs_rollout_collect_greedy(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                           const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                                           const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                           const int32_t* users, uint32_t* visited, int32_t force_length, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
    CIRS_REQUIRE(env_cfg && env_tab && env_st && users && workspace && n_env > 0, "cirs_rollout_collect_greedy: null argument");
    CIRS_REQUIRE(env_tab->pred_online == nullptr, "greedy rollout: the online-reward loop has no greedy mode (tables with pred_online are refused)");
    CIRS_REQUIRE(workspace_bytes >= (int64_t)sizeof(int64_t) * n_env, "workspace too small");
    CIRS_REQUIRE(env_st->user && env_st->turn && env_st->done && env_st->hist_action && env_st->cum_reward, "env state has null field");
    return rollout_impl(env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj, n_env, 0, env_cfg->max_turn, 0, 0, visited, force_length,
                        nullptr, nullptr, workspace, workspace_bytes, stream, nullptr, users, true);
}

namespace cirs {
// One unfused vector step: policy(obs_t), visited bit, the optional user-model scorer, env step, forced length, tracker step.  `tracker_step(act_t, rew_t,
// obs_n)` appends one position for every env that acted; `online` (nullable) scores the chosen pairs between the policy and the env step.
template <class TrackerStep>
static int unfused_vector_step(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st, const cirs_policy_cfg* pol_cfg,
                               const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env, long S, int t, uint64_t seed, uint32_t rng_base,
                               uint32_t* visited, int32_t force_length, bool greedy, const float* gumbel, const cirs_online_reward* online, void* workspace,
                               int64_t workspace_bytes, void* stream, TrackerStep tracker_step) {
    const long B = n_env;
    hipStream_t s = (hipStream_t)stream;
    float* obs_t = traj->obs + (size_t)t * B * S;
    float* obs_n = traj->obs + (size_t)(t + 1) * B * S;
    int64_t* act_t = traj->act + (size_t)t * B;
    double* rew_t = traj->rew + (size_t)t * B;
    uint8_t* done_t = traj->done + (size_t)t * B;
    // policy(obs_t): finished envs (env_st->done) are skipped and get act = -1
    if (greedy) {
        if (int rc = cirs_actor_greedy(pol_cfg, pol_w, obs_t, S, n_env, nullptr, visited, env_st->done, act_t, traj->logp + (size_t)t * B,
                                       traj->value + (size_t)t * B, workspace, workspace_bytes, stream))
            return rc;
    } else {
        if (int rc = cirs_actor_sample(pol_cfg, pol_w, obs_t, S, n_env, gumbel ? gumbel + (size_t)t * B * pol_cfg->n_items : nullptr, seed,
                                       rng_base + (uint32_t)t, nullptr, visited, env_st->done, act_t, traj->logp + (size_t)t * B,
                                       traj->value + (size_t)t * B, workspace, workspace_bytes, stream))
            return rc;
    }
    if (visited) {
        hipLaunchKernelGGL(mark_visited_kernel, dim3(cdiv(n_env, 256)), dim3(256), 0, s, act_t, n_env, pol_cfg->n_items, visited);
        CIRS_CHECK_LAUNCH("mark_visited_kernel");
    }
    if (online) {   // score the chosen (user, item) pairs with the DeepFM user model
        hipLaunchKernelGGL(online_pairs_kernel, dim3(cdiv(n_env, 256)), dim3(256), 0, s, env_st->user, act_t, n_env, *online);
        CIRS_CHECK_LAUNCH("online_pairs_kernel");
        if (int rc = cirs_deepfm_forward(online->cfg, online->w, online->uid_buf, online->pid_buf, online->feat_buf, online->dur_buf, n_env, online->pred_buf,
                                         stream))
            return rc;
    }
    // env.step: obs_next id == action, so the int64 obs row doubles as scratch we do not keep
    if (int rc = cirs_env_step(env_cfg, env_tab, env_st, act_t, nullptr, n_env, (int64_t*)workspace, rew_t, done_t, traj->ctr + (size_t)t * B, nullptr, stream))
        return rc;
    if (force_length > 0) {
        hipLaunchKernelGGL(force_done_kernel, dim3(cdiv(n_env, 256)), dim3(256), 0, s, env_st->done, done_t, act_t, n_env, (t + 1 >= force_length) ? 1 : 0);
        CIRS_CHECK_LAUNCH("force_done_kernel");
    }
    // preprocess_fn(obs_next, rew): the tracker appends one position for every env that acted this step
    return tracker_step(act_t, rew_t, obs_n);
}

// cirs_rollout_collect with a slot tracker (gru_tracker.hip, lstm_tracker.hip, avg_tracker.hip, caser_tracker.hip, nextitnet_tracker.hip, stamp_tracker.hip,
// narm_tracker.hip, fmlp_tracker.hip): unfused_vector_step without the scorer, built from the public entry points -- about five launches per vector step against the fused Transformer
// collect's two.  One loop for all of them: `init` / `step` are the tracker's entry points, `what` names it in the messages.
template <class Cfg, class Weights, class State>
static int collect_recurrent(const char* what, int (*init)(const Cfg*, const Weights*, State*, const int32_t*, const int32_t*, int32_t, float*, int64_t, void*),
                             int (*step)(const Cfg*, const Weights*, State*, const int64_t*, const double*, const int32_t*, const uint8_t*, int32_t, float*,
                                         int64_t, void*),
                             const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st, const Cfg* trk_cfg, const Weights* trk_w,
                             State* trk_st, const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                             const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length, int32_t greedy,
                             const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    const std::string p = std::string(what) + " rollout: ";
    CIRS_REQUIRE(env_cfg && env_tab && env_st && trk_cfg && trk_w && trk_st && pol_cfg && pol_w && traj && users && workspace && n_env > 0, p + "null argument");
    CIRS_REQUIRE(env_tab->pred_online == nullptr, p + "the online-reward loop is not built for this tracker (tables with pred_online are refused)");
    CIRS_REQUIRE(!(greedy && gumbel), p + "greedy draws no noise, it cannot be combined with gumbel");
    CIRS_REQUIRE(traj->obs && traj->act && traj->rew && traj->done && traj->logp && traj->value && traj->ctr, "trajectory pointer null");
    CIRS_REQUIRE(env_st->user && env_st->turn && env_st->done && env_st->hist_action && env_st->cum_reward, "env state has null field");
    CIRS_REQUIRE(trk_cfg->n_env == n_env, "tracker n_env mismatch");
    CIRS_REQUIRE(trk_cfg->dim_state == pol_cfg->dim_state, "tracker/policy dim_state mismatch");
    CIRS_REQUIRE(trk_cfg->max_len >= env_cfg->max_turn + 1, "tracker max_len < max_turn + 1");
    CIRS_REQUIRE(pol_cfg->n_items == env_cfg->n_items && trk_cfg->n_items == env_cfg->n_items, "policy/env/tracker n_items mismatch");
    CIRS_REQUIRE(workspace_bytes >= cirs_policy_workspace_bytes(pol_cfg, n_env) && workspace_bytes >= (int64_t)sizeof(int64_t) * n_env, "workspace too small");
    const long S = trk_cfg->dim_state;
    if (int rc = cirs_env_reset(env_cfg, env_st, users, nullptr, n_env, nullptr, stream)) return rc;
    if (int rc = init(trk_cfg, trk_w, trk_st, users, nullptr, n_env, traj->obs, S, stream)) return rc;
    auto tracker_step = [&](const int64_t* act_t, const double* rew_t, float* obs_n) {
        return step(trk_cfg, trk_w, trk_st, act_t, rew_t, nullptr, nullptr, n_env, obs_n, S, stream);
    };
    for (int t = 0; t < env_cfg->max_turn; ++t)
        if (int rc = unfused_vector_step(env_cfg, env_tab, env_st, pol_cfg, pol_w, traj, n_env, S, t, seed, rng_base, visited, force_length, greedy != 0, gumbel,
                                         nullptr, workspace, workspace_bytes, stream, tracker_step))
            return rc;
    return CIRS_OK;
}
}  // namespace cirs

extern "C" int cirs_rollout_collect_gru(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                        const cirs_gru_cfg* trk_cfg, const cirs_gru_weights* trk_w, cirs_gru_state* trk_st,
                                        const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                        const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                        int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("gru", cirs_gru_tracker_init, cirs_gru_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj,
                                   n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_collect_lstm(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                         const cirs_lstm_cfg* trk_cfg, const cirs_lstm_weights* trk_w, cirs_lstm_state* trk_st,
                                         const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                         const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                         int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("lstm", cirs_lstm_tracker_init, cirs_lstm_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj,
                                   n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_collect_avg(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                        const cirs_avg_cfg* trk_cfg, const cirs_avg_weights* trk_w, cirs_avg_state* trk_st,
                                        const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                        const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                        int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("avg", cirs_avg_tracker_init, cirs_avg_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj,
                                   n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_collect_caser(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                          const cirs_caser_cfg* trk_cfg, const cirs_caser_weights* trk_w, cirs_caser_state* trk_st,
                                          const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                          const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                          int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("caser", cirs_caser_tracker_init, cirs_caser_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w,
                                   traj, n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_collect_nextitnet(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                              const cirs_nextitnet_cfg* trk_cfg, const cirs_nextitnet_weights* trk_w, cirs_nextitnet_state* trk_st,
                                              const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                              const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                              int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("nextitnet", cirs_nextitnet_tracker_init, cirs_nextitnet_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st,
                                   pol_cfg, pol_w, traj, n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes,
                                   stream);
}

extern "C" int cirs_rollout_collect_stamp(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                          const cirs_stamp_cfg* trk_cfg, const cirs_stamp_weights* trk_w, cirs_stamp_state* trk_st,
                                          const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                          const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                          int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("stamp", cirs_stamp_tracker_init, cirs_stamp_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w,
                                   traj, n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_collect_narm(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                         const cirs_narm_cfg* trk_cfg, const cirs_narm_weights* trk_w, cirs_narm_state* trk_st,
                                         const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                         const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                         int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("narm", cirs_narm_tracker_init, cirs_narm_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w,
                                   traj, n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_collect_fmlp(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                         const cirs_fmlp_cfg* trk_cfg, const cirs_fmlp_weights* trk_w, cirs_fmlp_state* trk_st,
                                         const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                         const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                         int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("fmlp", cirs_fmlp_tracker_init, cirs_fmlp_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w,
                                   traj, n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_collect_lru(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                        const cirs_lru_cfg* trk_cfg, const cirs_lru_weights* trk_w, cirs_lru_state* trk_st,
                                        const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                        const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                                        int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs::collect_recurrent("lru", cirs_lru_tracker_init, cirs_lru_tracker_step, env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w,
                                   traj, n_env, users, seed, rng_base, visited, force_length, greedy, gumbel, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_steps(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                  const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w,
                                  cirs_tracker_state* trk_st, const cirs_policy_cfg* pol_cfg,
                                  const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                  int32_t t_begin, int32_t t_end, uint64_t seed, uint32_t rng_base, uint32_t* visited,
                                  int32_t force_length, void* workspace, int64_t workspace_bytes, void* stream) {
    return cirs_rollout_steps_online(env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj, n_env, t_begin, t_end,
                                     seed, rng_base, visited, force_length, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int cirs_rollout_steps_online(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                  const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w,
                                  cirs_tracker_state* trk_st, const cirs_policy_cfg* pol_cfg,
                                  const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                                  int32_t t_begin, int32_t t_end, uint64_t seed, uint32_t rng_base, uint32_t* visited,
                                  int32_t force_length, const cirs_online_reward* online, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    return rollout_impl(env_cfg, env_tab, env_st, trk_cfg, trk_w, trk_st, pol_cfg, pol_w, traj, n_env, t_begin, t_end, seed, rng_base,
                        visited, force_length, online, nullptr, workspace, workspace_bytes, stream);
}

// gumbel (nullable): harness-supplied sampler noise [max_turn][n_env][n_items] (g = -log q), row t used at vector step t
static int rollout_impl(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                        const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                        const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                        int32_t t_begin, int32_t t_end, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                        const cirs_online_reward* online, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream,
                        const cirs_redraw* redraw, const int32_t* init_users, bool greedy) {
    using namespace cirs;
    cirs_env_tables tab_local;
    CIRS_REQUIRE(!greedy || (!online && !redraw && !gumbel), "greedy rollout: not available with online reward, exact redraw or harness noise");
    const bool merge_tail = gumbel || greedy;     // the head kernel's partials are merged in the step kernel's tail (no pick)
    if (online) {
        CIRS_REQUIRE(env_tab && online->cfg && online->w && online->raw_uid && online->raw_pid && online->item_feats && online->item_dur &&
                     online->pred_minmax && online->uid_buf && online->pid_buf && online->feat_buf && online->dur_buf && online->pred_buf,
                     "online reward: null field");
        tab_local = *env_tab;
        tab_local.pred_online = online->pred_buf;
        tab_local.pred_minmax = online->pred_minmax;
        env_tab = &tab_local;
    }
    CIRS_REQUIRE(env_cfg && env_tab && env_st && trk_cfg && trk_w && trk_st && pol_cfg && pol_w && traj, "null argument");
    CIRS_REQUIRE(traj->obs && traj->act && traj->rew && traj->done && traj->logp && traj->value && traj->ctr, "trajectory pointer null");
    CIRS_REQUIRE(n_env > 0 && t_begin >= 0 && t_end <= env_cfg->max_turn && t_begin <= t_end, "bad step range");
    CIRS_REQUIRE(trk_cfg->n_env == n_env, "tracker n_env mismatch");
    CIRS_REQUIRE(trk_cfg->dim_state == pol_cfg->dim_state, "tracker/policy dim_state mismatch");
    CIRS_REQUIRE(trk_cfg->max_len >= env_cfg->max_turn + 1, "tracker max_len < max_turn + 1");
    const long B = n_env, S = trk_cfg->dim_state;
    hipStream_t s = (hipStream_t)stream;
    if (online) {  // per-step user-model scoring sits between the policy and the env step: unfused launch sequence
        auto tracker_step = [&](const int64_t* act_t, const double* rew_t, float* obs_n) {
            return cirs_tracker_step(trk_cfg, trk_w, trk_st, act_t, rew_t, nullptr, nullptr, n_env, obs_n, S, stream);
        };
        for (int t = t_begin; t < t_end; ++t)
            if (int rc = unfused_vector_step(env_cfg, env_tab, env_st, pol_cfg, pol_w, traj, n_env, S, t, seed, rng_base, visited, force_length, false, gumbel,
                                             online, workspace, workspace_bytes, stream, tracker_step))
                return rc;
        return CIRS_OK;
    }
    // ---- fused sequence: 2 launches per vector step ------------------------------------------------------------
    //   actor_head_kernel           MFMA head + Gumbel-max partials            (trunk of obs_t already in the workspace)
    //   tracker_step_kernel         one wavefront per env: merge -> act/logp, visited bit, env step, forced length (TailFuse);
    //                               tracker decode step; the policy trunk of obs_{t+1} (TrunkFuse)
    CIRS_REQUIRE(pol_cfg->hidden == kH && pol_cfg->dim_state == S && pol_cfg->n_items == env_cfg->n_items, "policy/env/tracker shape mismatch");
    CIRS_REQUIRE(pol_w->w1 && pol_w->b1 && pol_w->w2 && pol_w->b2 && pol_w->wa && pol_w->ba && pol_w->wc && pol_w->bc, "policy weight pointer null");
    CIRS_REQUIRE(workspace_bytes >= cirs_policy_workspace_bytes(pol_cfg, n_env), "workspace too small");
    CIRS_REQUIRE(env_tab->item_cats && (env_tab->normed_mat || !env_cfg->simulated) && (env_tab->mat || env_cfg->simulated), "env tables incomplete");
    if (t_begin >= t_end) return CIRS_OK;
    // packed weight image of the step kernel (tracker + policy trunk), rebuilt per call (the weights change between calls)
    float* img = (float*)((char*)workspace + ((workspace_bytes - kTrkImgBytes) & ~(int64_t)255));
    // ... the fp16 planes of the actor head for the chunk-mass kernels, likewise once per call, and (cirs_rollout_collect) env.reset: one launch
    uint4* rplanes = ws_rplanes(workspace, workspace_bytes, pol_cfg->n_items);
    if (int rc = pack_tracker_image(trk_cfg, trk_w, pol_w, S, img, s, pol_w->wa, pol_cfg->n_items, merge_tail ? nullptr : rplanes, init_users ? env_cfg : nullptr, env_st,
                                    init_users, n_env, (int64_t*)workspace))
        return rc;
    // sampler scratch at the head of the workspace (the kernels below take the env id of their row 0: always 0 here)
    const int n_pad = n_pad_of(n_env);
    const int n_mass_chunks = n_chunks_of(pol_cfg->n_items);
    float* h2 = (float*)workspace;
    const ActorPartialView pv = partial_view(workspace, n_env, pol_cfg->n_items);
    const HeadGrid hg = sampler_grid(pol_cfg->n_items, n_pad);
    const int cpw = mass_chunks_per_wg(n_mass_chunks, hg.n_row_blocks);
    // logit store (counter-based sampler, small env counts): behind the sampler scratch
    float* zstore = nullptr;
    if (!merge_tail && ws_zstore_floats(n_env, pol_cfg->n_items) > 0) {
        const char* ev = getenv("CIRS_ROLLOUT_ZSTORE");     // read per call (like CIRS_PPO_MERGE_KERNEL): a test may flip it between collects
        if (ev ? atoi(ev) != 0 : true) zstore = (float*)((char*)workspace + ((sampler_ws_bytes(pol_cfg, n_env) + 255) & ~(int64_t)255));
    }
    const char* ms_ev = getenv("CIRS_ROLLOUT_MASS_SMALL");   // per call as well
    const bool mass_small = (ms_ev ? atoi(ms_ev) != 0 : true) && !merge_tail && n_pad <= 128;
    const uint8_t* done_all = (const uint8_t*)env_st->done;
    // Exact-redraw dropout (the reference's procedure, core/state_tracker.py:170-186,243-246): the state of vector step t is NOT the cached decode's -- it is
    // ONE batched causal pass over positions 0 .. t of every env with the masks of build_state call t (cirs_tracker_prefix_states, key = the collect's key with
    // pseudo-env ids env_base0 + t * env_stride + e), followed by the trunk of that state; the step kernel keeps writing the input slots and its own state is
    // overwritten by the next call's pass.  (cirs_hip/redraw.py ran this loop from Python: ~18 launches and torch ops per step, host-bound.)
    // with_trunk: the policy trunk of the call's states (vector step t acts on them) rides in the prefix pass's launch when that is one launch, else trunk_kernel follows
    auto redraw_state = [&](int t, bool with_trunk) -> int {
        cirs_tracker_cfg cfg_t = *trk_cfg;
        cfg_t.dropout_seed = redraw->dropout_seed;
        cfg_t.drop_env_base = (int32_t)(redraw->env_base0 + (int64_t)t * redraw->env_stride);
        const size_t start = (size_t)B * t * (t + 1) / 2;
        TrunkFuse tf{};
        if (with_trunk) { tf.on = 1; tf.cfg = *pol_cfg; tf.w = *pol_w; tf.skip = done_all; tf.h2 = h2; tf.value = traj->value + (size_t)t * B; }
        int fused = 0;
        if (int rc = tracker_prefix_states_trunk(&cfg_t, trk_w, trk_st, redraw->row_env + start, redraw->row_t + start, redraw->offsets + (size_t)t * B,
                                                 redraw->lens + (size_t)t * B, (int32_t)(B * (t + 1)), traj->obs + (size_t)t * B * S, S, redraw->workspace,
                                                 redraw->workspace_bytes, stream, &tf, &fused))
            return rc;
        if (with_trunk && !fused) {
            hipLaunchKernelGGL(trunk_kernel, dim3(cdiv(n_env, 4)), dim3(256), 0, s, *pol_cfg, *pol_w, traj->obs + (size_t)t * B * S, (long)S, n_env, done_all, h2,
                               traj->value + (size_t)t * B, (float*)nullptr);
            CIRS_CHECK_LAUNCH("trunk_kernel");
        }
        return CIRS_OK;
    };
    // cirs_rollout_collect: the tracker's first position (Collector.reset_env's preprocess_fn(obs = ...)) from the packed image, with the trunk of the first
    // vector step in its launch -- cirs_tracker_init's row-major weight reads were 23 us per collect, the separate trunk launch 6
    bool first_trunk_done = false;
    if (init_users) {
        TrunkFuse tf0{};
        if (!redraw) {
            tf0.on = 1; tf0.cfg = *pol_cfg; tf0.w = *pol_w; tf0.skip = nullptr; tf0.h2 = h2; tf0.value = traj->value + (size_t)t_begin * B;
            first_trunk_done = true;
        }
        if (int rc = tracker_step_internal(trk_cfg, trk_w, trk_st, init_users, nullptr, nullptr, nullptr, nullptr, n_env, traj->obs + (size_t)t_begin * B * S, S, &tf0, s,
                                           nullptr, img))
            return rc;
    }
    if (redraw) { if (int rc = redraw_state(t_begin, true)) return rc; }
    // trunk of the first step of this call (later ones ride on the tracker step)
    if (!redraw && !first_trunk_done)
        hipLaunchKernelGGL(trunk_kernel, dim3(cdiv(n_env, 4)), dim3(256), 0, s, *pol_cfg, *pol_w, traj->obs + (size_t)t_begin * B * S, (long)S, n_env, done_all,
                           h2, traj->value + (size_t)t_begin * B, (float*)nullptr);
    CIRS_CHECK_LAUNCH("trunk_kernel");
    for (int t = t_begin; t < t_end; ++t) {
        const float* gum_t = gumbel ? gumbel + (size_t)t * B * pol_cfg->n_items : (const float*)nullptr;
        float* obs_n = traj->obs + (size_t)(t + 1) * B * S;
        int64_t* act_t = traj->act + (size_t)t * B;
        double* rew_t = traj->rew + (size_t)t * B;
        uint8_t* done_t = traj->done + (size_t)t * B;
        if (gum_t) {   // harness-supplied noise: plain Gumbel-max over the catalogue (reference-recorded fixtures)
            CIRS_PROF_LAUNCH(3, s, hipLaunchKernelGGL(actor_head_kernel<kNoiseHarness>, dim3(hg.grid_x, hg.n_row_blocks), dim3(256), 0, s, *pol_cfg,
                                                      pol_w->wa, pol_w->ba, (const float*)h2, n_env, gum_t, seed,
                                                      rng_base + (uint32_t)t, (const int32_t*)nullptr, (const uint32_t*)visited,
                                                      done_all, pv, n_pad, hg.tiles_per_chunk));
        } else if (greedy) {   // no noise: the arg-max of the masked logits (core/policy/ppo.py:149-151)
            CIRS_PROF_LAUNCH(3, s, hipLaunchKernelGGL(actor_head_kernel<kNoiseNone>, dim3(hg.grid_x, hg.n_row_blocks), dim3(256), 0, s, *pol_cfg,
                                                      pol_w->wa, pol_w->ba, (const float*)h2, n_env, (const float*)nullptr, (uint64_t)0, 0u,
                                                      (const int32_t*)nullptr, (const uint32_t*)visited, done_all, pv, n_pad, hg.tiles_per_chunk));
        } else if (mass_small) {   // few envs: one workgroup per chunk, one wave per (row tile, item tile)
            CIRS_PROF_LAUNCH(3, s, hipLaunchKernelGGL(actor_mass_small_kernel, dim3(n_mass_chunks), dim3(n_pad / kTileM * 256), 0, s, *pol_cfg, (const uint4*)rplanes,
                                                      pol_w->ba, (const float*)h2, n_env, (const uint32_t*)visited, done_all, pv.m, n_pad, 0, zstore));
        } else {       // counter-based sampler: chunk log-masses now, chunk + item draws in the tail of the step kernel
            CIRS_PROF_LAUNCH(3, s, hipLaunchKernelGGL(actor_mass_kernel, dim3(cdiv(n_mass_chunks, cpw), hg.n_row_blocks), dim3(kMassThreads), 0,
                                                      s, *pol_cfg, (const uint4*)rplanes, pol_w->ba, (const float*)h2, n_env, (const int32_t*)nullptr,
                                                      (const uint32_t*)visited, done_all, pv.m, n_pad, cpw, 0, 0, 0, zstore));
        }
        CIRS_CHECK_LAUNCH("sampler kernel");
        TrunkFuse tf{};
        if (t + 1 < t_end && !redraw) {
            tf.on = 1; tf.cfg = *pol_cfg; tf.w = *pol_w; tf.skip = done_all; tf.h2 = h2;
            tf.value = traj->value + (size_t)(t + 1) * B;
        }
        // preprocess_fn(obs_next, rew): the tracker appends one position for every env that acted this step
        // ... in the same launch as the tail of this step: action / logp, visited bit, env step, forced length
        TailFuse tl{};
        tl.on = 1; tl.cfg = *env_cfg; tl.tab = *env_tab; tl.st = *env_st; tl.n_pad = n_pad; tl.n_chunks = hg.n_chunks; tl.pv = pv;
        tl.env_base = 0;
        tl.visited = visited; tl.force_length = force_length;
        if (!merge_tail) {
            tl.pick_on = 1;
            tl.pick = PickArgs{pv.m, n_pad, n_mass_chunks, pol_w->wa, pol_w->ba, h2, visited, pol_cfg->n_items, 0, 0, seed, rng_base + (uint32_t)t, zstore};
        }
        tl.force_done = (t + 1 >= force_length) ? 1 : 0;
        // (exact redraw: obs_{t+1} is overwritten by call t + 1's prefix pass below -- under the same condition -- so the cached decode is not run)
        tl.slot_only = redraw && (t + 1 < t_end || t + 1 < trk_cfg->max_len) ? 1 : 0;
        tl.act_out = act_t; tl.logp_out = traj->logp + (size_t)t * B; tl.rew_out = rew_t; tl.done_out = done_t;
        tl.ctr_out = traj->ctr + (size_t)t * B;
        if (int rc = tracker_step_internal(trk_cfg, trk_w, trk_st, nullptr, act_t, rew_t, nullptr, nullptr, n_env, obs_n, S, &tf, s, &tl, img))
            return rc;
        if (redraw && (t + 1 < t_end || t + 1 < trk_cfg->max_len)) {      // the state of call t + 1 (the last one: obs_next of the final step)
            if (int rc = redraw_state(t + 1, t + 1 < t_end)) return rc;
        }
    }
    return CIRS_OK;
}

#ifdef CIRS_MASS_PROF
extern "C" int cirs_debug_mass_prof(unsigned long long* out_host32) {
    return hipMemcpyFromSymbol(out_host32, HIP_SYMBOL(cirs::g_mass_prof), 32 * sizeof(unsigned long long)) == hipSuccess ? 0 : -2;
}
#endif
