/* cirs_hip.h -- C ABI of libcirs_hip.so: the MI355X (gfx950) implementation of the CIRS rollout + PPO hot path.
 *
 * The reference (chongminggao/CIRS-codes) is pure Python and has no FFI; the drop-in boundary is the set of
 * duck-typed Python protocols listed in SURVEY.md §8(b).  This header is the native seam underneath those
 * protocols: every entry point below replaces the chain of Python/NumPy/pandas/torch calls cited next to it
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes stub that binds it.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All data pointers are DEVICE (HBM) pointers owned by the
 *     caller unless the name ends in _h (host).  The library allocates nothing that outlives a call, except
 *     the small launch-time scratch documented per function.
 *   - `stream` is a hipStream_t passed as void*; every call is stream-ordered and returns immediately.
 *   - return value: 0 = ok, <0 = error (CIRS_E_*); cirs_last_error() gives a thread-local message.
 *   - ids are env-encoded (LabelEncoder positions) unless stated; tables are row-major.
 */
#ifndef CIRS_HIP_H
#define CIRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIRS_OK 0
#define CIRS_E_INVALID (-1) /* bad argument (null pointer, size out of range)          */
#define CIRS_E_LAUNCH (-2)  /* HIP launch / runtime error                              */
#define CIRS_E_UNSUPPORTED (-3)

#define CIRS_MAX_CATS_PER_ITEM 4 /* KuaiRec item_categories.json has feat0..feat3 (kuaishouEnv.py:92) */
#define CIRS_CAT_NONE 0xFFu

const char* cirs_last_error(void);
int cirs_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Environment: batched SimulatedEnv(KuaishouEnv)
 * replaces  core/env/simulatedEnv/simulated_env.py:111-193  (SimulatedEnv.step/_compute_exposure_effect/
 *           _compute_pred_reward/_add_action_to_history/_reset_history)
 *           environments/KuaishouRec/env/kuaishouEnv.py:161-231 (KuaishouEnv.step/_determine_whether_to_leave/reset)
 *           core/util.py:21-54 (compute_action_distance, compute_exposure, clip0)
 *           tianshou/env/venvs.py:175-252 (the serial DummyVectorEnv loop)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct cirs_env_cfg {
    int32_t n_users;           /* U = mat.shape[0]                                                            */
    int32_t n_items;           /* I = mat.shape[1]                                                            */
    int32_t max_turn;          /* KuaishouEnv.max_turn (kuaishouEnv.py:36)                                    */
    int32_t num_leave_compute; /* N, exit-rule window (kuaishouEnv.py:56,203)                                 */
    int32_t leave_threshold;   /* leave iff count[c] > leave_threshold (kuaishouEnv.py:212)                   */
    int32_t version;           /* 1: r/(1+e*)   2: r - e*   (simulated_env.py:102-107)                        */
    int32_t use_exposure;      /* SimulatedEnv.use_exposure_intervention (simulated_env.py:118)               */
    int32_t has_ab;            /* alpha_u/beta_i given (simulated_env.py:157)                                 */
    int32_t dist_mode;         /* 0: dense I x I float64 table (df_dist_small); 1: on-the-fly 1/Jaccard       */
    int32_t simulated;         /* 1: SimulatedEnv reward; 0: bare KuaishouEnv (reward = mat[u,a]) test envs   */
    double tau;                /* compute_exposure: tau <= 0 -> 0 (util.py:42-44)                             */
    double gamma_exposure;     /* simulated_env.py:166                                                        */
    double r_decay;            /* simulated_env.py:130-132                                                    */
} cirs_env_cfg;

typedef struct cirs_env_tables { /* read-only, shared by all envs */
    const double* mat;         /* [U,I] real watch ratio  (kuaishouEnv.py:172)                                */
    const double* normed_mat;  /* [U,I] min-max normalised DeepFM prediction (simulated_env.py:100)           */
    const double* dist;        /* [I,I] 1/Jaccard, +inf when disjoint (util.py:36); NULL when dist_mode==1   */
    const uint32_t* item_cats; /* [I] four u8 category ids per item, CIRS_CAT_NONE padded (kuaishouEnv.py:49)*/
    const double* alpha_env;   /* [U] alpha_u[raw uid of env user] widened to f64 (simulated_env.py:158-160)  */
    const double* beta_env;    /* [I] beta_i[raw pid of env item]                                             */
    /* online-reward mode (catalogues too large for a U x I table, BASELINE configs[4]): when pred_online != NULL the
     * predicted reward of row j is (pred_online[j] - pred_minmax[0]) / (pred_minmax[1] - pred_minmax[0]) in float64
     * instead of normed_mat[u,a] -- the reference's own online variant (simulated_env.py:88-98, commented out there)
     * with the normalisation of compute_normed_reward (kuaishouEnv.py:139-143) applied per pair. */
    const float* pred_online;  /* [n] raw DeepFM score of (user of row j, action of row j), or NULL              */
    const float* pred_minmax;  /* [2] global {min, max} of the raw scores                                        */
} cirs_env_tables;

typedef struct cirs_env_state { /* mutable, SoA, one entry per env (B envs) */
    int32_t* user;        /* [B]    cur_user                                                                  */
    int32_t* turn;        /* [B]    total_turn                                                                */
    uint8_t* done;        /* [B]    episode finished (stepping a finished env is a no-op)          */
    int32_t* hist_action; /* [B,T]  history_action / sequence_action                                          */
    double* cum_reward;   /* [B]    cum_reward of the reward actually returned                                */
} cirs_env_state;

/* reset envs `env_ids[0..n)` (NULL = 0..n-1) to users[0..n) (kuaishouEnv.py:182-190; the user draw itself is
 * the caller's: the reference uses an unseeded random.randint).  obs_out[n] (nullable) = user id. */
int cirs_env_reset(const cirs_env_cfg* cfg, cirs_env_state* st, const int32_t* users, const int32_t* env_ids,
                   int32_t n, int64_t* obs_out, void* stream);

/* one vector step.  actions[n] are env-encoded item ids; outputs are indexed like env_ids (position j).
 *   obs_out[n]  int64   state = last action (kuaishouEnv.py:147-153)
 *   rew_out[n]  double  reward
 *   done_out[n] uint8   leave OR t >= max_turn-1 (kuaishouEnv.py:167-169)
 *   ctr_out[n]  double  info['CTR'] = cum_reward/total_turn/10 (simulated_env.py:145); bare env: cum_reward
 *   expo_out[n] double  (nullable) exposure_gamma e* stored in history_exposure[t] (simulated_env.py:166,190) */
int cirs_env_step(const cirs_env_cfg* cfg, const cirs_env_tables* tab, cirs_env_state* st, const int64_t* actions,
                  const int32_t* env_ids, int32_t n, int64_t* obs_out, double* rew_out, uint8_t* done_out,
                  double* ctr_out, double* expo_out, void* stream);

/* dense 1/Jaccard distance table from packed categories: replaces core/util.py:225-273 (get_distance_mat /
 * get_similarity_mat restricted to the env items).  dist_out is [I,I] float64. */
int cirs_dist_jaccard(const uint32_t* item_cats, int32_t n_items, double* dist_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker: incremental (KV-cached) StateTrackerTransformer
 * replaces  core/state_tracker.py:89-115 (get_embedding), :170-186 (forward), :188-250 (build_state)
 *           torch.nn.TransformerEncoder(2 x post-norm TransformerEncoderLayer, relu, eps 1e-5), eval mode
 * The reference re-runs the causal transformer over the whole prefix every step (O(L^2) per step); because the
 * mask is causal and only output[-1] is used, caching each layer's K/V per position is exact.
 * Fixed dims of this build: dim_model == 32, d_hid == 128, dim_state <= 32, nhead in {1,2,4,8}, nlayers <= 4.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_MAX_TRACKER_LAYERS 4

typedef struct cirs_tracker_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S = 20 */
    int32_t nhead;     /* 4 */
    int32_t d_hid;     /* 128 */
    int32_t nlayers;   /* 2 */
    int32_t max_len;   /* MAX_TURN + 1 (state_tracker.py:144) */
    int32_t n_env;     /* B: leading dimension of the state arrays */
    /* dropout (production mode; 0 = off, the mode every reference-recorded fixture uses).  The reference runs the tracker with
     * nn.Dropout(0.1) live in rollout, test and backward (core/state_tracker.py:155-156,176; never eval(), CIRS-RL-kuaishou.py:235-243).
     * Masks are counter-based: a pure function of (dropout_seed, drop_env_base + env, position, layer, site, element), see csrc/rng.h. */
    float dropout_p;
    int32_t drop_env_base; /* added to the local env index: global env id of the job (rank * n_env), same in forward and backward */
    uint64_t dropout_seed; /* changes per collect (seed, collect counter) */
} cirs_tracker_cfg;

typedef struct cirs_tracker_layer { /* names: transformer_encoder.layers.<l>.*  */
    const float *in_proj_w, *in_proj_b;   /* [3D,D], [3D] */
    const float *out_proj_w, *out_proj_b; /* [D,D], [D]   */
    const float *lin1_w, *lin1_b;         /* [H,D], [H]   */
    const float *lin2_w, *lin2_b;         /* [D,H], [D]   */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b; /* [D] */
} cirs_tracker_layer;

typedef struct cirs_tracker_weights {
    const float* emb_user;                 /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                 /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b;  /* [D,D], [D]   */
    const float *gate_w, *gate_b;          /* fnn_gate [D,1+D] (input order [r, a], state_tracker.py:240), [D] */
    const float* pe;                       /* pos_encoder.pe [max_len, D] */
    cirs_tracker_layer layer[CIRS_MAX_TRACKER_LAYERS];
    const float *dec_w, *dec_b;            /* decoder [S,D], [S] */
} cirs_tracker_weights;

typedef struct cirs_tracker_state {
    float* x_hist;  /* [B, max_len, D]  self.data: slot 0 = user projection, slot k = gated action (state_tracker.py:198,215,242) */
    float* kcache;  /* nlayers * B * max_len * D floats; per (layer, env) laid out [D/4][max_len][4] (private to the library) */
    float* vcache;  /* [nlayers, B, max_len, D] */
    int32_t* len;   /* [B] self.len_data */
} cirs_tracker_state;

/* build_state(obs=users): len=1, slot 0, s0 -> state_out[j*state_stride + 0..S) for j in [0,n). */
int cirs_tracker_init(const cirs_tracker_cfg* cfg, const cirs_tracker_weights* w, cirs_tracker_state* st,
                      const int32_t* users, const int32_t* env_ids, int32_t n, float* state_out,
                      int64_t state_stride, void* stream);
/* build_state(obs_next=items, rew): append one position, return s_t.  `rew` is the env's float64 reward (cast to
 * float32 like FloatTensor(rew), state_tracker.py:97).  state_out row stride = state_stride floats.
 * skip (nullable, [n]): rows with skip != 0 are left untouched (finished envs). */
int cirs_tracker_step(const cirs_tracker_cfg* cfg, const cirs_tracker_weights* w, cirs_tracker_state* st,
                      const int64_t* items, const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n,
                      float* state_out, int64_t state_stride, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Policy: shared trunk + actor head over the full catalogue + fused sampler + critic
 * replaces  tianshou/utils/net/common.py:87-92,184-197 (MLP/Net), utils/net/discrete.py:56-67 (Actor), :113-114 (Critic)
 *           core/policy/ppo.py:111-163 (PPOPolicy.forward: softmax, optional mask of recommended ids, Categorical.sample)
 *           core/policy/utils.py:30-58 (removed_recommended_id_from_embedding)
 * The B x I probability matrix is never written to HBM: the head GEMM (fp32 MFMA 32x32x2), the Gumbel-max
 * sampler (== torch.multinomial's exponential race) and the log-sum-exp are fused; per-chunk partials are merged
 * by a second tiny kernel.  Arithmetic order is fixed (see oracle) so action indices are bit-reproducible.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct cirs_policy_cfg {
    int32_t n_items;   /* I */
    int32_t dim_state; /* 20 */
    int32_t hidden;    /* 64 (two hidden layers of this width) */
} cirs_policy_cfg;

typedef struct cirs_policy_weights {
    const float *w1, *b1; /* actor.preprocess.model.model.0 [H,S],[H] */
    const float *w2, *b2; /* actor.preprocess.model.model.2 [H,H],[H] */
    const float *wa, *ba; /* actor.last.model.0 [I,H],[I] */
    const float *wc, *bc; /* critic.last.model.0 [1,H],[1] */
} cirs_policy_weights;

/* bytes of caller-provided scratch for cirs_actor_sample / cirs_actor_logp / cirs_rollout_steps* with batch n (h2 rows, sampler
 * partials, and -- for the fused rollout -- 256 KB for the packed weight image of its step kernel, rebuilt by every call) */
int64_t cirs_policy_workspace_bytes(const cirs_policy_cfg* cfg, int32_t n);

/* For rows j in [0,n): h2 = trunk(state[j]); value = critic; act = argmax_i (logit_i + g_i) over unmasked items,
 * logp = log(clamp(softmax(logits)[act], eps, 1-eps)) (Categorical(probs).log_prob).
 *   state        [n, state_stride] f32
 *   gumbel       nullable [n, I] f32 harness-supplied noise g = -log(q); NULL -> counter-based Philox4x32-10 keyed by
 *                (seed, rng_step) with counter (item, env_id>>2, ...) so results do not depend on batch composition
 *   env_ids      nullable [n] global env id of each row (RNG key + visited row); NULL -> j
 *   visited      nullable [B, ceil(I/32)] u32 bitmap of already recommended ids (remove_recommended_ids)
 *   skip         nullable [n]: rows with skip != 0 produce act = -1 and are not computed
 *   act_out [n] i64, logp_out [n] f32 (nullable), value_out [n] f32 (nullable), h2_out [n,H] f32 (nullable) */
int cirs_actor_sample(const cirs_policy_cfg* cfg, const cirs_policy_weights* w, const float* state,
                      int64_t state_stride, int32_t n, const float* gumbel, uint64_t seed, uint32_t rng_step,
                      const int32_t* env_ids, const uint32_t* visited, const uint8_t* skip, int64_t* act_out,
                      float* logp_out, float* value_out, void* workspace, int64_t workspace_bytes, void* stream);

/* deterministic_eval of a discrete actor (reference core/policy/ppo.py:149-151: in eval mode act = logits_masked.argmax(-1)): cirs_actor_sample
 * without noise -- the same trunk, fp32 MFMA logits, visited mask, skip and merge; act = the unmasked item of largest logit (ties -> lowest id),
 * logp = its log-probability under the masked soft-max with cirs_actor_sample's clamp, value as always; skipped rows get act = -1.
 * workspace: cirs_policy_workspace_bytes(cfg, n). */
int cirs_actor_greedy(const cirs_policy_cfg* cfg, const cirs_policy_weights* w, const float* state, int64_t state_stride, int32_t n,
                      const int32_t* env_ids, const uint32_t* visited, const uint8_t* skip, int64_t* act_out, float* logp_out,
                      float* value_out, void* workspace, int64_t workspace_bytes, void* stream);

/* The policy's top-k list per row: the k (1..CIRS_TOPK_MAX) unmasked items of largest logit in descending order, ties -> the lower id first
 * (the arg-max rule of core/policy/ppo.py:149-151 continued down the ranking; the counterpart of UserModel.recommend_k_item for the RL policy).
 *   ids_out [n, k] i64, logp_out [n, k] f32 (nullable): logp as in cirs_actor_greedy; fewer than k unmasked items left: the tail is -1 / -inf;
 *   a skipped row is all -1 / -inf.  k = 1 returns cirs_actor_greedy's act and logp bit for bit (the same head kernel and merge).
 *   workspace: cirs_actor_topk_workspace_bytes(cfg, n, k) (0 for a k outside 1..CIRS_TOPK_MAX): the greedy scratch + the masked logits. */
#define CIRS_TOPK_MAX 32
int64_t cirs_actor_topk_workspace_bytes(const cirs_policy_cfg* cfg, int32_t n, int32_t k);
int cirs_actor_topk(const cirs_policy_cfg* cfg, const cirs_policy_weights* w, const float* state, int64_t state_stride, int32_t n, int32_t k,
                    const int32_t* env_ids, const uint32_t* visited, const uint8_t* skip, int64_t* ids_out, float* logp_out, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ---- column-sharded actor head + row-sharded tables (BASELINE configs[4]: catalogue / embedding tables split over the ranks) ----
 * The reference has no counterpart (deepctr_torch/inputs.py:31-33 only prints a notice for use_hash); the spec is SURVEY 8(e):
 * "actor head column-sharded over items with a cross-rank (max, sum-exp, sampled-candidate) reduction", "tables row-sharded by
 * id mod W, per step an all-to-all of requested ids and returned rows".  Semantics to match: cirs_actor_sample on one device.
 *
 * cirs_actor_shard_partials: THIS rank's item shard (cfg_shard->n_items items whose first global id is item_base, a multiple of
 * 128 = the sampler's chunk (chunk ids are item_base / 128: every shard but the last must hold a multiple of 128 items);
 * w_shard->wa / ba = the shard's rows, trunk / critic weights replicated) against n env rows (all envs of the job; env_ids =
 * their global ids).  Noise counters, the visited bitmap and candidate ids use GLOBAL item ids, so a shard computes exactly what
 * the full kernel computes for its items.  tuples_out [5, n] f32: {noisy score, candidate id (int32 bits), candidate logit,
 * running max, running sum-exp}.  cirs_actor_merge_shards: tuples [n_shards, 5, n] folded in shard order -> act (argmax of the
 * noisy score, ties -> lowest id: identical to the single-device action) and logp (Categorical clamp). */
/* critic(obs) for n stored states with the current parameters: the value pass of A2CPolicy._compute_returns
   (tianshou/tianshou/policy/modelfree/a2c.py:80-86) when PPOPolicy(recompute_advantage=True) recomputes the advantages at every repeat
   (core/policy/ppo.py:176-177).  workspace: cirs_policy_workspace_bytes(cfg, n). */
int cirs_critic_values(const cirs_policy_cfg* cfg, const cirs_policy_weights* w, const float* state, int64_t state_stride, int32_t n,
                       float* value_out, void* workspace, int64_t workspace_bytes, void* stream);

int cirs_actor_shard_partials(const cirs_policy_cfg* cfg_shard, const cirs_policy_weights* w_shard, const float* state,
                              int64_t state_stride, int32_t n, uint64_t seed, uint32_t rng_step, const int32_t* env_ids,
                              const uint32_t* visited, const uint8_t* skip, int32_t item_base, int32_t n_items_total,
                              float* tuples_out, float* value_out, void* workspace, int64_t workspace_bytes, void* stream);
int cirs_actor_merge_shards(const float* tuples, int32_t n_shards, int32_t n, const uint8_t* skip, int64_t* act_out,
                            float* logp_out, void* stream);
/* out[k, :] = table[idx[k], :] (zeros where idx[k] < 0) for a row-major fp32 table with row_floats (multiple of 4) floats per row: the local side of a
 * row-sharded nn.Embedding lookup (core/user_model.py:435-437, core/state_tracker.py:97-110 `embedding_dict[...](ids)`). */
int cirs_gather_rows(const float* table, int32_t row_floats, const int64_t* idx, int64_t n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-resident rollout: the Collector hot loop with no host round trip per step
 * replaces  core/collector.py:219-317 (policy forward -> env.step -> preprocess_fn -> buffer.add, per vector step)
 *           tianshou/data/buffer/manager.py:91-142 (ReplayBufferManager.add) -- the trajectory IS the buffer
 *           core/policy/utils.py:7-27 (get_recommended_ids) via the visited bitmap
 * Trajectory tensors are TIME-MAJOR so every step reads/writes contiguous [B, .] rows (the reference's tracker
 * history `data` is (L, B, D) too, state_tracker.py:198).  Row t of act/rew/done/logp/value/ctr belongs to the
 * transition (s_t, a_t, r_t, s_{t+1}); obs has T+1 rows.  Finished envs keep act = -1 from their first idle step.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct cirs_traj {
    float* obs;     /* [T+1, B, S] tracker states; row 0 written by cirs_tracker_init                         */
    int64_t* act;   /* [T, B]     env-encoded item id, -1 = env already finished                               */
    double* rew;    /* [T, B]     */
    uint8_t* done;  /* [T, B]     */
    float* logp;    /* [T, B]     log pi(a_t | s_t) at rollout time (== logp_old of ppo.py:104-108)            */
    float* value;   /* [T, B]     V(s_t) at rollout time    (== v_s of a2c.py:83-88)                           */
    double* ctr;    /* [T, B]     info['CTR'] (simulated) / cum_reward (bare env)                              */
} cirs_traj;

/* Run vector steps t in [t_begin, t_end) for all n_env envs: actor_sample(obs[t]) -> env_step -> tracker_step -> obs[t+1].
 *   rng_base      step t draws its sampler noise with rng_step = rng_base + t
 *   visited       nullable [B, ceil(I/32)] bitmap; when given, chosen ids are masked from later draws of the same
 *                 env (remove_recommended_ids, the NX_* test collectors) and the bitmap is updated each step
 *   force_length  > 0: done is overridden to (t+1 >= force_length) for every env (core/collector.py:253-258)
 *   workspace     >= cirs_policy_workspace_bytes(policy_cfg, n_env) */
struct cirs_deepfm_cfg;
struct cirs_deepfm_weights;
/* Online scoring of the chosen (user, item) pairs with the DeepFM user model between the policy and the env step. */
typedef struct cirs_online_reward {
    const struct cirs_deepfm_cfg* cfg;
    const struct cirs_deepfm_weights* w;
    const int64_t* raw_uid;     /* [U] raw id of env user (lbe_user.classes_)        */
    const int64_t* raw_pid;     /* [I] raw id of env item (lbe_photo.classes_)       */
    const int32_t* item_feats;  /* [I,4] feat ids (0 = padding)                      */
    const float* item_dur;      /* [I]                                               */
    const float* pred_minmax;   /* [2]                                               */
    int64_t* uid_buf;           /* [B] scratch                                       */
    int64_t* pid_buf;           /* [B] scratch                                       */
    int32_t* feat_buf;          /* [B,4] scratch                                     */
    float* dur_buf;             /* [B] scratch                                       */
    float* pred_buf;            /* [B] scratch: raw scores of this step              */
} cirs_online_reward;

int cirs_rollout_steps(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                       const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                       const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                       int32_t n_env, int32_t t_begin, int32_t t_end, uint64_t seed, uint32_t rng_base,
                       uint32_t* visited, int32_t force_length, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* Collector.reset_env + one collect(n_episode = n_env) from ONE call (core/collector.py:123-134: reset_env -> env.reset + preprocess_fn(obs = ...);
 * :147-367: the loop): env reset with users[n_env], the tracker's first position (cirs_tracker_init's arithmetic from the step kernel's packed weight image,
 * the first vector step's trunk in the same launch), then cirs_rollout_steps(0, max_turn).  Every trajectory entry [t][env] is written (envs that finished
 * earlier: act -1, done 1, rew / ctr 0), so nothing has to be cleared before the call. */
int cirs_rollout_collect(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                         const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                         const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                         int32_t n_env, const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited,
                         int32_t force_length, void* workspace, int64_t workspace_bytes, void* stream);
/* same loop with HARNESS-SUPPLIED sampler noise instead of the counter-based generator: gumbel [max_turn][n_env][n_items] f32,
 * g = -log q with q ~ Exp(1) (torch.multinomial's race noise, core/policy/ppo.py:148-155 `dist.sample()`), row t is used at
 * vector step t and indexed by ORIGINAL item id also when recommended ids are masked (core/policy/utils.py:30-58): the device
 * rollout then reproduces a reference Collector.collect whose Categorical.sample was fed the same q (parity fixtures). */
int cirs_rollout_steps_noise(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                             const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                             const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                             int32_t n_env, int32_t t_begin, int32_t t_end, const float* gumbel, uint32_t* visited,
                             int32_t force_length, void* workspace, int64_t workspace_bytes, void* stream);
/* cirs_rollout_steps / cirs_rollout_collect with the arg-max action of a policy built with deterministic_eval and put in eval()
 * (reference core/policy/ppo.py:149-151: act = logits_masked.argmax(-1)): the no-noise head kernel in place of the sampler, everything else
 * -- visited, force_length, env step, tracker decode (its dropout included), trunk -- as in the sampled rollout.  No noise is drawn, so there is
 * no seed / rng_base.  Precomputed reward tables only: the online-reward loop, the exact-redraw rollout and the column-sharded head have no greedy mode. */
int cirs_rollout_steps_greedy(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                              const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                              const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                              int32_t n_env, int32_t t_begin, int32_t t_end, uint32_t* visited, int32_t force_length,
                              void* workspace, int64_t workspace_bytes, void* stream);
int cirs_rollout_collect_greedy(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                                const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                                int32_t n_env, const int32_t* users, uint32_t* visited, int32_t force_length, void* workspace,
                                int64_t workspace_bytes, void* stream);
/* same, with the predicted reward scored online (env_tab->normed_mat may be NULL) */
int cirs_rollout_steps_online(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                              const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w,
                              cirs_tracker_state* trk_st, const cirs_policy_cfg* pol_cfg,
                              const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env, int32_t t_begin,
                              int32_t t_end, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                              const cirs_online_reward* online, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Learner: PPO update over the collected trajectories
 * replaces  tianshou/policy/base.py:219-244 (update), :271-313 (compute_episodic_return), :380-396 (_gae_return)
 *           tianshou/policy/modelfree/a2c.py:80-109 (_compute_returns), tianshou/utils/statistics.py:80-95 (RunningMeanStd)
 *           core/policy/ppo.py:96-109 (process_fn), :166-246 (learn), torch.optim.Adam, clip_grad_norm_
 * Rows are kept in BUFFER ORDER (VectorReplayBuffer: env-major concatenation of each env's episode), so minibatch
 * index arrays drawn from np.random.permutation(N) mean the same rows as in the reference (batch.py:734-744).
 * v_s / v_s_ / logp_old are the values recorded at rollout time: the policy has not changed since, so they equal
 * what process_fn recomputes (a2c.py:83-88, ppo.py:104-108).
 * Reference quirks kept: the shared trunk appears twice in the optimiser and in clip_grad_norm_ ->
 * its squared gradient norm counts twice, the clip coefficient is applied twice and every optimiser step runs two
 * sequential Adam sub-steps on the trunk.
 * Parameter / gradient / Adam-moment buffers are FLAT fp32 with the layout
 *   [ w1 (H*S) | b1 (H) | w2 (H*H) | b2 (H) | wa (I*H) | ba (I) | wc (H) | bc (1) ]     (trunk = first four)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct cirs_ppo_cfg {
    int32_t n_items, dim_state, hidden;
    int32_t norm_adv, value_clip, rew_norm;
    float gamma, gae_lambda, eps_clip, vf_coef, ent_coef, max_grad_norm;
    float lr, beta1, beta2, adam_eps;
    float dual_clip;   /* 0: off; > 1: dual-clip PPO as the reference computes it, -max(min(surr1, surr2), dual_clip * adv) for EVERY sign of
                          adv (core/policy/ppo.py:190-193) */
} cirs_ppo_cfg;

typedef struct cirs_ppo_batch { /* N rows, buffer order */
    float* obs;        /* [N,S]  s_t                                    */
    int32_t* act;      /* [N]                                           */
    float* adv;        /* [N]    GAE advantage (float32 of the float64) */
    float* ret;        /* [N]    normalised returns                     */
    float* v_s;        /* [N]    old value (normalised scale)           */
    float* logp_old;   /* [N]                                           */
    int32_t* row_env;  /* [N]    env of the row                         */
    int32_t* row_t;    /* [N]    turn of the row                        */
} cirs_ppo_batch;

int64_t cirs_ppo_param_count(const cirs_ppo_cfg* cfg);
int64_t cirs_ppo_workspace_bytes(const cirs_ppo_cfg* cfg, int32_t max_minibatch);

/* process_fn: GAE (float64) per env, return normalisation with the running variance, RunningMeanStd update, and
 * compaction of the time-major trajectory into buffer order.  lens[B] = episode lengths, offsets[B] = exclusive
 * prefix sum of lens (row of env b's first transition).  rms_state = {mean, var, count} (float64, device). */
int cirs_ppo_prepare(const cirs_ppo_cfg* cfg, const cirs_traj* traj, const int32_t* lens, const int32_t* offsets,
                     int32_t n_env, int32_t max_turn, int32_t n_rows, double* rms_state, const cirs_ppo_batch* out,
                     void* stream);
/* The same preparation with the row count left on the device: offsets_out [n_env] and n_rows_out [1] are formed from `lens` by the
   first kernel, so the call can be enqueued behind the rollout before the host has read the episode lengths (the read-back then
   overlaps with these kernels).  scratch: n_env * max_turn doubles; `out` sized for n_env * max_turn rows.  Same results, bit for bit. */
int cirs_ppo_prepare_async(const cirs_ppo_cfg* cfg, const cirs_traj* traj, const int32_t* lens, int32_t n_env, int32_t max_turn,
                           int32_t* offsets_out, int32_t* n_rows_out, double* rms_state, const cirs_ppo_batch* out, double* scratch,
                           void* stream);
/* cirs_ppo_prepare_async + the update's minibatch permutations (cirs_random_permutations(n_rows, perm_seed, perm_tag0, n_perm, ..), n_perm <= 8) from
 * process_fn's last launch, the row count read on the device: perm_out[c * n_rows + i], i < n_rows (buffer: n_perm * n_env * max_turn ints).
 * replaces  Batch.split(shuffle=True)'s np.random.permutation per repeat (tianshou/data/batch.py:734-744; core/policy/ppo.py:173-181). */
int cirs_ppo_prepare_async_perms(const cirs_ppo_cfg* cfg, const cirs_traj* traj, const int32_t* lens, int32_t n_env, int32_t max_turn,
                                 int32_t* offsets_out, int32_t* n_rows_out, double* rms_state, const cirs_ppo_batch* out, double* scratch,
                                 uint64_t perm_seed, uint64_t perm_tag0, int32_t n_perm, int32_t* perm_out, int32_t offsets_ready, void* stream);

/* one minibatch gradient step of learn(): forward, clipped surrogate + clipped value loss + entropy, backward,
 * clip_grad_norm_, Adam.  idx[mb] are buffer-order row ids.  opt_step = optimiser steps taken so far.
 * dobs_accum (nullable) [T+1, B, S]: d loss / d obs rows are written at (row_t, row_env) -- the gradient that flows
 * into the state tracker through the stored obs (ppo.py:215 retain_graph).  loss_out[4] = {loss, clip, vf, ent}. */
int cirs_ppo_minibatch(const cirs_ppo_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                       int64_t opt_step, const cirs_ppo_batch* batch, const int32_t* idx, int32_t mb,
                       float* dobs_accum, int32_t n_env, float* loss_out, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* PPOPolicy.learn's loop (core/policy/ppo.py:173-233: `for step in range(repeat): for minibatch in batch.split(batch_size, merge_last=True)`) from
 * ONE call: n_repeat passes over the n_rows buffer rows, pass r in the order perms[r * n_rows .. (r + 1) * n_rows) (device; the host's
 * np.random.permutation of Batch.split, tianshou/data/batch.py:721-752), cut into minibatches of batch_size rows with the remainder merged into the
 * last one (batch.py:734-744).  Every minibatch is exactly one cirs_ppo_minibatch step -- same kernels, same bits -- with optimiser step
 * opt_step + k; what the call adds is that step k's optimiser launch also runs the head of step k + 1 (trunk forward of its rows on the updated
 * weights, its advantage statistics, the bf16 planes of the updated Wa), so the loop has one launch less per step and the host leaves the loop's
 * critical path (one ctypes call per update instead of one per step).  dobs_accum (nullable, dobs_floats floats): zeroed before the LAST pass and
 * filled by it (ppo.py:174 zero_grad at the top of every repeat: only the last pass's d loss / d obs reaches the state tracker).
 * losses [cirs_ppo_learn_steps(n_rows, batch_size, n_repeat)][4] = {loss, clip, vf, ent} per step.  workspace: cirs_ppo_workspace_bytes(cfg, m)
 * for the largest minibatch m (< 2 * batch_size). */
int32_t cirs_ppo_learn_steps(int32_t n_rows, int32_t batch_size, int32_t n_repeat);
int cirs_ppo_learn(const cirs_ppo_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t opt_step,
                   const cirs_ppo_batch* batch, const int32_t* perms, int32_t n_rows, int32_t batch_size, int32_t n_repeat,
                   float* dobs_accum, int64_t dobs_floats, int32_t n_env, float* losses, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* Health of the in-launch hand-offs of the minibatch step (no reference counterpart: the reference's optimiser step, core/policy/ppo.py:215-233,
 * is a sequence of synchronous torch calls and cannot lose one).  Inside cirs_ppo_learn / cirs_ppo_minibatch* some workgroups wait for arrival
 * flags of other workgroups of the SAME launch (trunk backward rows -> gradient sums; trunk Adam -> the next step's trunk forward).  The wait is
 * bounded; a workgroup that gives up counts itself in a sticky device word.  This call enqueues (on `stream`) a copy of that count to lost_out
 * (device pointer, one int32) and, with reset != 0, clears it.  A non-zero count means the update it belongs to used incomplete sums or stale
 * weights: the host must treat the update as failed (cirs_hip/learner.py raises at the update's read-back). */
int cirs_ppo_handoff_status(int32_t* lost_out, int32_t reset, void* stream);
/* The one read-back of an update (the host needs the episode lengths to schedule the minibatches: len(buffer) in tianshou/policy/base.py:231-244) as one
 * launch: lens[n_env] and the hand-off count above written straight to PINNED host memory (device-accessible: hipHostMalloc); lost_host_pinned may be NULL.
 * offsets_out / n_rows_out (both or neither): process_fn's first job -- the buffer offsets of the envs and the row count, cirs_ppo_prepare_async's
 * outputs -- formed in the same launch; cirs_ppo_prepare_async_perms(.., offsets_ready = 1, ..) then starts at the GAE. */
int cirs_ppo_update_readback(const int32_t* lens, int32_t n_env, int32_t* lens_host_pinned, int32_t* lost_host_pinned, int32_t* offsets_out,
                             int32_t* n_rows_out, void* stream);

/* Data-parallel form of cirs_ppo_minibatch for a learner sharded over ranks.  A GLOBAL minibatch of mb_global rows
 * (idx_global) is split by rows; this rank owns idx_local[mb_local].  Advantage normalisation uses the statistics of
 * the global minibatch (every rank holds the gathered buffer) and every mean is over mb_global rows, so the SUM over
 * ranks of the gradients equals the single-device gradient of the global minibatch.
 *   phase 1: forward + backward -> grads[0 .. P) and the loss partials {clip, vf, ent, 0} in grads[P .. P+4)
 *            (P = cirs_ppo_param_count; the grads buffer must hold P+4 floats)
 *   -- caller all-reduces (sum) grads[0 .. P+4) over the ranks (RCCL) --
 *   phase 2: clip_grad_norm_ + Adam from the reduced gradients, loss_out[4] from the reduced partials
 *   phase 0: both phases back to back (single rank). */
int cirs_ppo_minibatch_dp(const cirs_ppo_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                          int64_t opt_step, const cirs_ppo_batch* batch, const int32_t* idx_local, int32_t mb_local,
                          const int32_t* idx_global, int32_t mb_global, float* dobs_accum, int32_t n_env,
                          float* loss_out, void* workspace, int64_t workspace_bytes, int32_t phase, void* stream);

/* cirs_ppo_minibatch_dp for a CHAIN of data-parallel steps (one update's minibatches; no reference counterpart, same semantics and bits as
 * cirs_ppo_minibatch_dp step by step): the workspace is laid out for max_mb_local rows (the update's largest local minibatch), so that consecutive
 * steps of different size share it;
 *   phase 1, head_done != 0: the head of this step (trunk forward of its rows, advantage statistics of the global minibatch, Wa planes) already ran
 *            inside the previous step's phase 2 -- three launches (head statistics, head backward, trunk backward incl. every gradient sum and this
 *            rank's loss partials) instead of seven;
 *   phase 2, next_idx_local != NULL: the optimiser launch also runs the head of the next step on the weights it forms (rows next_idx_local
 *            [next_mb_local] of this rank, statistics over next_idx_global [next_mb_global]); the caller passes head_done = 1 to that step's phase 1. */
int cirs_ppo_minibatch_dp_chain(const cirs_ppo_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t opt_step,
                                const cirs_ppo_batch* batch, const int32_t* idx_local, int32_t mb_local, const int32_t* idx_global,
                                int32_t mb_global, float* dobs_accum, int32_t n_env, float* loss_out, void* workspace, int64_t workspace_bytes,
                                int32_t phase, int32_t max_mb_local, int32_t head_done, const int32_t* next_idx_local, int32_t next_mb_local,
                                const int32_t* next_idx_global, int32_t next_mb_global, void* stream);

/* Tensor-parallel form of cirs_ppo_minibatch for an ITEM-SHARDED actor head (BASELINE configs[4]: the catalogue does not fit / is not
 * replicated; SURVEY 8(e): "actor head column-sharded over items with a cross-rank (max, sum-exp, ...) reduction").  No reference
 * counterpart (the reference is single-process); semantics = cirs_ppo_minibatch on one device with the whole catalogue.
 * Rank r holds rows [item_base, item_base + cfg->n_items) of wa / ba -- cfg, params, grads and the Adam moments describe the SHARD
 * (flat layout as above with I = the shard's item count); trunk and critic are replicated, batch->act holds GLOBAL item ids and every
 * rank processes every row of the minibatch.  Per minibatch, two collectives:
 *   phase 1  trunk forward, statistics of the local items -> stats4 [4][n_pad] = {max, sum-exp, sum exp z, logit of the row's action
 *            if this shard owns it else NaN}                                            (n_pad = rows rounded up to 32)
 *   -- all-gather; the caller hands the result back as stats_all [4][world][n_pad] (field-major) --
 *   phase 2  merge in rank order (identical on every rank) -> row losses / coefficients; fused head backward on the local items:
 *            the shard's wa|ba gradient is COMPLETE (it saw every row); red = {d h2 partial [n_pad,64], entropy clamp partial
 *            [n_pad], this rank's squared-norm partials of the wa|ba gradient in its slots of [world, 176]} =
 *            cirs_ppo_tp_exchange_floats(mb, world) floats
 *   -- all-reduce (sum) of red --
 *   phase 3  trunk / critic backward (replicated, identical inputs), clip_grad_norm_ over trunk x 2 + every shard's head + critic,
 *            Adam on the shard + the replicated trunk; loss_out[4]; dobs_accum as in cirs_ppo_minibatch. */
int64_t cirs_ppo_tp_exchange_floats(int32_t n_rows, int32_t world);
int cirs_ppo_minibatch_tp(const cirs_ppo_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t opt_step,
                          const cirs_ppo_batch* batch, const int32_t* idx, int32_t mb, int32_t item_base, int32_t rank,
                          int32_t world, float* stats4, const float* stats_all, float* red, float* dobs_accum, int32_t n_env,
                          float* loss_out, void* workspace, int64_t workspace_bytes, int32_t phase, void* stream);

/* Sharded optimiser step of the data-parallel learner (the reduce-scatter -> sharded Adam -> all-gather form of the step above):
 * after phase 1 the caller reduce-scatters grads[0 .. P_pad) (P_pad = P + 4 rounded up to a multiple of 4 * world; the padding
 * stays zero) so that this rank holds the summed shard [shard_begin, shard_begin + shard_len) of the flat gradient.
 *   cirs_ppo_shard_norm   stats_out[cirs_ppo_shard_stat_floats()] = fixed-order partial sums of squares of the shard (trunk elements
 *                         counted twice) + the loss partials of the gradient tail where the shard holds them
 *   -- caller all-gathers the stats of all ranks: stats_all [world, cirs_ppo_shard_stat_floats()] --
 *   cirs_ppo_shard_adam   clip_grad_norm_ coefficient from stats_all (summed in rank order: identical on every rank), Adam on the
 *                         shard only (params / moments pointers are those OF THE SHARD), loss_out[4] (nullable)
 *   -- caller all-gathers the parameter shards --
 * No reference counterpart (the reference is single-process); semantics = cirs_ppo_minibatch_dp phase 2. */
int32_t cirs_ppo_shard_stat_floats(void);
int cirs_ppo_shard_norm(const cirs_ppo_cfg* cfg, const float* grads_shard, int64_t shard_begin, int64_t shard_len,
                        float* stats_out, void* stream);
int cirs_ppo_shard_adam(const cirs_ppo_cfg* cfg, float* params_shard, const float* grads_shard, float* adam_m_shard,
                        float* adam_v_shard, int64_t shard_begin, int64_t shard_len, int64_t opt_step, const float* stats_all,
                        int32_t world, float* loss_out, void* stream);

/* torch.optim.Adam single-tensor update over a flat buffer, `n_sub` sequential sub-steps with the same gradient
 * starting at step `step_before`+1; grad is multiplied by (*grad_scale)^scale_pow when grad_scale != NULL. */
int cirs_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, int64_t step_before,
                   int32_t n_sub, float lr, float beta1, float beta2, float eps, const float* grad_scale,
                   int32_t scale_pow, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State-tracker backward: the gradient PPO sends into the tracker through the stored obs
 * replaces  the retained autograd graph of core/collector.py:261-269 + core/policy/ppo.py:174,215,235
 *           (loss.backward(retain_graph=True) accumulating into state_tracker.parameters(), one optim_state.step()).
 * Because the mask is causal and dropout is off, the per-step recomputations of the reference are one causal
 * transformer pass over each episode; rows are the buffer rows (env b, position p = t), p < len_b.  The forward is
 * recomputed from the stored slots (x_hist) and back-propagated analytically down to the embedding tables.
 * Every reduction over rows (weight gradients and the embedding-table scatter) has a fixed order: no float atomics,
 * so replicated learners on different ranks produce identical bits.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct cirs_tracker_layer_grads {
    float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *lin1_w, *lin1_b, *lin2_w, *lin2_b;
    float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} cirs_tracker_layer_grads;

typedef struct cirs_tracker_grads { /* same tensors as cirs_tracker_weights (pe is a buffer: no gradient) */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float* pe_unused;
    cirs_tracker_layer_grads layer[CIRS_MAX_TRACKER_LAYERS];
    float *dec_w, *dec_b;
} cirs_tracker_grads;

int64_t cirs_tracker_backward_workspace_bytes(const cirs_tracker_cfg* cfg, int32_t n_rows);

/* users[B]; act/rew are the time-major trajectory rows [T,B]; row_env/row_t/offsets/lens describe the buffer rows
 * (see cirs_ppo_prepare); dstate [T+1,B,S] = d loss / d obs.  Every gradient tensor is OVERWRITTEN. */
int cirs_tracker_backward(const cirs_tracker_cfg* cfg, const cirs_tracker_weights* w, const cirs_tracker_state* st,
                          const int32_t* users, const int64_t* act, const double* rew, const int32_t* row_env,
                          const int32_t* row_t, const int32_t* offsets, const int32_t* lens, int32_t n_rows,
                          const float* dstate, const cirs_tracker_grads* grads, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* cirs_tracker_backward for an upstream gradient that sits on the LAST row of every env only: dstate_last [n_env, S] = d loss / d state(env b, position
 * lens[b] - 1) (envs with lens[b] == 0 are ignored); same gradients as cirs_tracker_backward with a dstate that is zero everywhere else.
 * replaces  the backward of ONE build_state call under live dropout: the policy only receives s_t = the decoder of the last position of the prefix
 *           (core/state_tracker.py:243-246 `s_t = ...[:, -1, :]` behind the re-run encoder of :170-186), so in that call's graph the top encoder layer is
 *           needed at one row per env: its attention has one query, its row chain, five of its six weight-gradient problems and the decoder's run on
 *           n_env rows instead of n_rows; every layer below is the ordinary pass.  The exact-redraw learner (cirs_hip/redraw.py) runs all calls of a
 *           buffer as ONE such pass over pseudo-envs (call c, env e).
 * Workspace: cirs_tracker_backward_workspace_bytes(cfg, max(n_rows, cfg->n_env)).  Falls back to the general pass (same results, no saving) for a
 * one-layer tracker or max_len > 64. */
int cirs_tracker_backward_last(const cirs_tracker_cfg* cfg, const cirs_tracker_weights* w, const cirs_tracker_state* st,
                               const int32_t* users, const int64_t* act, const double* rew, const int32_t* row_env,
                               const int32_t* row_t, const int32_t* offsets, const int32_t* lens, int32_t n_rows,
                               const float* dstate_last, const cirs_tracker_grads* grads, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* Exact-redraw dropout inside the fused rollout (core/state_tracker.py:170-186,243-246: the reference never switches the tracker to eval(), so every
 * build_state call re-runs the encoder over the WHOLE prefix with fresh masks).  cirs_rollout_steps_redraw = cirs_rollout_steps in which the state of
 * vector step t comes from cirs_tracker_prefix_states over positions 0 .. t of every env under the masks of call t (pseudo-env ids env_base0 +
 * t * env_stride + e of the key dropout_seed), instead of from the cached decode.  Row lists of all calls, concatenated: call c describes n_env * (c + 1)
 * rows (env-major) starting at n_env * c * (c + 1) / 2 of row_env / row_t, and row c of offsets / lens [max_turn + 1][n_env].
 * workspace: cirs_tracker_backward_workspace_bytes(cfg, n_env * (max_turn + 1)). */
typedef struct {
    const int32_t* row_env;
    const int32_t* row_t;
    const int32_t* offsets;
    const int32_t* lens;
    uint64_t dropout_seed;
    int64_t env_base0, env_stride;
    void* workspace;
    int64_t workspace_bytes;
} cirs_redraw;
int cirs_rollout_steps_redraw(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                              const cirs_tracker_cfg* trk_cfg, const cirs_tracker_weights* trk_w, cirs_tracker_state* trk_st,
                              const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                              int32_t t_begin, int32_t t_end, uint64_t seed, uint32_t rng_base, const cirs_redraw* redraw,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* The forward half of cirs_tracker_backward as an entry point: ONE causal pass over the buffer rows (env b, positions 0 .. lens[b]-1) from the
 * stored input slots, with the dropout masks of the key currently set in cfg (dropout_seed / drop_env_base), and the state of every env's LAST row
 * -> state_out[b * state_stride + 0 .. dim_state) (envs with lens[b] == 0 are left untouched).  This is the reference's build_state under live
 * dropout -- the encoder re-run over the WHOLE prefix with fresh masks at every call (core/state_tracker.py:170-186, 243-246) -- as one batched
 * pass per call instead of a replay of the cached decode (cirs_hip/redraw.py).  Workspace: cirs_tracker_backward_workspace_bytes(cfg, n_rows). */
int cirs_tracker_prefix_states(const cirs_tracker_cfg* cfg, const cirs_tracker_weights* w, const cirs_tracker_state* st,
                               const int32_t* row_env, const int32_t* row_t, const int32_t* offsets, const int32_t* lens,
                               int32_t n_rows, float* state_out, int64_t state_stride, void* workspace, int64_t workspace_bytes,
                               void* stream);

/* Ordered scatter of embedding-gradient rows (dim_model == 32) into a table: grad_table [n_table_rows, 32] is OVERWRITTEN with, per row k,
 * the sum of contrib[r] over the rows r with keys[r] == k, added in ascending r (stable radix sort + ordered segment sums: no float
 * atomics, cost O(n_rows) whatever the table size); keys outside [0, n_table_rows) contribute nothing.  It is the scatter of
 * cirs_tracker_backward's embedding gradients as an entry point of its own: the OWNER side of row-sharded tables (BASELINE configs[4],
 * "tables row-sharded by id mod W") after the all-to-all of (row id, gradient row) pairs.  No reference counterpart. */
int64_t cirs_embedding_scatter_workspace_bytes(int64_t n_rows);
int cirs_embedding_scatter(const int32_t* keys, const float* contrib, int64_t n_rows, int32_t n_table_rows, float* grad_table,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, recurrent: StateTrackerGRU (csrc/gru_tracker.hip)
 * The reference declares the class and leaves it empty (core/state_tracker.py:282-289); the model is defined here:
 *   inputs  the Transformer tracker's slots, unchanged (state_tracker.py:205-215,225-242): slot 0 = ffn_user(Emb_user[u]),
 *           slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k; no sqrt(D) scale, no positional encoding
 *   cell    torch.nn.GRU(input_size = D, hidden_size = D, num_layers = nlayers), h_{-1} = 0, gate order r, z, n:
 *             r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
 *             n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h
 *           layer l > 0 reads layer l - 1's h' of the same position
 *   state   s_t = decoder(h_t of the top layer)
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, nlayers in {1, 2}.  No dropout (nn.GRU has it between layers only).
 * The existing tracker structs are not touched: a GRU tracker has its own.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_GRU_MAX_LAYERS 2

typedef struct cirs_gru_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t nlayers;   /* 1 or 2 */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
} cirs_gru_cfg;

typedef struct cirs_gru_layer { /* names: gru.weight_ih_l<k>, gru.weight_hh_l<k> [3D,D]; gru.bias_ih_l<k>, gru.bias_hh_l<k> [3D]; rows r | z | n */
    const float *w_ih, *w_hh, *b_ih, *b_hh;
} cirs_gru_layer;

typedef struct cirs_gru_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    cirs_gru_layer layer[CIRS_GRU_MAX_LAYERS];
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_gru_weights;

typedef struct cirs_gru_state {
    float* x_hist; /* [B, max_len, D] the input slots (what the backward recomputes from) */
    float* h;      /* [nlayers, B, D] the carried hidden state of every layer */
    int32_t* len;  /* [B] positions appended so far */
} cirs_gru_state;

typedef struct cirs_gru_layer_grads {
    float *w_ih, *w_hh, *b_ih, *b_hh;
} cirs_gru_layer_grads;

typedef struct cirs_gru_grads { /* same tensors, same order as cirs_gru_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    cirs_gru_layer_grads layer[CIRS_GRU_MAX_LAYERS];
    float *dec_w, *dec_b;
} cirs_gru_grads;

/* cirs_tracker_init / cirs_tracker_step for the GRU tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j (NULL: j);
 * init writes slot 0, h = cell(x_0, 0), len = 1; step appends one position.  Rows with skip != 0 (step) or item < 0 are left untouched: neither
 * the tracker state nor their row of state_out is written.  state_out row stride = state_stride floats. */
int cirs_gru_tracker_init(const cirs_gru_cfg* cfg, const cirs_gru_weights* w, cirs_gru_state* st, const int32_t* users,
                          const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_gru_tracker_step(const cirs_gru_cfg* cfg, const cirs_gru_weights* w, cirs_gru_state* st, const int64_t* items,
                          const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                          int64_t state_stride, void* stream);

/* cirs_tracker_backward for the GRU tracker: back-propagation through time, recomputed from the stored slots.  users[B]; act / rew are the
 * time-major trajectory rows [T,B]; row_env / row_t / offsets / lens describe the buffer rows (env-major, see cirs_ppo_prepare);
 * dstate [T+1,B,S] = d loss / d obs.  Every gradient tensor is OVERWRITTEN.  No float atomics; every reduction has a fixed order, so two
 * calls give the same bits.  A workspace smaller than cirs_gru_tracker_backward_workspace_bytes(cfg, n_rows) is refused before any launch. */
int64_t cirs_gru_tracker_backward_workspace_bytes(const cirs_gru_cfg* cfg, int32_t n_rows);
int cirs_gru_tracker_backward(const cirs_gru_cfg* cfg, const cirs_gru_weights* w, const cirs_gru_state* st, const int32_t* users,
                              const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                              const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                              const cirs_gru_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect with a GRU tracker: env reset, cirs_gru_tracker_init, then per vector step cirs_actor_sample (greedy != 0:
 * cirs_actor_greedy), the visited bits, cirs_env_step, the forced length and cirs_gru_tracker_step -- the unfused launch sequence of
 * cirs_rollout_steps_online without its scorer, on the caller's stream, no host synchronisation.  Same trajectory contract: every entry
 * [t][env] is written (envs that finished earlier: act -1, done 1, rew / ctr 0).  gumbel (nullable; not with greedy): harness-supplied
 * sampler noise [max_turn][n_env][n_items] as in cirs_rollout_steps_noise.  workspace >= cirs_policy_workspace_bytes(pol_cfg, n_env). */
int cirs_rollout_collect_gru(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                             const cirs_gru_cfg* trk_cfg, const cirs_gru_weights* trk_w, cirs_gru_state* trk_st,
                             const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                             int32_t n_env, const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited,
                             int32_t force_length, int32_t greedy, const float* gumbel, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, recurrent: StateTrackerLSTM (csrc/lstm_tracker.hip)
 * The reference declares the class and leaves it empty (core/state_tracker.py:282-289); the model is defined here:
 *   inputs  the GRU tracker's slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k;
 *           no sqrt(D) scale, no positional encoding
 *   cell    torch.nn.LSTM(input_size = D, hidden_size = D, num_layers = nlayers), h_{-1} = c_{-1} = 0, gate order i, f, g, o:
 *             i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)   f = sigmoid(W_if x + b_if + W_hf h + b_hf)
 *             g = tanh(W_ig x + b_ig + W_hg h + b_hg)      o = sigmoid(W_io x + b_io + W_ho h + b_ho)
 *             c' = f * c + i * g                           h' = o * tanh(c')
 *           layer l > 0 reads layer l - 1's h' of the same position; no proj_size, not bidirectional
 *   state   s_t = decoder(h_t of the top layer)
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, nlayers in {1, 2}.  No dropout (nn.LSTM has it between layers only).
 * The existing tracker structs are not touched: an LSTM tracker has its own.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_LSTM_MAX_LAYERS 2

typedef struct cirs_lstm_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t nlayers;   /* 1 or 2 */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
} cirs_lstm_cfg;

typedef struct cirs_lstm_layer { /* names: lstm.weight_ih_l<k>, lstm.weight_hh_l<k> [4D,D]; lstm.bias_ih_l<k>, lstm.bias_hh_l<k> [4D]; rows i | f | g | o */
    const float *w_ih, *w_hh, *b_ih, *b_hh;
} cirs_lstm_layer;

typedef struct cirs_lstm_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    cirs_lstm_layer layer[CIRS_LSTM_MAX_LAYERS];
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_lstm_weights;

typedef struct cirs_lstm_state {
    float* x_hist; /* [B, max_len, D] the input slots (what the backward recomputes from) */
    float* h;      /* [nlayers, B, D] the carried hidden state of every layer */
    float* c;      /* [nlayers, B, D] the carried cell state of every layer */
    int32_t* len;  /* [B] positions appended so far */
} cirs_lstm_state;

typedef struct cirs_lstm_layer_grads { /* b_ih and b_hh receive the same gradient; both are written */
    float *w_ih, *w_hh, *b_ih, *b_hh;
} cirs_lstm_layer_grads;

typedef struct cirs_lstm_grads { /* same tensors, same order as cirs_lstm_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    cirs_lstm_layer_grads layer[CIRS_LSTM_MAX_LAYERS];
    float *dec_w, *dec_b;
} cirs_lstm_grads;

/* cirs_gru_tracker_init / cirs_gru_tracker_step for the LSTM tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j
 * (NULL: j); init writes slot 0, (h, c) = cell(x_0, 0, 0), len = 1; step appends one position.  Rows with skip != 0 (step), an env / user /
 * item id out of range (item < 0: the env finished), a never-initialised or a full history are left untouched: neither h, c, len nor their
 * row of state_out is written.  state_out row stride = state_stride floats. */
int cirs_lstm_tracker_init(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w, cirs_lstm_state* st, const int32_t* users,
                           const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_lstm_tracker_step(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w, cirs_lstm_state* st, const int64_t* items,
                           const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                           int64_t state_stride, void* stream);

/* cirs_gru_tracker_backward for the LSTM tracker: back-propagation through time through h and c, recomputed from the stored slots.  Same
 * arguments: users[B]; act / rew are the time-major trajectory rows [T,B]; row_env / row_t / offsets / lens describe the buffer rows
 * (env-major, see cirs_ppo_prepare); dstate [T+1,B,S] = d loss / d obs.  Every gradient tensor is OVERWRITTEN.  No float atomics; every
 * reduction has a fixed order, so two calls give the same bits.  A workspace smaller than
 * cirs_lstm_tracker_backward_workspace_bytes(cfg, n_rows), or one not 16-byte aligned, is refused before any launch. */
int64_t cirs_lstm_tracker_backward_workspace_bytes(const cirs_lstm_cfg* cfg, int32_t n_rows);
int cirs_lstm_tracker_backward(const cirs_lstm_cfg* cfg, const cirs_lstm_weights* w, const cirs_lstm_state* st, const int32_t* users,
                               const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                               const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                               const cirs_lstm_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect_gru with an LSTM tracker: the same launch sequence (one loop serves both, csrc/rollout.hip) with
 * cirs_lstm_tracker_init / cirs_lstm_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_lstm(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                              const cirs_lstm_cfg* trk_cfg, const cirs_lstm_weights* trk_w, cirs_lstm_state* trk_st,
                              const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                              int32_t n_env, const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited,
                              int32_t force_length, int32_t greedy, const float* gumbel, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, pooled window: StateTrackerAvg (csrc/avg_tracker.hip)
 * The reference has no counterpart; the model is defined here:
 *   inputs  the recurrent trackers' slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k;
 *           no sqrt(D) scale, no positional encoding
 *   pooling n_p = min(window, p);  m_0 = 0,  m_p = (x_{p-n_p+1} + ... + x_p) / n_p  -- fp32, summed in ascending k starting from
 *           x_{p-n_p+1}, then one division by float(n_p);  h_p = x_0 + m_p.  The sum is formed anew from the stored slots at every
 *           step (no running sum): position p depends on its window only.  A window beyond the history is the mean of all of it.
 *   state   s_p = decoder(h_p)
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, window >= 1, max_len <= 4096.  No new parameters, no dropout site.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct cirs_avg_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t window;    /* W >= 1: item slots in the mean */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
} cirs_avg_cfg;

typedef struct cirs_avg_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_avg_weights;

typedef struct cirs_avg_state {
    float* x_hist; /* [B, max_len, D] the input slots: the window of every step and the backward read them */
    int32_t* len;  /* [B] positions appended so far */
} cirs_avg_state;

typedef struct cirs_avg_grads { /* same tensors, same order as cirs_avg_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float *dec_w, *dec_b;
} cirs_avg_grads;

/* cirs_lstm_tracker_init / cirs_lstm_tracker_step for the Avg tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j
 * (NULL: j); init writes slot 0, len = 1; step appends one position.  Rows with skip != 0 (step), an env / user / item id out of range
 * (item < 0: the env finished), a never-initialised or a full history are left untouched: neither x_hist, len nor their row of state_out
 * is written.  state_out row stride = state_stride floats.  window < 1 is refused (CIRS_E_INVALID). */
int cirs_avg_tracker_init(const cirs_avg_cfg* cfg, const cirs_avg_weights* w, cirs_avg_state* st, const int32_t* users,
                          const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_avg_tracker_step(const cirs_avg_cfg* cfg, const cirs_avg_weights* w, cirs_avg_state* st, const int64_t* items,
                          const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                          int64_t state_stride, void* stream);

/* cirs_gru_tracker_backward for the Avg tracker.  The pooling is linear: with dH[b,p] = sum_s dstate[p,b,s] W_dec[s,:],
 *   dX[b,0] = sum_{p=0}^{len_b-1} dH[b,p]      dX[b,k] = sum_{p=k}^{min(len_b-1, k+window-1)} dH[b,p] / float(n_p)   (k >= 1; p ascending)
 * then the slot stage of the recurrent trackers.  Same arguments: users[B]; act / rew are the time-major trajectory rows [T,B];
 * row_env / row_t / offsets / lens describe the buffer rows (env-major, see cirs_ppo_prepare); dstate [T+1,B,S] = d loss / d obs; of st
 * only x_hist is read.  Every gradient tensor is OVERWRITTEN.  No float atomics; every reduction has a fixed order, so two calls give
 * the same bits.  A workspace smaller than cirs_avg_tracker_backward_workspace_bytes(cfg, n_rows), or one not 16-byte aligned, is
 * refused before any launch. */
int64_t cirs_avg_tracker_backward_workspace_bytes(const cirs_avg_cfg* cfg, int32_t n_rows);
int cirs_avg_tracker_backward(const cirs_avg_cfg* cfg, const cirs_avg_weights* w, const cirs_avg_state* st, const int32_t* users,
                              const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                              const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                              const cirs_avg_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect_gru with an Avg tracker: the same launch sequence (one loop serves the three, csrc/rollout.hip) with
 * cirs_avg_tracker_init / cirs_avg_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_avg(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                             const cirs_avg_cfg* trk_cfg, const cirs_avg_weights* trk_w, cirs_avg_state* trk_st,
                             const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                             int32_t n_env, const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited,
                             int32_t force_length, int32_t greedy, const float* gumbel, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, convolutional window: StateTrackerCaser (csrc/caser_tracker.hip)
 * The reference has no counterpart; the model is defined here (Caser: horizontal filters max-pooled over time plus one vertical filter
 * over the window of the last W item slots, treated as a [W, D] image):
 *   inputs  the other trackers' slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k;
 *           no sqrt(D) scale, no positional encoding
 *   window  win_p[j] = x_{p-W+1+j} if p-W+1+j >= 1, else the zero row    (j = 0..W-1: the last W ITEM slots, zero rows in front; x_0 is
 *           never in it; position 0 has an all-zero window and no special case)
 *   banks   c_{i,f,t} = bh_i[f] + sum_{j<h_i} sum_d Wh_i[f,j,d] win_p[t+j,d]   (t = 0..W-h_i; fp32, one chain from the bias, j then d ascending)
 *           o_{i,f}   = relu(max_t c_{i,f,t})     zero rows take part in the convolution and in the max; arg-max = the FIRST maximal t
 *   vertical v_d = relu(bv + sum_j wv[j] win_p[j,d])
 *   fc      z = relu(fc([o_0 | o_1 | ... | v]))    fc: [D, 16 n_heights + D]
 *   state   h_p = x_0 + z;  s_p = decoder(h_p)
 * The window is read anew from the stored slots at every step: position p depends on its window and x_0 only.
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, 16 filters per bank, heights a non-empty strictly ascending subset of
 * {1, 2, 3, 4}, max(heights) <= window <= 16, max_len <= 4096.  No dropout site.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_CASER_MAX_HEIGHTS 4
#define CIRS_CASER_FILTERS 16
#define CIRS_CASER_MAX_WINDOW 16

typedef struct cirs_caser_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t window;    /* W: item slots in the window, max(heights) <= W <= 16 */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
    int32_t n_heights; /* horizontal banks, 1..4 */
    int32_t heights[CIRS_CASER_MAX_HEIGHTS]; /* h_i, strictly ascending, each in 1..4; entries >= n_heights are ignored */
} cirs_caser_cfg;

typedef struct cirs_caser_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    const float* conv_w[CIRS_CASER_MAX_HEIGHTS]; /* horizontal_cnn.<i>.weight [16,1,h_i,D] */
    const float* conv_b[CIRS_CASER_MAX_HEIGHTS]; /* horizontal_cnn.<i>.bias [16] */
    const float *vert_w, *vert_b;         /* vertical_cnn.weight [1,1,W,1], vertical_cnn.bias [1] */
    const float *fc_w, *fc_b;             /* fc [D, 16 n_heights + D] (input order o_0 | o_1 | ... | v), [D] */
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_caser_weights;

typedef struct cirs_caser_state {
    float* x_hist; /* [B, max_len, D] the input slots: the window of every step and the backward read them */
    int32_t* len;  /* [B] positions appended so far */
} cirs_caser_state;

typedef struct cirs_caser_grads { /* same tensors, same order as cirs_caser_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float* conv_w[CIRS_CASER_MAX_HEIGHTS];
    float* conv_b[CIRS_CASER_MAX_HEIGHTS];
    float *vert_w, *vert_b, *fc_w, *fc_b;
    float *dec_w, *dec_b;
} cirs_caser_grads;

/* cirs_avg_tracker_init / cirs_avg_tracker_step for the Caser tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j
 * (NULL: j); init writes slot 0, len = 1; step appends one position.  Rows with skip != 0 (step), an env / user / item id out of range
 * (item < 0: the env finished), a never-initialised or a full history are left untouched: neither x_hist, len nor their row of state_out
 * is written.  state_out row stride = state_stride floats.  A cfg outside the fixed sizes is refused (CIRS_E_INVALID / CIRS_E_UNSUPPORTED)
 * with a message that names the member, before any pointer is read. */
int cirs_caser_tracker_init(const cirs_caser_cfg* cfg, const cirs_caser_weights* w, cirs_caser_state* st, const int32_t* users,
                            const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_caser_tracker_step(const cirs_caser_cfg* cfg, const cirs_caser_weights* w, cirs_caser_state* st, const int64_t* items,
                            const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                            int64_t state_stride, void* stream);

/* cirs_avg_tracker_backward for the Caser tracker.  No sequential pass: the forward of every buffer row is recomputed from the stored slots
 * (the pooling's arg-max included), the decoder stage is the other trackers', then fc, both ReLUs, the vertical filter and the max-pool give
 * a window gradient per row, which is folded into dX[b,k] in ascending p (dX[b,0] = sum_p dH[b,p]); then the slot stage of the recurrent
 * trackers.  Same arguments: users[B]; act / rew are the time-major trajectory rows [T,B]; row_env / row_t / offsets / lens describe the
 * buffer rows (env-major, see cirs_ppo_prepare); dstate [T+1,B,S] = d loss / d obs; of st only x_hist is read.  Every gradient tensor is
 * OVERWRITTEN.  No float atomics; every reduction has a fixed order, so two calls give the same bits.  A workspace smaller than
 * cirs_caser_tracker_backward_workspace_bytes(cfg, n_rows), or one not 16-byte aligned, is refused before any launch. */
int64_t cirs_caser_tracker_backward_workspace_bytes(const cirs_caser_cfg* cfg, int32_t n_rows);
int cirs_caser_tracker_backward(const cirs_caser_cfg* cfg, const cirs_caser_weights* w, const cirs_caser_state* st, const int32_t* users,
                                const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                                const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                                const cirs_caser_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect_gru with a Caser tracker: the same launch sequence (one loop serves the four, csrc/rollout.hip) with
 * cirs_caser_tracker_init / cirs_caser_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_caser(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                               const cirs_caser_cfg* trk_cfg, const cirs_caser_weights* trk_w, cirs_caser_state* trk_st,
                               const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj,
                               int32_t n_env, const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited,
                               int32_t force_length, int32_t greedy, const float* gumbel, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, dilated causal convolutions: StateTrackerNextItNet (csrc/nextitnet_tracker.hip)
 * The reference has no counterpart; the model is defined here (NextItNet: a stack of residual blocks of dilated causal 1-D convolutions
 * of width 3 over the item slots; no max-pool, nothing carried):
 *   inputs  the other trackers' slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k;
 *           no sqrt(D) scale, no positional encoding
 *   blocks  y^{-1}_t = x_t  (t >= 1: item slots only; x_0 is never convolved)
 *           c^l_t = b_l + sum_{j=0..2} W_l[:,:,j] y^{l-1}_{t-(2-j) d_l}     with y^{l-1}_s = 0 for s < 1: zero padding at EVERY layer's
 *                   input, not values computed from padding  (fp32; taps j ascending, channels ascending inside a tap)
 *           n^l_t = LayerNorm_l(c^l_t) over the 32 channels  (eps 1e-5, biased variance: the mean, then the variance of the centred values)
 *           y^l_t = y^{l-1}_t + relu(n^l_t)
 *   state   h_p = x_0 + y^{n-1}_p (p >= 1), h_0 = x_0;  s_p = decoder(h_p)
 * Only the last R = 1 + 2 sum_l d_l item slots reach position p; they are read anew from the stored slots at every step: position p depends
 * on them and on x_0 only.
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, kernel width 3, 1 <= n_blocks <= 4, every dilation in 1..4 (any order),
 * sum of the dilations <= 7 (R <= 15: one 16-row tile), max_len <= 4096.  No dropout site.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_NEXTITNET_MAX_BLOCKS 4
#define CIRS_NEXTITNET_MAX_DILATION 4
#define CIRS_NEXTITNET_MAX_DILATION_SUM 7

typedef struct cirs_nextitnet_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t n_blocks;  /* residual blocks, 1..4 */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
    int32_t dilations[CIRS_NEXTITNET_MAX_BLOCKS]; /* d_l, each in 1..4, sum <= 7; entries >= n_blocks are ignored */
} cirs_nextitnet_cfg;

typedef struct cirs_nextitnet_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    const float* conv_w[CIRS_NEXTITNET_MAX_BLOCKS]; /* blocks.<l>.conv.weight [D,D,3] (out, in, tap) */
    const float* conv_b[CIRS_NEXTITNET_MAX_BLOCKS]; /* blocks.<l>.conv.bias [D] */
    const float* ln_w[CIRS_NEXTITNET_MAX_BLOCKS];   /* blocks.<l>.ln.weight [D] */
    const float* ln_b[CIRS_NEXTITNET_MAX_BLOCKS];   /* blocks.<l>.ln.bias [D] */
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_nextitnet_weights;

typedef struct cirs_nextitnet_state {
    float* x_hist; /* [B, max_len, D] the input slots: the blocks of every step and the backward read them */
    int32_t* len;  /* [B] positions appended so far */
} cirs_nextitnet_state;

typedef struct cirs_nextitnet_grads { /* same tensors, same order as cirs_nextitnet_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float* conv_w[CIRS_NEXTITNET_MAX_BLOCKS];
    float* conv_b[CIRS_NEXTITNET_MAX_BLOCKS];
    float* ln_w[CIRS_NEXTITNET_MAX_BLOCKS];
    float* ln_b[CIRS_NEXTITNET_MAX_BLOCKS];
    float *dec_w, *dec_b;
} cirs_nextitnet_grads;

/* cirs_avg_tracker_init / cirs_avg_tracker_step for the NextItNet tracker, same argument conventions: env_ids (nullable, [n]) = the env of
 * row j (NULL: j); init writes slot 0, len = 1; step appends one position.  Rows with skip != 0 (step), an env / user / item id out of range
 * (item < 0: the env finished), a never-initialised or a full history are left untouched: neither x_hist, len nor their row of state_out
 * is written.  state_out row stride = state_stride floats.  A cfg outside the fixed sizes is refused (CIRS_E_INVALID / CIRS_E_UNSUPPORTED)
 * with a message that names the member, before any pointer is read. */
int cirs_nextitnet_tracker_init(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w, cirs_nextitnet_state* st,
                                const int32_t* users, const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride,
                                void* stream);
int cirs_nextitnet_tracker_step(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w, cirs_nextitnet_state* st,
                                const int64_t* items, const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n,
                                float* state_out, int64_t state_stride, void* stream);

/* cirs_avg_tracker_backward for the NextItNet tracker.  No sequential pass: the forward of every buffer row is recomputed from the stored
 * slots (every block's input, normalised values and inverse standard deviation are kept), the decoder stage is the other trackers', then per
 * row the blocks from the top down (ReLU, LayerNorm, the three taps transposed, the residual path) give a gradient per window slot, which is
 * folded into dX[b,k] in ascending p (dX[b,0] = sum_p dH[b,p]); then the slot stage of the recurrent trackers.  Same arguments: users[B];
 * act / rew are the time-major trajectory rows [T,B]; row_env / row_t / offsets / lens describe the buffer rows (env-major, see
 * cirs_ppo_prepare); dstate [T+1,B,S] = d loss / d obs; of st only x_hist is read.  Every gradient tensor is OVERWRITTEN.  No float atomics;
 * every reduction has a fixed order, so two calls give the same bits.  A workspace smaller than
 * cirs_nextitnet_tracker_backward_workspace_bytes(cfg, n_rows), or one not 16-byte aligned, is refused before any launch. */
int64_t cirs_nextitnet_tracker_backward_workspace_bytes(const cirs_nextitnet_cfg* cfg, int32_t n_rows);
int cirs_nextitnet_tracker_backward(const cirs_nextitnet_cfg* cfg, const cirs_nextitnet_weights* w, const cirs_nextitnet_state* st,
                                    const int32_t* users, const int64_t* act, const double* rew, const int32_t* row_env,
                                    const int32_t* row_t, const int32_t* offsets, const int32_t* lens, int32_t n_rows,
                                    const float* dstate, const cirs_nextitnet_grads* grads, void* workspace, int64_t workspace_bytes,
                                    void* stream);

/* cirs_rollout_collect_gru with a NextItNet tracker: the same launch sequence (one loop serves the five, csrc/rollout.hip) with
 * cirs_nextitnet_tracker_init / cirs_nextitnet_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_nextitnet(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                                   const cirs_nextitnet_cfg* trk_cfg, const cirs_nextitnet_weights* trk_w,
                                   cirs_nextitnet_state* trk_st, const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w,
                                   const cirs_traj* traj, int32_t n_env, const int32_t* users, uint64_t seed, uint32_t rng_base,
                                   uint32_t* visited, int32_t force_length, int32_t greedy, const float* gumbel, void* workspace,
                                   int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, attention pool over the window: StateTrackerSTAMP (csrc/stamp_tracker.hip)
 * The reference has no counterpart; the model is defined here (STAMP, Liu et al., KDD 2018: a general-interest query, a last-click query, a
 * small gate network without softmax, a multiplicative read-out; nothing carried):
 *   inputs     the other trackers' slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k;
 *              no sqrt(D) scale, no positional encoding
 *   window     n_p = min(window, p), the slots k = p - n_p + 1 .. p  (p >= 1)
 *              m_s = (x_{p-n_p+1} + ... + x_p) / n_p   (fp32, k ascending, then ONE division by float(n_p): the Avg tracker's m_p, same bits)
 *              m_t = x_p
 *   attention  c   = W2 m_t + W3 m_s + b_a
 *              e_k = w0 . sigmoid(W1 x_k + c)          (a scalar per window slot; no softmax)
 *              m_a = sum_k e_k x_k                     (k ascending)
 *   read-out   h_s = tanh(A m_a + b_A),  h_t = tanh(B m_t + b_B);  h_p = x_0 + h_s * h_t,  h_0 = x_0;  s_p = decoder(h_p)
 * The window is read anew from the stored slots at every step: position p depends on it and on x_0 only; a slot older than the window
 * does not reach it.
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, 1 <= window <= 16 (one 16-row tile), max_len <= 4096.  No dropout site.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_STAMP_MAX_WINDOW 16

typedef struct cirs_stamp_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t window;    /* W in 1..16: item slots in the window */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
} cirs_stamp_cfg;

typedef struct cirs_stamp_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    const float* attn_b;                  /* attn.bias [D] (a module's own tensor: listed before its children's, as state_dict lists it) */
    const float *w1, *w2, *w3;            /* attn.w1.weight, attn.w2.weight, attn.w3.weight [D,D] */
    const float* w0;                      /* attn.w0.weight [1,D] */
    const float *mlp_a_w, *mlp_a_b;       /* mlp_a [D,D], [D] */
    const float *mlp_b_w, *mlp_b_b;       /* mlp_b [D,D], [D] */
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_stamp_weights;

typedef struct cirs_stamp_state {
    float* x_hist; /* [B, max_len, D] the input slots: the window of every step and the backward read them */
    int32_t* len;  /* [B] positions appended so far */
} cirs_stamp_state;

typedef struct cirs_stamp_grads { /* same tensors, same order as cirs_stamp_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float *attn_b, *w1, *w2, *w3, *w0, *mlp_a_w, *mlp_a_b, *mlp_b_w, *mlp_b_b;
    float *dec_w, *dec_b;
} cirs_stamp_grads;

/* cirs_avg_tracker_init / cirs_avg_tracker_step for the STAMP tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j
 * (NULL: j); init writes slot 0, len = 1; step appends one position.  Rows with skip != 0 (step), an env / user / item id out of range
 * (item < 0: the env finished), a never-initialised or a full history are left untouched: neither x_hist, len nor their row of state_out
 * is written.  state_out row stride = state_stride floats.  A cfg outside the fixed sizes (window outside 1..16 among them) is refused
 * (CIRS_E_INVALID / CIRS_E_UNSUPPORTED) with a message that names the member, before any pointer is read. */
int cirs_stamp_tracker_init(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w, cirs_stamp_state* st, const int32_t* users,
                            const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_stamp_tracker_step(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w, cirs_stamp_state* st, const int64_t* items,
                            const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                            int64_t state_stride, void* stream);

/* cirs_avg_tracker_backward for the STAMP tracker.  No sequential pass: the forward of every buffer row is recomputed from the stored slots
 * (the window tile, the sigmoids, e, m_s, m_a, h_s and h_t are kept), the decoder stage is the other trackers', then per row the product,
 * the two tanh, m_a (both factors), the sigmoid tile, W1 and c give a gradient per window slot, which is folded into dX[b,k] in ascending
 * p (dX[b,0] = sum_p dH[b,p]); then the slot stage of the recurrent trackers.  Same arguments: users[B]; act / rew are the time-major
 * trajectory rows [T,B]; row_env / row_t / offsets / lens describe the buffer rows (env-major, see cirs_ppo_prepare); dstate [T+1,B,S] =
 * d loss / d obs; of st only x_hist is read.  Every gradient tensor is OVERWRITTEN.  No float atomics; every reduction has a fixed order,
 * so two calls give the same bits.  A workspace smaller than cirs_stamp_tracker_backward_workspace_bytes(cfg, n_rows), or one not 16-byte
 * aligned, is refused before any launch. */
int64_t cirs_stamp_tracker_backward_workspace_bytes(const cirs_stamp_cfg* cfg, int32_t n_rows);
int cirs_stamp_tracker_backward(const cirs_stamp_cfg* cfg, const cirs_stamp_weights* w, const cirs_stamp_state* st, const int32_t* users,
                                const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                                const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                                const cirs_stamp_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect_gru with a STAMP tracker: the same launch sequence (one loop serves the six, csrc/rollout.hip) with
 * cirs_stamp_tracker_init / cirs_stamp_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_stamp(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                               const cirs_stamp_cfg* trk_cfg, const cirs_stamp_weights* trk_w, cirs_stamp_state* trk_st,
                               const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                               const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                               int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, a GRU encoder with attention over its hidden states: StateTrackerNARM (csrc/narm_tracker.hip)
 * The reference has no counterpart; the model is defined here (NARM, Li et al., CIKM 2017: the last hidden state as the global
 * encoder, an additive attention over every hidden state of the session as the local one, a bilinear read-out):
 *   inputs     the GRU tracker's slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k
 *   encoder    h_p = GRU cell(x_p, h_{p-1}), h_{-1} = 0: torch.nn.GRU(D, D, 1), gate order r, z, n, both bias vectors
 *   attention  for position p over j = 0 .. p (the whole session so far, position 0 and p itself included):
 *                q_j = A2 h_j,  a_p = A1 h_p
 *                alpha_{p,j} = v . sigmoid(a_p + q_j)          (a scalar; no softmax, as in the paper)
 *                c_p = sum_{j=0}^{p} alpha_{p,j} h_j
 *   read-out   m_p = Bw [h_p ; c_p]                            (Bw: D x 2D; global = h_p, local = c_p);  s_p = decoder(m_p)
 * A1, A2, v and Bw have no bias (the paper has none).  The attention spans the whole session: a step costs O(p) at position p.
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, ONE encoder layer (the cfg keeps the GRU tracker's `nlayers` member so
 * that the two cfgs have one layout; any value but 1 is refused), max_len <= 4096.  The paper's two dropout sites are not built.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_NARM_MAX_LAYERS 1

typedef struct cirs_narm_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t nlayers;   /* 1 */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
} cirs_narm_cfg;

typedef struct cirs_narm_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    const float *w_ih, *w_hh, *b_ih, *b_hh; /* gru.weight_ih_l0, gru.weight_hh_l0 [3D,D]; gru.bias_ih_l0, gru.bias_hh_l0 [3D]; rows r | z | n */
    const float *a1, *a2;                 /* attn.a1.weight, attn.a2.weight [D,D] */
    const float* v;                       /* attn.v.weight [1,D] */
    const float* bw;                      /* bilinear.weight [D,2D]: columns [0,D) read h_p, [D,2D) read c_p */
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_narm_weights;

typedef struct cirs_narm_state {
    float* x_hist; /* [B, max_len, D] the input slots (what the backward recomputes from) */
    float* h;      /* [1, B, D] the carried hidden state */
    float* h_hist; /* [B, max_len, D] h_j of every position appended so far */
    float* q_hist; /* [B, max_len, D] q_j = A2 h_j: A2 is applied once per position, not once per pair */
    int32_t* len;  /* [B] positions appended so far */
} cirs_narm_state;

typedef struct cirs_narm_grads { /* same tensors, same order as cirs_narm_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float *w_ih, *w_hh, *b_ih, *b_hh, *a1, *a2, *v, *bw;
    float *dec_w, *dec_b;
} cirs_narm_grads;

/* cirs_gru_tracker_init / cirs_gru_tracker_step for the NARM tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j
 * (NULL: j); init writes slot 0, h_0, q_0, len = 1; step appends one position.  Rows with skip != 0 (step), an env / user / item id out of
 * range (item < 0: the env finished), a never-initialised or a full history are left untouched: neither the tracker state nor their row of
 * state_out is written.  state_out row stride = state_stride floats.  A cfg outside the fixed sizes is refused (CIRS_E_INVALID /
 * CIRS_E_UNSUPPORTED) with a message prefixed "narm tracker:", before any pointer is read. */
int cirs_narm_tracker_init(const cirs_narm_cfg* cfg, const cirs_narm_weights* w, cirs_narm_state* st, const int32_t* users,
                           const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_narm_tracker_step(const cirs_narm_cfg* cfg, const cirs_narm_weights* w, cirs_narm_state* st, const int64_t* items,
                           const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                           int64_t state_stride, void* stream);

/* cirs_gru_tracker_backward for the NARM tracker: the encoder is recomputed from the stored slots by the GRU tracker's sequential
 * kernels, the attention per buffer row (nothing per (p, j) pair is stored: the workspace is O(n_rows)); its backward runs once by query
 * row and once by key row, both parallel over the rows, and feeds dH into the GRU's sequential back-propagation through time.  Same
 * arguments as cirs_gru_tracker_backward; of st only x_hist is read.  Every gradient tensor is OVERWRITTEN.  No float atomics; every
 * reduction has a fixed order, so two calls give the same bits.  A workspace smaller than
 * cirs_narm_tracker_backward_workspace_bytes(cfg, n_rows) (0 for a cfg that is refused), or one not 16-byte aligned, is refused before any
 * launch. */
int64_t cirs_narm_tracker_backward_workspace_bytes(const cirs_narm_cfg* cfg, int32_t n_rows);
int cirs_narm_tracker_backward(const cirs_narm_cfg* cfg, const cirs_narm_weights* w, const cirs_narm_state* st, const int32_t* users,
                               const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                               const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                               const cirs_narm_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect_gru with a NARM tracker: the same launch sequence (one loop serves the seven, csrc/rollout.hip) with
 * cirs_narm_tracker_init / cirs_narm_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_narm(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                              const cirs_narm_cfg* trk_cfg, const cirs_narm_weights* trk_w, cirs_narm_state* trk_st,
                              const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                              const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                              int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, a learnable frequency-domain filter and an MLP: StateTrackerFMLP (csrc/fmlp_tracker.hip)
 * The reference has no counterpart; the model is defined here (FMLP-Rec, Zhou et al., WWW 2022: self-attention replaced by a learned
 * per-channel circular filter, then the Transformer's LayerNorm / GELU feed-forward block; nothing carried):
 *   inputs     the other trackers' slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k;
 *              no sqrt(D) scale, no positional encoding, no LayerNorm on the input
 *   tile       Y^{-1}[i] = x_{p-W+1+i} if p-W+1+i >= 1 else 0, i = 0 .. W-1   (left zero padding; row W-1 is the newest item)
 *   layer l    w_l = complex_weight_l [W/2+1, D] complex (stored [W/2+1, D, 2]: re, im);  h_l = irfft(w_l, n = W)  [W, D]
 *              F[i,d]  = sum_{m<W} h_l[(i-m) mod W, d] Y^{l-1}[m,d]           (= irfft(rfft(Y, ortho) w_l, n = W, ortho) over the rows)
 *              A       = LayerNorm(Y^{l-1} + F)                              (filter.ln, eps 1e-5)
 *              M       = dense_2(gelu(dense_1(A)))                           (D -> 128 -> D, the exact erf GELU)
 *              Y^l     = LayerNorm(A + M)                                    (ffn.ln)
 *   state      h_p = x_0 + Y^{L-1}[W-1]  (p >= 1),  h_0 = x_0;  s_p = decoder(h_p)
 * Rows before the first item are zero at the input of layer 0 only: the circular filter writes into them and the next layer reads them
 * (FMLP-Rec masks nothing).  The imaginary parts of the DC bin and, for even W, of the Nyquist bin have no effect; their gradient is
 * exactly 0.  The taps h_l are formed from complex_weight on the device, the phase index k n reduced modulo W as an integer first.
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, 1 <= window <= 16 (one 16-row tile), nlayers in {1, 2}, the hidden width
 * 128, max_len <= 4096.  FMLP-Rec's two dropout sites are not built.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_FMLP_MAX_WINDOW 16
#define CIRS_FMLP_MAX_LAYERS 2
#define CIRS_FMLP_HIDDEN 128

typedef struct cirs_fmlp_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t window;    /* W in 1..16: rows of the tile */
    int32_t nlayers;   /* L in {1, 2} */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
} cirs_fmlp_cfg;

typedef struct cirs_fmlp_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    /* per layer l (entries l >= nlayers are not read): */
    const float* cw[CIRS_FMLP_MAX_LAYERS];    /* layers.l.filter.complex_weight [W/2+1, D, 2] */
    const float* fln_w[CIRS_FMLP_MAX_LAYERS]; /* layers.l.filter.ln.weight [D] */
    const float* fln_b[CIRS_FMLP_MAX_LAYERS]; /* layers.l.filter.ln.bias [D] */
    const float* d1_w[CIRS_FMLP_MAX_LAYERS];  /* layers.l.ffn.dense_1.weight [128,D] */
    const float* d1_b[CIRS_FMLP_MAX_LAYERS];  /* layers.l.ffn.dense_1.bias [128] */
    const float* d2_w[CIRS_FMLP_MAX_LAYERS];  /* layers.l.ffn.dense_2.weight [D,128] */
    const float* d2_b[CIRS_FMLP_MAX_LAYERS];  /* layers.l.ffn.dense_2.bias [D] */
    const float* ln_w[CIRS_FMLP_MAX_LAYERS];  /* layers.l.ffn.ln.weight [D] */
    const float* ln_b[CIRS_FMLP_MAX_LAYERS];  /* layers.l.ffn.ln.bias [D] */
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_fmlp_weights;

typedef struct cirs_fmlp_state {
    float* x_hist; /* [B, max_len, D] the input slots: the tile of every step and the backward read them */
    int32_t* len;  /* [B] positions appended so far */
} cirs_fmlp_state;

typedef struct cirs_fmlp_grads { /* same tensors, same order as cirs_fmlp_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float *cw[CIRS_FMLP_MAX_LAYERS], *fln_w[CIRS_FMLP_MAX_LAYERS], *fln_b[CIRS_FMLP_MAX_LAYERS], *d1_w[CIRS_FMLP_MAX_LAYERS],
        *d1_b[CIRS_FMLP_MAX_LAYERS], *d2_w[CIRS_FMLP_MAX_LAYERS], *d2_b[CIRS_FMLP_MAX_LAYERS], *ln_w[CIRS_FMLP_MAX_LAYERS],
        *ln_b[CIRS_FMLP_MAX_LAYERS];
    float *dec_w, *dec_b;
} cirs_fmlp_grads;

/* cirs_avg_tracker_init / cirs_avg_tracker_step for the FMLP tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j
 * (NULL: j); init writes slot 0, len = 1; step appends one position.  Rows with skip != 0 (step), an env / user / item id out of range
 * (item < 0: the env finished), a never-initialised or a full history are left untouched: neither x_hist, len nor their row of state_out
 * is written.  state_out row stride = state_stride floats.  A cfg outside the fixed sizes (window outside 1..16, nlayers outside {1, 2}
 * among them) is refused (CIRS_E_INVALID / CIRS_E_UNSUPPORTED) with a message prefixed "fmlp tracker:" that names the member, before any
 * pointer is read. */
int cirs_fmlp_tracker_init(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w, cirs_fmlp_state* st, const int32_t* users,
                           const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_fmlp_tracker_step(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w, cirs_fmlp_state* st, const int64_t* items,
                           const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                           int64_t state_stride, void* stream);

/* cirs_avg_tracker_backward for the FMLP tracker.  No sequential pass: the forward of every buffer row is recomputed from the stored slots
 * (per layer the input tile, both LayerNorms' normalised values and inverse deviations, A and the hidden pre-activations are kept), the
 * decoder stage is the other trackers', then per row, top layer down, both LayerNorms, the two dense products transposed, the exact
 * GELU's derivative and the filter's two correlations give a gradient per tile row, which is folded into dX[b,k] in ascending p
 * (dX[b,0] = sum_p dH[b,p]); then the slot stage of the recurrent trackers.  The gradient of complex_weight is the closed form of
 * d irfft applied to the summed tap gradient; the entries without effect receive an exact 0.  Same arguments as
 * cirs_avg_tracker_backward; of st only x_hist is read.  Every gradient tensor is OVERWRITTEN.  No float atomics; every reduction has a
 * fixed order, so two calls give the same bits.  A workspace smaller than cirs_fmlp_tracker_backward_workspace_bytes(cfg, n_rows)
 * (0 for a cfg that is refused), or one not 16-byte aligned, is refused before any launch. */
int64_t cirs_fmlp_tracker_backward_workspace_bytes(const cirs_fmlp_cfg* cfg, int32_t n_rows);
int cirs_fmlp_tracker_backward(const cirs_fmlp_cfg* cfg, const cirs_fmlp_weights* w, const cirs_fmlp_state* st, const int32_t* users,
                               const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                               const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                               const cirs_fmlp_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect_gru with an FMLP tracker: the same launch sequence (one loop serves the eight, csrc/rollout.hip) with
 * cirs_fmlp_tracker_init / cirs_fmlp_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_fmlp(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                              const cirs_fmlp_cfg* trk_cfg, const cirs_fmlp_weights* trk_w, cirs_fmlp_state* trk_st,
                              const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                              const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                              int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * State tracker, a linear recurrent unit: StateTrackerLRU (csrc/lru_tracker.hip)
 * The reference has no counterpart; the model is defined here (the diagonal complex recurrence of LRU / S4-style sequence models, as
 * LRURec, Yue et al., 2023, uses it for sequential recommendation, followed by FMLP's feed-forward block).  All arithmetic is real; a
 * complex number is a (re, im) pair:
 *   inputs     the GRU tracker's slots, unchanged: slot 0 = ffn_user(Emb_user[u]), slot k >= 1 = sigmoid(fnn_gate([r_k, a_k])) * a_k
 *   lambda     = exp(-exp(nu_log)) (cos phi, sin phi), phi = exp(theta_log);  gamma = exp(gamma_log)      (|lambda| < 1 by construction)
 *   v_p        = W_in x_p + b_in                  (W_in [2D, D]: rows 0..D-1 the real part, D..2D-1 the imaginary part)
 *   h_p        = lambda * h_{p-1} + gamma * v_p, h_{-1} = 0     (the complex product per feature d; gamma scales both parts of feature d):
 *                  h_re' = lr h_re - li h_im + gamma v_re      h_im' = lr h_im + li h_re + gamma v_im
 *   y_p        = W_out [h_re ; h_im] + b_out      (W_out [D, 2D]: the real part of a complex read-out)
 *   z_p        = LayerNorm(y_p + x_p)             (lru.ln, eps 1e-5)
 *   m_p        = LayerNorm(z_p + W2 gelu(W1 z_p + b1) + b2)     (D -> 128 -> D, the exact (erf) GELU, ffn.ln);  s_p = decoder(m_p)
 * Position 0 (the user slot) is the first input of the recurrence.  An env carries 2 D floats whatever its position.
 * Fixed dims of this build: dim_model == 32, dim_state <= 32, ONE layer (the cfg keeps the GRU tracker's `nlayers` member so that the two
 * cfgs have one layout; any value but 1 is refused), hidden width 128, max_len <= 4096.  LRURec's dropout sites are not built.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_LRU_MAX_LAYERS 1
#define CIRS_LRU_HIDDEN 128

typedef struct cirs_lru_cfg {
    int32_t n_users, n_items;
    int32_t dim_model; /* D = 32 */
    int32_t dim_state; /* S <= 32 */
    int32_t nlayers;   /* 1 */
    int32_t max_len;   /* MAX_TURN + 1 */
    int32_t n_env;     /* B: leading dimension of the state arrays */
} cirs_lru_cfg;

typedef struct cirs_lru_weights {
    const float* emb_user;                /* embedding_dict.feat_user.weight [U,D] */
    const float* emb_item;                /* embedding_dict.feat_item.weight [I,D] */
    const float *ffn_user_w, *ffn_user_b; /* [D,D], [D] */
    const float *gate_w, *gate_b;         /* fnn_gate [D,1+D] (input order [r, a]), [D] */
    const float *nu_log, *theta_log, *gamma_log; /* lru.nu_log, lru.theta_log, lru.gamma_log [D] */
    const float *in_w, *in_b;             /* lru.in_proj [2D,D] (rows: real part | imaginary part), [2D] */
    const float *out_w, *out_b;           /* lru.out_proj [D,2D] (columns: real part | imaginary part), [D] */
    const float *lln_w, *lln_b;           /* lru.ln [D], [D] */
    const float *d1_w, *d1_b;             /* ffn.dense_1 [128,D], [128] */
    const float *d2_w, *d2_b;             /* ffn.dense_2 [D,128], [D] */
    const float *ln_w, *ln_b;             /* ffn.ln [D], [D] */
    const float *dec_w, *dec_b;           /* decoder [S,D], [S] */
} cirs_lru_weights;

typedef struct cirs_lru_state {
    float* x_hist; /* [B, max_len, D] the input slots (what the backward recomputes from) */
    float* h_re;   /* [1, B, D] the carried state, real part */
    float* h_im;   /* [1, B, D] the carried state, imaginary part */
    int32_t* len;  /* [B] positions appended so far */
} cirs_lru_state;

typedef struct cirs_lru_grads { /* same tensors, same order as cirs_lru_weights */
    float *emb_user, *emb_item, *ffn_user_w, *ffn_user_b, *gate_w, *gate_b;
    float *nu_log, *theta_log, *gamma_log, *in_w, *in_b, *out_w, *out_b, *lln_w, *lln_b;
    float *d1_w, *d1_b, *d2_w, *d2_b, *ln_w, *ln_b;
    float *dec_w, *dec_b;
} cirs_lru_grads;

/* cirs_gru_tracker_init / cirs_gru_tracker_step for the LRU tracker, same argument conventions: env_ids (nullable, [n]) = the env of row j
 * (NULL: j); init writes slot 0, h_0 = gamma * v_0, len = 1; step appends one position.  Rows with skip != 0 (step), an env / user / item id
 * out of range (item < 0: the env finished), a never-initialised or a full history are left untouched: neither the tracker state nor their
 * row of state_out is written.  state_out row stride = state_stride floats.  A cfg outside the fixed sizes is refused (CIRS_E_INVALID /
 * CIRS_E_UNSUPPORTED) with a message prefixed "lru tracker:", before any pointer is read. */
int cirs_lru_tracker_init(const cirs_lru_cfg* cfg, const cirs_lru_weights* w, cirs_lru_state* st, const int32_t* users,
                          const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream);
int cirs_lru_tracker_step(const cirs_lru_cfg* cfg, const cirs_lru_weights* w, cirs_lru_state* st, const int64_t* items,
                          const double* rew, const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out,
                          int64_t state_stride, void* stream);

/* cirs_gru_tracker_backward for the LRU tracker: recomputed from the stored slots; every dense product runs over all buffer rows at once,
 * the only sequential work is one complex multiply-add per position in the forward scan and in its adjoint (one env per wavefront).  Same
 * arguments as cirs_gru_tracker_backward; of st only x_hist is read.  The workspace is O(n_rows) + O(n_env) and does not depend on max_len.
 * Every gradient tensor is OVERWRITTEN.  No float atomics; every reduction has a fixed order, so two calls give the same bits.  A workspace
 * smaller than cirs_lru_tracker_backward_workspace_bytes(cfg, n_rows) (0 for a cfg that is refused), or one not 16-byte aligned, is refused
 * before any launch. */
int64_t cirs_lru_tracker_backward_workspace_bytes(const cirs_lru_cfg* cfg, int32_t n_rows);
int cirs_lru_tracker_backward(const cirs_lru_cfg* cfg, const cirs_lru_weights* w, const cirs_lru_state* st, const int32_t* users,
                              const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t,
                              const int32_t* offsets, const int32_t* lens, int32_t n_rows, const float* dstate,
                              const cirs_lru_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* cirs_rollout_collect_gru with an LRU tracker: the same launch sequence (one loop serves the nine, csrc/rollout.hip) with
 * cirs_lru_tracker_init / cirs_lru_tracker_step, the same arguments and the same trajectory contract. */
int cirs_rollout_collect_lru(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                             const cirs_lru_cfg* trk_cfg, const cirs_lru_weights* trk_w, cirs_lru_state* trk_st,
                             const cirs_policy_cfg* pol_cfg, const cirs_policy_weights* pol_w, const cirs_traj* traj, int32_t n_env,
                             const int32_t* users, uint64_t seed, uint32_t rng_base, uint32_t* visited, int32_t force_length,
                             int32_t greedy, const float* gumbel, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * DeepFM user model (UserModel_Pairwise) and the full-catalogue sweep
 * replaces  core/user_model_pairwise.py:98-154 (_deepfm/forward), core/user_model.py:419-447 (input_from_feature_columns),
 *           core/layers.py:43-72 (Linear), DeepCTR-Torch deepctr_torch/layers/interaction.py:26-34 (FM),
 *           layers/core.py:120-134 (DNN), :155-161 (PredictionLayer, regression), inputs.py:126-138 (combined_dnn_input)
 *           environments/KuaishouRec/env/kuaishouEnv.py:113-145 (compute_normed_reward)
 * y = sum_f w_f[x_f] + dur*w_d  +  FM(v_user, v_item, v_f0..3)  +  last . DNN([v_user, v_item, v_f0..3, dur]) + bias
 * Feature order in X: user_id, photo_id, feat0..feat3, photo_duration; the `feat` table is
 * shared by feat0..3 (row 0 = padding, trained to stay zero).  hidden == 64 (two DNN layers), emb_dim in {8,16,32,64}.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct cirs_deepfm_cfg {
    int32_t n_user_vocab, n_item_vocab, n_feat_vocab;
    int32_t emb_dim; /* E */
    int32_t hidden;  /* 64 */
} cirs_deepfm_cfg;

typedef struct cirs_deepfm_weights {
    const float *emb_user, *emb_item, *emb_feat; /* embedding_dict.{user_id,photo_id,feat}.weight [V,E]            */
    const float *lin_user, *lin_item, *lin_feat; /* linear.embedding_dict.*.weight [V] (Q12: `linear`, not linear_model) */
    const float* lin_dense;                      /* linear.weight [1] (photo_duration)                              */
    const float *w1, *b1;                        /* dnn.linears.0 [H, 6E+1], [H]                                     */
    const float *w2, *b2;                        /* dnn.linears.1 [H, H], [H]                                        */
    const float* last;                           /* last.weight [H]                                                  */
    const float* out_bias;                       /* out.bias [1]                                                     */
} cirs_deepfm_weights;

/* UserModel_Pairwise.forward on n (user,item) rows: ids index the vocab tables directly (raw ids), feats[n,4]. */
int cirs_deepfm_forward(const cirs_deepfm_cfg* cfg, const cirs_deepfm_weights* w, const int64_t* uid, const int64_t* pid,
                        const int32_t* feats, const float* dur, int32_t n, float* out, void* stream);

/* K1-K2 alone: embedding gather + linear logit + FM bi-interaction, no DNN -- the cache/HBM-bound stage.
 * replaces  core/user_model.py:419-447 (input_from_feature_columns), core/layers.py:59-70 (Linear.forward),
 *           DeepCTR-Torch deepctr_torch/layers/interaction.py:26-34 (FM.forward)
 * X[n,7] float32 rows = [user_id, photo_id, feat0..3, photo_duration] -- the reference's own input tensor of
 * UserModel_Pairwise.forward (ids as float32, exact below 2^24).  out[n] = linear logit + FM term.
 * cirs_deepfm_forward(x) == cirs_gather_fm(x) + (last . DNN(x) + out_bias) up to fp32 summation order. */
int cirs_gather_fm(const cirs_deepfm_cfg* cfg, const cirs_deepfm_weights* w, const float* X, int64_t n, float* out, void* stream);

int64_t cirs_deepfm_sweep_workspace_bytes(const cirs_deepfm_cfg* cfg, int32_t n_users, int32_t n_items);

/* Scores every (user, item) pair of users x items: pred_out[nu, ni] fp32 (nullable) and the global {min, max}
 * (minmax[2], device; must be initialised to {+inf, -inf} by the caller or by passing init_minmax != 0).
 * The DNN's first layer is split into a per-user and a per-item partial sum (each computed once), the 64x64 second
 * layer runs on the fp32 matrix cores for 32 pairs at a time, the FM cross term is one E-long dot per pair. */
int cirs_deepfm_sweep(const cirs_deepfm_cfg* cfg, const cirs_deepfm_weights* w, const int64_t* user_ids, int32_t nu,
                      const int64_t* item_ids, const int32_t* item_feats, const float* item_dur, int32_t ni,
                      float* pred_out, float* minmax, int32_t init_minmax, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* normed = (pred - min) / (max - min) in float64 (kuaishouEnv.py:139-143) */
int cirs_normed_reward(const float* pred, int64_t n, const float* minmax, double* normed_out, void* stream);

/* ---- user-model training ---------------------------------------------------------------------------
 * One optimiser step of fit_data's inner loop (reference core/user_model.py:150-170) for UserModel_Pairwise:
 *   loss = loss_kuaishou_pairwise(y, y_pos, y_neg, exposure, alpha_u[uid], beta_i[pid])   (CIRS-UserModel-kuaishou.py:262-278,
 *                                                                                         core/user_model_pairwise.py:134-151)
 *        + get_regularization_loss()                                                      (core/user_model.py:401-417)
 *   total_loss.backward(); Adam step (lr, betas, eps of torch.optim.Adam).
 * Parameters, gradients and the two Adam moments are flat fp32 buffers of cirs_deepfm_train_param_count(cfg) floats in
 * the order  emb_user [U,E] | emb_item [I,E] | emb_feat [F,E] | lin_user [U] | lin_item [I] | lin_feat [F] | lin_dense [1]
 *          | w1 [64,6E+1] | b1 [64] | w2 [64,64] | b2 [64] | last [64] | out_bias [1] | alpha_u [U] | beta_i [I]
 *          | linear_model.{user,item,feat} [U],[I],[F] | linear_model.weight [1]      (the unused duplicate of SURVEY Q12,
 *                                                                                       which the regulariser still decays).
 * Batch columns: positive pair (uid, pid, feats[n,4], dur), negative pair (same layout), y [n], exposure [n].
 * l2_embedding / l2_linear / l2_all: the three regularisation lists of the reference (embedding_dict, linear_model, all).
 * loss_out[5] = {loss, loss_y, bpr, loss_ab, reg_loss}. */
int64_t cirs_deepfm_train_param_count(const cirs_deepfm_cfg* cfg);
int64_t cirs_deepfm_train_workspace_bytes(const cirs_deepfm_cfg* cfg, int32_t n);
int cirs_deepfm_train_step(const cirs_deepfm_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                           int64_t step_before, const int64_t* uid_pos, const int64_t* pid_pos, const int32_t* feats_pos,
                           const float* dur_pos, const int64_t* uid_neg, const int64_t* pid_neg, const int32_t* feats_neg,
                           const float* dur_neg, const float* y, const float* exposure, int32_t n, int32_t use_ab,
                           float lambda_ab, float l2_embedding, float l2_linear, float l2_all, float lr, float beta1,
                           float beta2, float eps, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
/* All steps of one pass over a data set that stays on the device in the column form of the step (every column n_rows long,
 * feats [n_rows,4]): batch b is the rows order[b * batch_size .. min(n_order, (b + 1) * batch_size)) (int64, device, every entry in
 * [0, n_rows); NULL = the identity, then n_order <= n_rows; the last batch may be short).  The row kernel reads through `order`: there
 * is no gather launch, no host synchronisation and no host round trip between the steps; step_before advances per step.
 * loss_kind selects the loss of the row kernel and the meaning of `score`:
 *   0  loss_kuaishou_pairwise (score = exposure), as cirs_deepfm_train_step;
 *   1  loss_kuaishou_IPS_pairwise (DeepFM-IPS-pairwise.py:249-258): mean((yp - y)^2 w) + mean(-log sigmoid(yp - yn) w), w = score;
 *   2  loss_kuaishou_PD_pairwise (PD-pairwise.py:242-251): mean((yp pop - y)^2) + mean(-log sigmoid(yp - yn)), pop = score.
 * Kinds 1 and 2 take no alpha/beta: use_ab != 0 with them is refused (both scripts build the model without ab_columns); lambda_ab
 * is ignored.  losses_out [ceil(n_order / batch_size)][5] = per-step {loss, loss_y, bpr, loss_ab, reg_loss} (device).
 * Kind 0 is bit-identical to one cirs_deepfm_train_step per batch on the gathered rows; a single step of kind 1 or 2 is this call with
 * n_order = batch_size = n.  workspace: cirs_deepfm_train_workspace_bytes(cfg, min(batch_size, n_order)). */
int cirs_deepfm_train_epoch(const cirs_deepfm_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                            int64_t step_before, const int64_t* uid_pos, const int64_t* pid_pos, const int32_t* feats_pos,
                            const float* dur_pos, const int64_t* uid_neg, const int64_t* pid_neg, const int32_t* feats_neg,
                            const float* dur_neg, const float* y, const float* score, int64_t n_rows, const int64_t* order,
                            int64_t n_order, int32_t batch_size, int32_t loss_kind, int32_t use_ab, float lambda_ab,
                            float l2_embedding, float l2_linear, float l2_all, float lr, float beta1, float beta2, float eps,
                            float* losses_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the DICE debiasing baseline (UserModel_DICE) ------------------------------------------------------------------
 * replaces  core/user_model_DICE.py:122-160 (_deepfm), :162-187 (get_loss), :189-192 (forward), DICE.py:273-286 (loss_kuaishou_DICE),
 *           core/user_model.py:401-417 (get_regularization_loss) and the inner loop of fit_data (core/user_model.py:150-170).
 * Two DeepFM networks over five shared embedding tables (entity_dim == feature_dim == E):
 *   main  fields [user_int, user_con, photo_int, photo_con, feat0..3] + duration: linear_main + FM over 8 fields + dnn_main -> last_main
 *         + out_main.bias; run on the positive row and on the negative row (same user ids, the negative item's columns);
 *   ui    fields (user, photo): linear_ui + FM over 2 fields + dnn_ui -> last_ui + out_ui.bias; run on (user_int, photo_int) and on
 *         (user_con, photo_con), positive and negative item each.  linear_ui has the tables user_int / photo_int only and is indexed
 *         with the ids of the call's own columns (the con ids in the con calls), as the reference does.
 * loss = mean((yp - y)^2) + mean(-log sigmoid(yp - yn)) + mean(-log sigmoid(yp_con - yn_con) s) + mean(-log sigmoid(yp_int - yn_int) [s < 0]),
 * s = score in {+1, -1}.
 * Parameters, gradients and the two Adam moments are flat fp32 buffers of cirs_dice_train_param_count(cfg) floats in the order
 *   embedding_dict.{user_int [U,E] | user_con [U,E] | photo_int [I,E] | photo_con [I,E] | feat [F,E]}
 * | linear_main.embedding_dict.{user_int [U] | user_con [U] | photo_int [I] | photo_con [I] | feat [F]} | linear_main.weight [1]
 * | linear_ui.embedding_dict.{user_int [U] | photo_int [I]}
 * | dnn_main.linears.0 [64,8E+1],[64] | dnn_main.linears.1 [64,64],[64] | last_main [64] | out_main.bias [1]
 * | dnn_ui.linears.0 [64,2E],[64] | dnn_ui.linears.1 [64,64],[64] | last_ui [64] | out_ui.bias [1]
 * | linear_model.embedding_dict.{user_int [U] | user_con [U] | photo_int [I] | photo_con [I] | feat [F]} | linear_model.weight [2]
 *   (the base class's unused copy: no data gradient, decayed by l2_linear + l2_all).
 * emb_dim in {8, 16, 32}, hidden == 64.  Row 0 of embedding_dict.feat (padding_idx) gets no data gradient. */
typedef struct cirs_dice_cfg {
    int32_t n_user_vocab, n_item_vocab, n_feat_vocab;
    int32_t emb_dim; /* E */
    int32_t hidden;  /* 64 */
} cirs_dice_cfg;

int64_t cirs_dice_train_param_count(const cirs_dice_cfg* cfg);
int64_t cirs_dice_train_workspace_bytes(const cirs_dice_cfg* cfg, int32_t n);
/* All steps of one pass over a data set resident on the device in column form, like cirs_deepfm_train_epoch: the 16 columns of the
 * reference's x as uid_int, uid_con, pid_int, pid_con, feats_pos [n_rows,4], dur_pos | pid_int_neg, pid_con_neg, feats_neg [n_rows,4],
 * dur_neg (the int and con id columns are separate arguments and need not be equal), then y and score.  Batch b is the rows
 * order[b * batch_size .. min(n_order, (b + 1) * batch_size)) (int64, device; NULL = the identity, then n_order <= n_rows), read by the
 * row kernel itself; an entry outside [0, n_rows) is not read and turns that step's loss into NaN.  The steps are queued back to back
 * without a host round trip; step_before advances per step.  losses_out [ceil(n_order / batch_size)][6] = per-step
 * {loss, loss_y, bpr_click, bpr_con, bpr_int, reg_loss} (device).  A single step is this call with n_order = batch_size = n.
 * Every sum has a fixed order (no float atomics): two runs give identical bits.
 * Precondition, as for cirs_deepfm_train_epoch: every id of the data set lies inside its table (user ids in [0, n_user_vocab), photo ids in
 * [0, n_item_vocab), feat ids in [0, n_feat_vocab)); the row kernel indexes the tables with them unchecked (DiceTrainer.load checks once).
 * workspace: cirs_dice_train_workspace_bytes(cfg, min(batch_size, n_order)). */
int cirs_dice_train_epoch(const cirs_dice_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t step_before,
                          const int64_t* uid_int, const int64_t* uid_con, const int64_t* pid_int, const int64_t* pid_con,
                          const int32_t* feats_pos, const float* dur_pos, const int64_t* pid_int_neg, const int64_t* pid_con_neg,
                          const int32_t* feats_neg, const float* dur_neg, const float* y, const float* score, int64_t n_rows,
                          const int64_t* order, int64_t n_order, int32_t batch_size, float l2_embedding, float l2_linear, float l2_all,
                          float lr, float beta1, float beta2, float eps, float* losses_out, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* UserModel_DICE.forward on n rows (uid, pid, feats [n,4], dur): the main DeepFM with the user and the photo id in both of their
 * columns, over the flat parameter buffer above.  A row with an id outside its table is not read and gives NaN. */
int cirs_dice_forward(const cirs_dice_cfg* cfg, const float* params, const int64_t* uid, const int64_t* pid, const int32_t* feats,
                      const float* dur, int64_t n, float* out, void* stream);

/* ---- validation pass of the Kuaishou user models (csrc/userval.hip) -------------------------------------------------
 * replaces  core/user_model.py:351-359 (evaluate_data), :361-399 (predict_data) and the scripts' metric lambdas
 *           (CIRS-UserModel-kuaishou.py:204-207, DICE.py:236-239) for UserModel_Pairwise.forward and UserModel_DICE.forward.
 * One launch scores the n rows (uid, pid, feats [n,4], dur) in tiles of 32 rows per wavefront -- both dense layers on the fp32 matrix
 * cores, the weights staged in LDS once per workgroup -- and reduces the errors against y [n] (float64):
 *   pred = the fp32 forward (cirs_deepfm_forward / cirs_dice_forward up to fp32 summation order), e = (double)pred - y[r];
 *   pred_out [n] fp32, NULL: no prediction is written;  sums_out [2] float64 = {sum |e|, sum e^2}, NULL: y is not read.
 * At least one of the two outputs is given.  Per-wavefront partial pairs go to the workspace and a final launch adds them in index
 * order: no atomics, two runs give the same bits.  n < 1 is refused (CIRS_E_INVALID).  emb_dim as for the forward entries
 * ({8,16,32,64} DeepFM, {8,16,32} DICE), hidden == 64.
 * Precondition, as for cirs_deepfm_train_epoch: every id lies inside its table; the kernel indexes the tables with them unchecked
 * (cirs_hip.userval.ValSet checks once at load).  workspace: cirs_*_validate_workspace_bytes(cfg, n), needed with sums_out only. */
int64_t cirs_deepfm_validate_workspace_bytes(const cirs_deepfm_cfg* cfg, int64_t n);
int cirs_deepfm_validate(const cirs_deepfm_cfg* cfg, const cirs_deepfm_weights* w, const int64_t* uid, const int64_t* pid,
                         const int32_t* feats, const float* dur, const double* y, int64_t n, float* pred_out, double* sums_out,
                         void* workspace, int64_t workspace_bytes, void* stream);
int64_t cirs_dice_validate_workspace_bytes(const cirs_dice_cfg* cfg, int64_t n);
int cirs_dice_validate(const cirs_dice_cfg* cfg, const float* params, const int64_t* uid, const int64_t* pid, const int32_t* feats,
                       const float* dur, const double* y, int64_t n, float* pred_out, double* sums_out, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ---- the disjoint-arm LinUCB baseline (csrc/linucb.hip) --------------------------------------------------------------
 * replaces  core/policy/linucb.py (paths relative to the reference root).  Everything is float64.  n_arms arms keep A [n_arms, d, d]
 * (identity at start) and b [n_arms, d] (zero at start); 2 <= d <= 16, anything else is refused with CIRS_E_UNSUPPORTED.
 *
 * cirs_linucb_update replaces the per-row loop of linucb_trainer (:168-180) and linucb_disjoint_arm.reward_update (:59-68):
 *   x [n_rows, ld >= d], y [n_rows]: the log;  order [m]: row indices grouped by arm and, inside an arm, in log order;
 *   seg [n_arms + 1]: arm a owns order[seg[a] .. seg[a + 1]).  Every element of A_a and b_a is owned by one lane, which walks the
 *   arm's rows in that order with a rounded product and then a rounded sum: A and b are bit-identical to the reference's loop.
 *   It continues from the A and b it is given (epochs accumulate).  m == 0 or n_arms == 0: nothing is launched, 0 is returned.
 *   An entry of order outside [0, n_rows) adds nothing.
 * cirs_linucb_solve replaces the A_inv and theta properties (:33-40): A_inv [n_arms, d, d] = inv(A_a), theta [n_arms, d] = inv(A_a) b_a
 *   for every arm (arms == NULL) or for arms[0 .. n_listed) only; Cholesky plus iterative refinement with the residual in twice the
 *   working precision.
 * cirs_linucb_score replaces calc_UCB / calc_reward (:28-57) inside the loops of recommend_k_item (:133-159) and select_arm (:77-103):
 *   x_fixed == NULL: for every user u < n_users and arm a, x = [users[u], a, item_feats[a, 0 .. d - 2)] (item_feats [n_arms, d - 2]);
 *   x_fixed [d]: the one x of select_arm / forward scored against every arm (n_users is ignored, one output row).
 *   mean = theta_a^T x, ucb = mean + alpha sqrt(x^T A_inv_a x).  best_arm [rows] int64 = the first arg-max of ucb over the arms,
 *   best_mean [rows] = that arm's mean; ucb_out / mean_out / var_out [rows, n_arms] or NULL each (var = x^T A_inv_a x).
 * cirs_linucb_predict replaces the per-row loop of evaluate_data (:120-126): y_pred[r] = theta[arm[r]]^T x[r] (x [n, ld >= d]),
 *   0 where arm[r] lies outside [0, n_arms). */
int cirs_linucb_update(double* A, double* b, int32_t n_arms, int32_t d, const double* x, int64_t ld, int64_t n_rows, const double* y,
                       const int64_t* order, int64_t m, const int64_t* seg, void* stream);
int cirs_linucb_solve(const double* A, const double* b, int32_t n_arms, int32_t d, const int32_t* arms, int32_t n_listed, double* A_inv,
                      double* theta, void* stream);
int cirs_linucb_score(const double* A_inv, const double* theta, int32_t n_arms, int32_t d, const double* users, int32_t n_users,
                      const double* item_feats, const double* x_fixed, double alpha, int64_t* best_arm, double* best_mean,
                      double* ucb_out, double* mean_out, double* var_out, void* stream);
int cirs_linucb_predict(const double* theta, int32_t n_arms, int32_t d, const double* x, int64_t ld, const int64_t* arm, int64_t n,
                        double* y_pred, void* stream);

/* ---- user-model dataset preparation ---------------------------------------------------------------
 * cirs_exposure_history replaces compute_exposure_each_user / the per-user loop of compute_exposure_effect_kuaishouRec
 * (reference core/util.py:56-76,135-169): rows are the logged interactions in file order, a user's rows contiguous;
 *   user_start[r] = index of the first row of row r's user, photo[r] item id, timestamp[r] (float64 seconds);
 *   dist [n_items, n_items] float64 (1 / similarity) or NULL -> 1 / Jaccard from item_cats [n_items] packed category words;
 *   exposure_out[r] = sum_{j in [user_start[r], r)} exp(-(max(ts_r - ts_j, ...)) * dist[photo_j, photo_r] / tau), dt == 0 -> 1.
 * cirs_find_negative replaces find_negative (core/util.py:173-196): seen_small / seen_big are bitmaps
 *   [n_users, ceil(n_items/32)] of the (user, item) pairs present in the small / big matrix; absent_id = 1225 for KuaiRec;
 *   neg_out[i] = the sampled negative item (or -1 if none exists). */
int cirs_exposure_history(const int64_t* user_start, const int32_t* photo, const double* timestamp, int64_t n_rows,
                          const double* dist, const uint32_t* item_cats, int32_t n_items, double tau, double* exposure_out,
                          void* stream);
int cirs_find_negative(const int64_t* user_ids, const int64_t* photo_ids, int64_t n, const uint32_t* seen_small,
                       const uint32_t* seen_big, int32_t n_items, int64_t absent_id, int64_t* neg_out, void* stream);
/* The score columns of the debiasing baselines: the count of every item among the log rows of a time bin.
 * cirs_item_bin_counts replaces the Series.map passes of compute_IPS_kuaishouRec (DeepFM-IPS-pairwise.py:79-86) and
 * compute_popularity_kuaishouRec_pairwise (PD-pairwise.py:76-108): photo [n] item ids, timestamp [n] float64, bounds [num_bin + 1]
 * float64; row r falls in bin b when bounds[b] <= ts < bounds[b + 1], the last bin closed (PD-pairwise.py:93-96).  timestamp NULL: one
 * bin takes every row (num_bin must be 1, bounds unused).  bin_out [n] = the row's bin, -1 when no bin takes it or its item id is
 * outside [0, n_items); counts [num_bin, n_items] int32 is cleared and filled with integer atomics (independent of the order).
 * cirs_item_bin_gather: out[r] = table[bin[r], photo[r]] (float64 [num_bin, n_items]), 0 where bin[r] < 0.  The host turns counts
 * into the score table with the reference's own float64 arithmetic; the device does none. */
int cirs_item_bin_counts(const int32_t* photo, const double* timestamp, int64_t n, const double* bounds, int32_t num_bin,
                         int32_t n_items, int32_t* bin_out, int32_t* counts, void* stream);
int cirs_item_bin_gather(const int32_t* photo, const int32_t* bin, int64_t n, const double* table, int32_t num_bin,
                         int32_t n_items, double* out, void* stream);

/* ---- the user model as a static recommendation policy ---------------------------------------------
 * cirs_select_items replaces the tail of UserModel.recommend_k_item (reference core/user_model.py:296-346, k = 1) for n
 * users at once, given their catalogue scores (cirs_deepfm_sweep):
 *   scores [n, row_stride >= n_items] f32;  bonus [n_items] or NULL (UCB bound, :303-314);
 *   visited [n, ceil(n_items/32)] or NULL (recommended_ids, :263-266);  skip [n] or NULL (row inactive -> act -1);
 *   softmax != 0: multinomial(softmax(u_value)) as arg-max of u_value + Gumbel noise (gumbel [n, n_items] supplied, or
 *   the counter-based generator keyed (seed, rng_step, row, item));  softmax == 0: arg-max, lowest id on ties (:331);
 *   epsilon: probability of a uniform random non-removed item instead (:333-335).
 *   act_out [n] int64 (-1: no item), value_out [n] or NULL: u_value of the chosen item (value_rec, :346).
 * cirs_rollout_static replaces the loop of interactive_evaluation (reference evaluation.py:87-120) for n_env
 * trajectories in lock-step: select -> mark visited -> env step -> forced length; traj->value holds reward_pred. */
int cirs_select_items(const float* scores, int64_t row_stride, int32_t n, int32_t n_items, int32_t softmax,
                      const float* bonus, const uint32_t* visited, const uint8_t* skip, float epsilon, const float* gumbel,
                      uint64_t seed, uint32_t rng_step, int64_t* act_out, float* value_out, void* stream);
int cirs_rollout_static(const cirs_env_cfg* env_cfg, const cirs_env_tables* env_tab, cirs_env_state* env_st,
                        const float* scores, int64_t row_stride, const float* bonus, const cirs_traj* traj, int32_t n_env,
                        int32_t t_begin, int32_t t_end, int32_t softmax, float epsilon, uint64_t seed, uint32_t rng_base,
                        uint32_t* visited, int32_t force_length, int64_t* obs_scratch, void* stream);

/* ---- feature hashing (BASELINE configs[4]: open-vocabulary ids hashed into fixed-size tables) -----------------------
 * out[i] = splitmix64(ids[i]) mod n_buckets.  No reference counterpart (DeepCTR-Torch inputs.py:31-33 only prints a notice
 * for use_hash): the mapping is this build's own and is restated bit for bit by the oracle. */
int cirs_hash_ids(const int64_t* ids, int64_t n, int64_t n_buckets, int64_t* out, void* stream);

/* ---- minibatch shuffle (Batch.split(shuffle=True): np.random.permutation(n), tianshou/data/batch.py:734-744) --------------
 * out[i] = P(i), a keyed pseudo-random permutation of [0, n): 6-round Feistel network over splitmix64 with cycle walking, one
 * thread per element, no sort and no host round trip.  Same (seed, tag) -> same permutation (ranks of a data-parallel learner
 * pass the same pair).  The oracle restates it bit for bit. */
int cirs_random_permutation(int64_t n, uint64_t seed, uint64_t tag, int32_t* out, void* stream);
/* out[c][i], c < count: the permutations of tags tag0 .. tag0 + count - 1 from one launch (the repeats of an update, core/policy/ppo.py:173-181). */
int cirs_random_permutations(int64_t n, uint64_t seed, uint64_t tag0, int32_t count, int32_t* out, void* stream);

/* ---- per-kernel timing hook (measurement only; no reference counterpart) ----------------------------------------------
 * cirs_prof_start arms HIP-event pairs around the next `max_samples` launches of one named kernel, recorded on the stream
 * the kernel is launched on; cirs_prof_stop waits for them and returns the summed duration and the sample count.
 * kernel_id: 1 = head_bwd_fused_kernel (PPO minibatch, fused actor-head backward), 2 = head_stats_kernel (PPO
 * minibatch, forward statistics), 3 = actor_head_kernel (rollout sampler).  bench.py's `roofline` object uses it so that
 * `seconds_per_launch` is the same quantity as the kernel's average in the rocprofv3 --kernel-trace --stats summary. */
int cirs_prof_start(int32_t kernel_id, int32_t max_samples);
int cirs_prof_stop(double* total_seconds, int32_t* n_samples);

/* ---- evaluation metrics on device trajectories ---------------------------------------------------
 * Replaces the buffer walks of Callback_Coverage_Count.on_epoch_end (reference evaluation.py:303-352) and the
 * row test of get_feat_dominate_dict (evaluation.py:36-44):
 *   act       [n] int64: the time-major act tensor of a rollout ([T,B], -1 where an env had finished)
 *   item_flag [n_items] u8 or NULL: 1 if the item has one of the dominating feature values
 *   bitmap    [ceil(n_items/32)] scratch
 *   out3      {hit_item, n_acts, n_flagged}: CV = hit_item / n_items, CV_turn = hit_item / n_acts,
 *             ifeat_feat = n_flagged / n_acts */
int cirs_eval_coverage(const int64_t* act, int64_t n, int32_t n_items, const uint8_t* item_flag, uint32_t* bitmap,
                       int64_t* out3, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Environment: batched VirtualTaobao (VirtualTB-v0 and SimulatedEnv(VirtualTB-v0)), csrc/virtualtb.hip
 * replaces  environments/VirtualTaobao/virtualTB/envs/virtualTB.py:11-146 (VirtualTB.reset/step, the user generator,
 *           the action model) and the VirtualTB branch of core/env/simulatedEnv/simulated_env.py:44-193 (exposure effect,
 *           UserModel_MMOE reward), one env at a time in the reference.  One launch per vector step.
 * Noise: Philox4x32-10, key = seed, counter = (env id, per-env event index, block, tag); tag 0 = the 21 Gumbels of a step
 * (clicks: words 0..10, second draw: words 11..20), tag 1 = a user draw (words 0..127 -> z = u01, words 128..215 -> the 88
 * Gumbels of the 11 groups).  Every reset and every step of an env is one event; a redraw inside a step uses that step's
 * event with tag 1.  Weights are fp32, stored TRANSPOSED ([in][out], row-major) unless noted.
 * ---------------------------------------------------------------------------------------------------------- */
#define CIRS_VTB_USER_DIM 88
#define CIRS_VTB_ACTION_DIM 27
#define CIRS_VTB_GROUPS 11
#define CIRS_VTB_NOISE_COLS 237 /* 21 step Gumbels | 128 z | 88 user Gumbels */

typedef struct cirs_vtb_cfg {
    int32_t n_env;             /* envs held by the state arrays; env ids must lie in [0, n_env)               */
    int32_t max_turn;          /* VirtualTB.max_turn; history rows per env                                    */
    int32_t num_leave_compute; /* N: the exit rule looks at the last min(t, N-1) actions          */
    int32_t simulated;         /* 1: SimulatedEnv(VirtualTB-v0), MMoE reward; 0: raw VirtualTB-v0, reward = clicks */
    int32_t version;           /* simulated: 1 = r/(1+e), 2 = r - e                                           */
    int32_t use_exposure;      /* SimulatedEnv.use_exposure_intervention                                      */
    /* MMoE shape (simulated kind): only UserModel_MMOE's all-dense one-task regression build is supported:
     * d_in 118, dnn (128, 128), 4 experts of dim 8, 1 task of logit dim 1 */
    int32_t mmoe_d_in, mmoe_dnn_layers, mmoe_h1, mmoe_h2, mmoe_experts, mmoe_expert_dim, mmoe_tasks, mmoe_task_dim;
    double leave_threshold;    /* L2 distance                                                                  */
    double tau;                /* exposure: tau <= 0 -> 0                                                      */
    double gamma_exposure;
} cirs_vtb_cfg;

typedef struct cirs_vtb_weights {
    const float *gen_w1, *gen_b1, *gen_w2, *gen_b2;                  /* generator 128 -> 128 -> 88          */
    const float *act_w1, *act_b1, *act_w2, *act_b2, *act_w3, *act_b3; /* action model 116 -> 128 -> 256 -> 21 */
    const float *mm_w1, *mm_b1, *mm_w2, *mm_b2;                      /* MMoE dnn 118 -> 128 -> 128 (ReLU)   */
    const float *mm_we, *mm_be;                                       /* experts 128 -> 32 (column d*4 + e)  */
    const float *mm_wg;                                               /* gate 128 -> 4, no bias              */
    const float *mm_wt;                                               /* tower [8] (8 -> 1, no bias)         */
    const float *mm_wlin;                                             /* linear_model_task [118]             */
    const float *mm_bias;                                             /* [1]                                 */
} cirs_vtb_weights;

typedef struct cirs_vtb_state { /* mutable, SoA over n_env envs */
    int32_t* task_user;   /* [n_env,11] one-hot positions (0..87) of the wrapped VirtualTB's cur_user        */
    int32_t* sim_user;    /* [n_env,11] SimulatedEnv.cur_user (set by reset only)                            */
    int32_t* turn;        /* [n_env]    total_turn                                                          */
    uint32_t* event;      /* [n_env]    noise event counter                                                  */
    double* prev_reward;  /* [n_env]    SimulatedEnv.reward (input of the next MMoE call)                    */
    double* cum_reward;   /* [n_env]                                                                         */
    int32_t* lst_action;  /* [n_env,2]  (clicks, second draw); (0, 0) after a done step                      */
    float* hist;          /* [n_env,max_turn,27] the actions of turns 0..max_turn-1                          */
} cirs_vtb_state;

/* draw a user for envs env_ids[0..n) (NULL = 0..n-1) and zero their turn / rewards / history; obs_out [n,91] double
 * (nullable) = [user one-hot 88 | 0, 0 | 0]. */
int cirs_vtb_reset(const cirs_vtb_cfg* cfg, const cirs_vtb_weights* w, cirs_vtb_state* st, uint64_t seed,
                   const int32_t* env_ids, int32_t n, double* obs_out, void* stream);
/* one vector step of envs env_ids[0..n) (distinct ids) with actions[n,27] fp32.  Outputs (position j):
 *   obs_out [n,30] double  simulated: [action | reward, 0, t+1]; raw: [action | a, b, t+1], [action | 0, 0, t+1] when done
 *   rew_out [n]    double  simulated: MMoE reward after the exposure effect; raw: clicks a
 *   done_out[n]    uint8   exit rule OR t >= max_turn - 1
 *   ctr_out [n]    double  cum_reward / (t+1) / 10
 *   expo_out[n]    double  (nullable) exposure effect of the step (simulated kind; 0 otherwise)
 * The simulated kind supports t <= max_turn (the caller rejects later steps); the raw kind any t. */
int cirs_vtb_step(const cirs_vtb_cfg* cfg, const cirs_vtb_weights* w, cirs_vtb_state* st, uint64_t seed,
                  const float* actions, const int32_t* env_ids, int32_t n, double* obs_out, double* rew_out,
                  uint8_t* done_out, double* ctr_out, double* expo_out, void* stream);
/* the noise the kernels draw for (env_ids[j], events[j]): out [n,237] fp32 = [21 step Gumbels | z (128) | 88 user Gumbels],
 * bit for bit. */
int cirs_vtb_noise(uint64_t seed, const int32_t* env_ids, const uint32_t* events, int32_t n, float* out, void* stream);
/* UserModel_MMOE.forward on x[n,118] -> y_out[n] (unclamped), the user-model part of cirs_vtb_step. */
int cirs_vtb_mmoe_forward(const cirs_vtb_cfg* cfg, const cirs_vtb_weights* w, const float* x, int32_t n, float* y_out,
                          void* stream);

/* ---- VirtualTaobao static baselines: a whole evaluation per launch (csrc/vtb_static.hip, csrc/vtb_mmoe.h) -------------------
 * replaces  evaluation.py:238-282 (test_taobao: num_trajectory trajectories of a two-task UserModel_MMOE played against a
 *           VirtualTB in static-state mode, one batch-1 forward and one host env step at a time; called at every epoch end by
 *           MLP-taobao.py and MLP-epsilonGreedy-taobao.py) with core/user_model_mmoe.py:232-262 (the forward).
 * Trajectory i is env id i of the Philox convention above: event 0 = its user draw (tag 1), event 1 + t = turn t (tag 0: the 21
 * step Gumbels; tag 2: word 0 -> the epsilon uniform u01, words 1..27 -> the 27 exploration uniforms u01).  The user redrawn by
 * VirtualTB.step on done is not drawn: test_taobao resets the env before it is ever seen. */
#define CIRS_VTB_STATIC_STATE_DIM 91  /* [user one-hot 88 | last clicks, last second draw | turn] */
#define CIRS_VTB_STATIC_MAX_DNN 3
#define CIRS_VTB_STATIC_NOISE_COLS 265 /* cirs_vtb_noise's 237 | epsilon uniform | 27 exploration uniforms */
/* bytes of cirs_vtb_static_out.metrics: double[4] | int64[2] | int32 len[n_traj] */
#define CIRS_VTB_STATIC_METRICS_BYTES(n_traj) (48 + 4 * (int64_t)(n_traj))

typedef struct cirs_vtb_mmoe_shape { /* all-dense UserModel_MMOE with two regression tasks (y_columns: feat_item, y) */
    int32_t d_in;                             /* 91                                                       */
    int32_t n_dnn;                            /* 1..CIRS_VTB_STATIC_MAX_DNN hidden layers (ReLU)          */
    int32_t hidden[CIRS_VTB_STATIC_MAX_DNN];  /* each 1..256                                              */
    int32_t experts, expert_dim;              /* experts * expert_dim <= 64                               */
    int32_t n_tasks;                          /* 2                                                        */
    int32_t task_dim[2];                      /* (27, 1)                                                  */
} cirs_vtb_mmoe_shape;

typedef struct cirs_vtb_mmoe_weights { /* fp32, TRANSPOSED ([in][out]) like cirs_vtb_weights */
    const float* dnn_w[CIRS_VTB_STATIC_MAX_DNN];
    const float* dnn_b[CIRS_VTB_STATIC_MAX_DNN];
    const float *expert_w, *expert_b; /* h_last -> experts * expert_dim (column d * experts + e) */
    const float* gate_w[2];           /* h_last -> experts, no bias, per task                    */
    const float* tower_w[2];          /* [expert_dim][task_dim], no bias                         */
    const float* lin_w;               /* linear_model_task of the dim-1 task [d_in]              */
    const float* bias[2];             /* out.<task>.bias [task_dim]                              */
} cirs_vtb_mmoe_weights;

typedef struct cirs_vtb_static_cfg {
    int32_t n_traj;            /* 1..1048576                                                                  */
    int32_t max_turn;          /* VirtualTB.max_turn, 1..16383                                                */
    int32_t num_leave_compute; /* N of the exit rule, as cirs_vtb_cfg                                         */
    int32_t reserved;          /* 0                                                                           */
    double leave_threshold;
    double epsilon;            /* 0..1; 0: no exploration draw is compared (evaluation.py:253)                */
    cirs_vtb_mmoe_shape policy;
} cirs_vtb_static_cfg;

typedef struct cirs_vtb_static_out { /* rows (trajectory i, turn t) at i * max_turn + t; turns >= len[i] are not written */
    int32_t* user;      /* [n_traj,11]   one-hot positions of the trajectory's user                                 */
    float* state;       /* [rows,91]     the policy's input                                                         */
    float* action;      /* [rows,27]     the action played (raw prediction or the exploration uniforms); the kernel
                                         reads the exit rule's window back from here                               */
    float* reward_pred; /* [rows]        the dim-1 task's output                                                    */
    int32_t* reward;    /* [rows]        clicks 0..10                                                               */
    uint8_t* done;      /* [rows]                                                                                   */
    uint8_t* explore;   /* [rows]        1: the epsilon branch fired                                                */
    void* metrics;      /* CIRS_VTB_STATIC_METRICS_BYTES: {ctr, click_loss, len_tra, R_tra} double | {clicks, turns}
                                         int64 | len[n_traj] int32                                                  */
} cirs_vtb_static_out;

/* bytes of cirs_vtb_static_eval's workspace (per-trajectory click counts and |reward_pred - reward| sums); -1 on a bad cfg */
int64_t cirs_vtb_static_workspace_bytes(const cirs_vtb_static_cfg* cfg);
/* Play n_traj trajectories from the user draw to the exit: ONE vtb_static_eval_kernel launch (4 trajectories per workgroup, the
 * turn loop inside), then a one-workgroup reduction of the metrics in a fixed order: click_loss sums fp64 in turn order inside a
 * trajectory, the trajectories' sums in trajectory order; clicks and turns are integers.  `w`: generator and action model only
 * (the mm_* fields are not read). */
int cirs_vtb_static_eval(const cirs_vtb_static_cfg* cfg, const cirs_vtb_weights* w, const cirs_vtb_mmoe_weights* pw, uint64_t seed,
                         const cirs_vtb_static_out* out, void* workspace, int64_t workspace_bytes, void* stream);
/* the noise cirs_vtb_static_eval draws for (trajectory traj_ids[j], turn turns[j]): out [n,265] fp32 = [21 step Gumbels of the
 * turn | z (128) | 88 user Gumbels (the trajectory's, the same at every turn) | epsilon uniform | 27 exploration uniforms] */
int cirs_vtb_static_noise(uint64_t seed, const int32_t* traj_ids, const int32_t* turns, int32_t n, float* out, void* stream);

/* ---- VirtualTaobao PPO rollout on the device (csrc/vtb_rollout.hip) -------------------------------------------------------
 * The policy side of CIRS-RL-taobao.py's per-step loop: the dense-feature state tracker (HostStateTracker: ffn_user / fnn_gate
 * input slot, positional encoding, post-norm causal TransformerEncoder, decoder) as a K/V-cached decode step, and ActorProb over
 * its Net trunk with a Gaussian draw.  One vtb_policy_step_kernel launch + one vtb_step_kernel launch per vector step. */
#define CIRS_VTB_RO_MAX_LAYERS 4
#define CIRS_VTB_RO_MAX_HIDDEN 3

/* The model both stages run: HostStateTracker + ActorProb over a Net trunk (CIRS-RL-taobao.py).  Declared once and embedded in
 * cirs_vtb_rollout_cfg and cirs_vtb_learn_cfg; its rules are checked in one place (csrc/vtb_model.h).  The capacity limits noted
 * per field are the rollout's; the learner's are wider (d_hid <= 1024, dim_state <= 128). */
typedef struct cirs_vtb_model_cfg {
    int32_t dim_model;         /* D == 27 (the action slot), D % nhead == 0                                      */
    int32_t nhead;
    int32_t d_hid;             /* <= 256                                                                         */
    int32_t nlayers;           /* 1..4                                                                           */
    int32_t dim_state;         /* <= 64                                                                          */
    int32_t max_len;           /* tracker MAX_TURN rows (pe rows, K/V cache rows); nhead * max_len <= 2048        */
    int32_t n_hidden;          /* actor trunk layers 1..3                                                        */
    int32_t hidden[CIRS_VTB_RO_MAX_HIDDEN]; /* trunk widths <= 128                                               */
    int32_t unbounded;         /* 1: mu = head output; 0: max_action * tanh(head output)                         */
    int32_t conditioned_sigma; /* 1: sigma = exp(clamp(sigma head, -20, 2)); 0: exp(sigma_param)                */
    float max_action;
    float dropout_p;           /* 0 <= p < 1; 0 = no mask work.  With the next two: the position-keyed dropout key of one collect */
    int32_t drop_env_base;     /* dropout env id = drop_env_base + env                                           */
    uint64_t dropout_seed;     /* dropout key of this collect                                                    */
} cirs_vtb_model_cfg;

typedef struct cirs_vtb_rollout_cfg {
    int32_t n_env;             /* == vtb_cfg->n_env                                                              */
    int32_t max_turn;          /* vector steps of a collect; == vtb_cfg->max_turn and <= model.max_len - 1       */
    int32_t force_length;      /* > 0: every episode ends after this many steps, overriding the env (<= max_turn) */
    int32_t bound_method;      /* mapped action: 0 none, 1 clip to [-1, 1], 2 tanh                               */
    int32_t action_scaling;    /* 1: [-1, 1] -> [act_low, act_high]                                              */
    cirs_vtb_model_cfg model;
    uint64_t env_seed;         /* Philox key of the env (DeviceVirtualTB.seed)                                   */
} cirs_vtb_rollout_cfg;

typedef struct cirs_vtb_policy_layer { /* one post-norm TransformerEncoderLayer, matrices stored [in][out] */
    const float *in_w, *in_b;     /* [D][3D], [3D] (q | k | v)  */
    const float *out_w, *out_b;   /* [D][D], [D]                */
    const float *lin1_w, *lin1_b; /* [D][d_hid], [d_hid]        */
    const float *lin2_w, *lin2_b; /* [d_hid][D], [D]            */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} cirs_vtb_policy_layer;

typedef struct cirs_vtb_policy_weights { /* fp32, matrices stored [in][out] */
    const float *user_w, *user_b;   /* ffn_user [88][D], [D]                                  */
    const float *gate_w, *gate_b;   /* fnn_gate [1 + 27][D] (row 0: reward), [D]              */
    const float* pe;                /* [max_len][D]                                           */
    cirs_vtb_policy_layer layer[CIRS_VTB_RO_MAX_LAYERS];
    const float *dec_w, *dec_b;     /* [D][dim_state], [dim_state]                            */
    const float* trunk_w[CIRS_VTB_RO_MAX_HIDDEN]; /* Net: [in][hidden[i]] (ReLU after each)   */
    const float* trunk_b[CIRS_VTB_RO_MAX_HIDDEN];
    const float *mu_w, *mu_b;       /* [hidden[n-1]][27], [27]                                */
    const float *sigma_w, *sigma_b; /* conditioned_sigma: [hidden[n-1]][27], [27]; else NULL  */
    const float* sigma_param;       /* [27] (not conditioned)                                 */
    const float *act_low, *act_high; /* [27] action box (action_scaling)                      */
} cirs_vtb_policy_weights;

typedef struct cirs_vtb_traj { /* device buffers owned by the caller; t = vector step, e = env id */
    float* state;       /* [max_turn + 1][n_env][dim_state] tracker state of every visited position     */
    float* act;         /* [max_turn][n_env][27] raw action (what the buffer stores)                     */
    float* act_mapped;  /* [max_turn][n_env][27] the action the env received                              */
    double* obs0;       /* [n_env][91] reset observations                                                */
    double* obs;        /* [max_turn][n_env][30] observation of step t, as the env returns it            */
    double* rew;        /* [max_turn][n_env]                                                             */
    uint8_t* done;      /* [max_turn][n_env] after force_length                                          */
    double* ctr;        /* [max_turn][n_env]                                                             */
    int32_t* len;       /* [n_env] episode lengths                                                       */
    /* scratch */
    float* kcache;      /* [nlayers][n_env][max_len][D] */
    float* vcache;      /* [nlayers][n_env][max_len][D] */
    int32_t* lists;     /* [max_turn + 1][n_env] active env ids per step                                 */
    int32_t* counts;    /* [max_turn + 1]                                                                */
    float* act_buf;     /* [n_env][27] mapped actions of the current step, in list order                 */
    double* step_obs;   /* [n_env][30] */
    double* step_rew;   /* [n_env] */
    double* step_ctr;   /* [n_env] */
    uint8_t* step_done; /* [n_env] */
} cirs_vtb_traj;

/* One collect of n_env whole episodes on `stream`, no host synchronisation: vtb_reset of every env, then per vector step the policy
 * kernel (record the previous step, input slot, decode, actor, mapped action, compaction of the active ids) and vtb_step over the
 * envs still active; finished envs are dropped, not reset.  The Gaussian noise of (env, t, dim) is keyed by (seed, collect_id). */
int cirs_vtb_rollout_collect(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* pw, const cirs_vtb_cfg* vtb_cfg,
                             const cirs_vtb_weights* vtb_w, cirs_vtb_state* vtb_st, cirs_vtb_traj* traj, uint64_t seed,
                             uint32_t collect_id, void* stream);
/* Either collect with the MEAN action of a policy built with deterministic_eval and put in eval() (reference core/policy/ppo.py:152-153:
 * act = logits[0] for a continuous actor): act = mu, no Gaussian draw; mapping, clipping, compaction and the trajectory as in the sampled collect.
 * redraw_ws == NULL: the position-keyed collect (cirs_vtb_rollout_collect); non-NULL: the exact-redraw collect (cirs_vtb_rollout_collect_redraw).
 * The tracker's dropout is untouched (it stays in train() during tests): an evaluation is deterministic given model.dropout_seed. */
int cirs_vtb_rollout_collect_greedy(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* pw, const cirs_vtb_cfg* vtb_cfg,
                                    const cirs_vtb_weights* vtb_w, cirs_vtb_state* vtb_st, cirs_vtb_traj* traj, float* redraw_ws, void* stream);

/* cirs_vtb_rollout_collect with the reference's own dropout procedure (core/state_tracker.py:170-250: the tracker stays in train(), every
 * build_state call runs the whole prefix through the encoder again and nn.Dropout draws fresh masks over it).  Call c of env e (c = 0 on
 * the reset observation, c = len_e after the last step) is ONE causal pass over the input slots 0..c with masks of its own at all five
 * sites, those of dropout env id drop_env_base + c * n_env + e (cirs_vtb_rollout_masks with env0 = c * n_env, n_pos = c + 1), and hands
 * out the state of position c.  Call 0 has the position-keyed key: state[0] is the same in both modes, bit for bit.  One workgroup per
 * env per vector step; K/V of the prefix are rebuilt at every call.  model.dropout_p == 0 runs cirs_vtb_rollout_collect's own launches.
 * redraw_ws: max_len * n_env * dim_model * nlayers floats of scratch.  Refused: drop_env_base + (max_turn + 1) * n_env >= 2^31,
 * nhead * max_len > 1088. */
int cirs_vtb_rollout_collect_redraw(const cirs_vtb_rollout_cfg* cfg, const cirs_vtb_policy_weights* pw, const cirs_vtb_cfg* vtb_cfg,
                                    const cirs_vtb_weights* vtb_w, cirs_vtb_state* vtb_st, cirs_vtb_traj* traj, float* redraw_ws,
                                    uint64_t seed, uint32_t collect_id, void* stream);
/* the standard normals z the policy kernel draws for (env_ids[j], ts[j], dim 0..dims-1): out [n][dims] fp32, bit for bit.
 * Box-Muller on Philox (counter (dim / 4, env, t, collect_id), key seed ^ 'GAUS'): the words (w0, w1) give dims 4b, 4b+1, (w2, w3)
 * dims 4b+2, 4b+3; u = u01_from_bits(w); z = sqrt(-2 det_logf(u1)) * {cos, sin}(2 pi u2) with fixed polynomials. */
int cirs_vtb_rollout_noise(uint64_t seed, uint32_t collect_id, const int32_t* env_ids, const int32_t* ts, int32_t n, int32_t dims,
                           float* out, void* stream);
/* keep masks of dropout envs env0..env0+n_env-1, positions pos0..pos0+n_pos-1, (layer, site), elements 0..n_elem-1:
 * out [n_env][n_pos][n_elem] = keep ? 1 / (1 - p) : 0 (csrc/rng.h dropout_keep; ATTN element = key_pos * nhead + head). */
int cirs_vtb_rollout_masks(uint64_t dropout_seed, float p, int32_t env0, int32_t n_env, int32_t pos0, int32_t n_pos, int32_t layer,
                           int32_t site, int32_t n_elem, float* out, void* stream);

/* ---- VirtualTaobao PPO update on the device (csrc/vtb_learn.hip) ---------------------------------------------------------
 * Replaces HostPPOPolicy.update (core/host_rl.py: _returns_stage, process_fn, learn) over a buffer of one device collect, with the
 * tracker gradient through the teacher-forced causal pass of cirs_hip/vtb_host.py tracker_states (reference core/state_tracker.py:
 * 129-250, core/policy/ppo.py:96-246, tianshou/policy/base.py:219-244, modelfree/a2c.py:80-109).
 * Parameter images are fp32 in torch's own layout ([out][in] row-major), in module registration order:
 *   tracker: ffn_user W b | fnn_gate W b | per layer: in_proj W b, out_proj W b, linear1 W b, linear2 W b, norm1 w b, norm2 w b |
 *            decoder W b
 *   policy:  trunk (Net) W b per hidden layer | mu W b | sigma W b (conditioned) or sigma_param [27] | critic W [width] b [1]
 * Adam moments have the layout of their image.  The trunk is the first part of the policy image: it is listed twice in the policy
 * optimiser (actor + critic share the Net), so its squared norm counts twice, the clip coefficient is applied twice and it takes two
 * Adam sub-steps per minibatch. */
typedef struct cirs_vtb_learn_cfg {
    int32_t n_env, max_turn;                     /* the collect's shape (trajectory [max_turn][n_env])                      */
    cirs_vtb_model_cfg model;                    /* with the dropout key of the collect the rows come from                  */
    int32_t n_rows, n_seg;                       /* sampled rows, GAE segments of the sample order                           */
    int32_t scale_returns, whiten_adv, clip_value, has_dual, has_max_norm;
    float clip, dual, c_value, c_entropy, max_norm;
    double discount, lam, floor;
    float lr, beta1, beta2, eps;                 /* policy Adam                                                              */
    float t_lr, t_beta1, t_beta2, t_eps;         /* tracker Adam                                                             */
} cirs_vtb_learn_cfg;

typedef struct cirs_vtb_learn_bufs {
    float* tparams; float* t_m; float* t_v;      /* tracker image + Adam moments                                             */
    float* pparams; float* p_m; float* p_v;      /* policy image + Adam moments                                              */
    const float* pe;                             /* [max_len][D] positional encoding                                         */
    const double* obs0;                          /* the rollout's trajectory: [n_env][91]                                    */
    const double* obs;                           /* [max_turn][n_env][30]                                                    */
    const double* rew;                           /* [max_turn][n_env]                                                        */
    const uint8_t* done;                         /* [max_turn][n_env]                                                        */
    const float* act;                            /* [max_turn][n_env][27] raw actions                                        */
    const int32_t* len;                          /* [n_env]                                                                  */
    const int32_t* rows;                         /* [2][n_rows]: t, env of each sampled row                                  */
    const uint8_t* boundary;                     /* [n_rows] done | unfinished                                               */
    const int32_t* seg_end;                      /* [n_seg] exclusive ends of the GAE segments                               */
    const int32_t* grad_rows;                    /* [n_rows] sample positions sorted by (env, t)                             */
    const int32_t* grad_start;                   /* [n_env * max_turn + 1] CSR starts into grad_rows                          */
    double* rms;                                 /* [3] running return mean, var, count (merged on the device)              */
    float* ws;                                   /* workspace of cirs_vtb_learn_sizes()[2] floats                           */
    float* losses;                               /* [n_minibatches][4] loss, clip, vf, ent                                   */
} cirs_vtb_learn_bufs;

/* out[0] tracker image floats, out[1] policy image floats, out[2] workspace floats, out[3] offset of the states [max_turn + 1]
 * [n_env][dim_state] in the workspace, out[4] offset of the per-row block (v_s, adv, returns, logp_old: [4][n_rows]). */
int cirs_vtb_learn_sizes(const cirs_vtb_learn_cfg* cfg, int64_t* out);
/* Returns stage (HostPPOPolicy._returns_stage + process_fn): the teacher-forced tracker forward over every episode (states and the
 * saved activations), critic values of obs / obs_next, GAE per segment in fp64, returns on the pre-update scale, the block merged
 * into rms, logp_old of the stored actions. */
int cirs_vtb_learn_prepare(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, void* stream);
/* HostPPOPolicy.learn after prepare: `repeat` passes over the rows in the orders perms [repeat][n_rows] (device), minibatches of
 * batch_size rows (a short tail joins the last one); per minibatch the row objective and its gradient, clip_grad_norm_ and Adam on the
 * policy image (step counts continue from p_step0 heads / 2 * p_step0 trunk); recompute_adv reruns the returns stage before every
 * pass after the first; after the last pass the tracker gradient through each row's obs state and one tracker Adam step (t_step0 + 1).
 * No host synchronisation. */
int cirs_vtb_learn_update(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, const int32_t* perms, int32_t repeat,
                          int32_t batch_size, int32_t recompute_adv, int64_t p_step0, int64_t t_step0, void* stream);
/* The same three calls over the buffer of a cirs_vtb_rollout_collect_redraw (reference core/state_tracker.py:170-250 with
 * core/policy/ppo.py:96-246: every build_state call keeps a graph of its own).  Row (t, e) has obs = the state of call t and obs_next =
 * the state of call t + 1; the tracker gradient is the sum over the sampled rows of dL/d obs pushed through that call's own pass
 * (positions 0..t of env e, masks of dropout env id drop_env_base + t * n_env + e, gradient on the last position only).  Each tracker
 * workgroup runs forward and backward of its calls one after the other in one episode workspace and adds into one gradient slab, in a
 * fixed order; min(8, 1024 / n_env) (at least 1) workgroups per env, so the workspace (sizes out[2]) does not grow with the number of
 * calls.  Everything else is cirs_vtb_learn_*'s.  model.dropout_p == 0 runs those calls' own launches.  Refused:
 * drop_env_base + (max_turn + 1) * n_env >= 2^31. */
int cirs_vtb_learn_redraw_sizes(const cirs_vtb_learn_cfg* cfg, int64_t* out);
int cirs_vtb_learn_prepare_redraw(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, void* stream);
int cirs_vtb_learn_update_redraw(const cirs_vtb_learn_cfg* cfg, const cirs_vtb_learn_bufs* b, const int32_t* perms, int32_t repeat,
                                 int32_t batch_size, int32_t recompute_adv, int64_t p_step0, int64_t t_step0, void* stream);

/* ---- VirtualTaobao user-model training (csrc/mmoe_train.hip) ---------------------------------------------------------------
 * One optimiser step of UserModel_MMOE.fit_data's inner loop (reference core/user_model.py:150-170, core/user_model_mmoe.py:144-233,
 * CIRS-UserModel-taobao.py:185-191) for the all-dense one-regression-task build cirs_vtb_mmoe_forward accepts:
 *   h1 = relu(W1 x + b1); h2 = relu(W2 h1 + b2); experts = (We h2 + be) as [expert_dim, n_experts]; gate = softmax(Wg h2)
 *   y_pred = (x . w_lin_task + tower . (experts @ gate)) + out_bias
 *   loss = mean((y_pred / (1 + exposure) - y)^2 (y + 1))                                        (loss_taobao)
 *   reg  = l2_linear |linear_model.weight|^2 + l2_all sum over EVERY parameter of |p|^2          (biases, gate and the unused
 *          duplicate linear_model.weight included: add_regularization_weight(self.parameters(), l2_reg_dnn))
 *   (loss + reg).backward(); torch.optim.Adam step (no weight decay, no amsgrad).
 * Shapes: d_in 118, h1 and h2 from {64, 128}, 4 experts of dim 8, one task of logit dim 1; anything else: CIRS_E_UNSUPPORTED.
 * Parameters, gradients and both Adam moments are flat fp32 buffers of cirs_mmoe_train_param_count(cfg) floats (16-byte aligned) in
 * the order  dnn.linears.1.weight [h2,h1] | expert_network.weight [32,h2] | gating_networks.0.weight [4,h2]
 *          | dnn.linears.0.weight TRANSPOSED [118,h1] | dnn.linears.0.bias [h1] | dnn.linears.1.bias [h2] | expert_network.bias [32]
 *          | tower_network.0.weight [8] | linear_model.weight [118] | linear_model_task.0.weight [118] | out.0.bias [1].
 * Two launches per step, every sum in a fixed order (no float atomics): two runs from one state give identical bits. */
typedef struct cirs_mmoe_train_cfg {
    int32_t d_in, h1, h2, n_experts, expert_dim, n_tasks, task_dim;
    float l2_linear, l2_all;      /* the two regularisation lists of the reference (linear_model, all parameters)  */
    float lr, beta1, beta2, eps;  /* torch.optim.Adam                                                              */
} cirs_mmoe_train_cfg;
int64_t cirs_mmoe_train_param_count(const cirs_mmoe_train_cfg* cfg);               /* 0 for an unsupported shape */
int64_t cirs_mmoe_train_workspace_bytes(const cirs_mmoe_train_cfg* cfg, int32_t n); /* n = rows of the largest batch */
/* one step on the batch x [n,118], y [n], exposure [n] (fp32, device); step_before = optimiser steps taken so far;
 * loss_out[2] = {loss, reg} (device). */
int cirs_mmoe_train_step(const cirs_mmoe_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                         int64_t step_before, const float* x, const float* y, const float* exposure, int32_t n, float* loss_out,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* all steps of one pass: the data set x [n_rows,118], y [n_rows], exposure [n_rows] stays on the device, batch b is the rows
 * order[b * batch_size .. min(n_order, (b + 1) * batch_size)) (int64, device, every entry in [0, n_rows); the last batch may be
 * short, as in DataLoader).  losses_out [ceil(n_order / batch_size)][2] = per-step {loss, reg} (device).  The launches are queued
 * back to back: no host synchronisation, no host round trip between steps.  Bit-identical to the same steps issued through
 * cirs_mmoe_train_step.  workspace: cirs_mmoe_train_workspace_bytes(cfg, min(batch_size, n_order)). */
int cirs_mmoe_train_epoch(const cirs_mmoe_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                          int64_t step_before, const float* x, const float* y, const float* exposure, int64_t n_rows,
                          const int64_t* order, int64_t n_order, int32_t batch_size, float* losses_out, void* workspace,
                          int64_t workspace_bytes, void* stream);
/* compute_exposure_effect_virtualTaobao (CIRS-UserModel-taobao.py:52-70).  Rows are in log order; a row whose timestamp is 1 opens a
 * session: exposure_out[r] = sum_{j in [start(r), r)} exp(-(r - j) ||a_r - a_j||_2 / tau) in float64, 0 for a session's first row and
 * for tau <= 0.  timestamp_host [n_rows] int32 in HOST memory (the session starts are found and checked on the host: a log whose
 * first row does not open a session is refused, the reference would read an undefined `start` there); action [n_rows,27] float64,
 * start_scratch [n_rows] int64 and exposure_out [n_rows] float64 on the device. */
int cirs_vtb_exposure_history(const int32_t* timestamp_host, const double* action, int64_t n_rows, double tau,
                              int64_t* start_scratch, double* exposure_out, void* stream);

/* ---- VirtualTaobao static baselines: training (csrc/mlp_train.hip) ----------------------------------------------------------
 * One optimiser step of UserModel_MMOE.fit_data's inner loop (reference core/user_model.py:150-170, core/user_model_mmoe.py:144-233,
 * loss_taobao of MLP-taobao.py:137-155; the same lines serve MLP-epsilonGreedy-taobao.py) for the all-dense build with the two
 * regression tasks feat_item (27) and y (1) -- the model cirs_vtb_static_eval plays, any shape cirs_vtb_mmoe_shape describes:
 *   h = relu(W_l h + b_l), l < n_dnn; experts = (We h + be) as [expert_dim, experts]; gate_t = softmax(Wg_t h)
 *   pred[:, :27] = tower_0 (experts @ gate_0) + out_0;  pred[:, 27] = (x . w_lin_task + tower_1 (experts @ gate_1)) + out_1
 *   click = y[:, 27];  loss = mean over n * 27 of (click (pred[:, :27] - y[:, :27]))^2 + mean over n of (pred[:, 27] - click)^2
 *   reg  = l2_linear |linear_model.weight|^2 + l2_all sum over EVERY parameter of |p|^2  (biases, both gates and the unused
 *          duplicate linear_model.weight included)
 *   (loss + reg).backward(); torch.optim.Adam step (no weight decay, no amsgrad).
 * Shapes: d_in 91, 1..3 hidden layers of 1..256, experts * expert_dim <= 64, tasks (27, 1); anything else: CIRS_E_UNSUPPORTED.
 * Parameters, gradients and both Adam moments are flat fp32 buffers of cirs_mlp_train_param_count(cfg) floats (16-byte aligned) in
 * the order (H_l = hidden[l], L = n_dnn, E = experts, D = expert_dim; torch layouts unless said otherwise)
 *     dnn.linears.l.weight [H_l,H_(l-1)] for l = 1 .. L-1
 *   | expert_network.weight [E D,H_(L-1)] | gating_networks.0.weight [E,H_(L-1)] | gating_networks.1.weight [E,H_(L-1)]
 *   | dnn.linears.0.weight TRANSPOSED [91,H_0] | dnn.linears.l.bias [H_l] for l = 0 .. L-1 | expert_network.bias [E D]
 *   | tower_network.0.weight [27,D] | tower_network.1.weight [1,D] | out.0.bias [27] | out.1.bias [1]
 *   | linear_model.weight [91] | linear_model_task.1.weight [91].
 * Two launches per step, every sum in a fixed order (no float atomics): two runs from one state give identical bits. */
typedef struct cirs_mlp_train_cfg {
    cirs_vtb_mmoe_shape shape;
    float l2_linear, l2_all;      /* the two regularisation lists of the reference (linear_model, all parameters)  */
    float lr, beta1, beta2, eps;  /* torch.optim.Adam                                                              */
} cirs_mlp_train_cfg;
int64_t cirs_mlp_train_param_count(const cirs_mlp_train_cfg* cfg);               /* 0 for an unsupported shape */
int64_t cirs_mlp_train_workspace_bytes(const cirs_mlp_train_cfg* cfg, int32_t n); /* n = rows of the largest batch */
/* one step on the batch x [n,91], y [n,28] = [27 item features | click] (fp32, device); step_before = optimiser steps taken so
 * far; loss_out[2] = {loss, reg} (device). */
int cirs_mlp_train_step(const cirs_mlp_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                        int64_t step_before, const float* x, const float* y, int32_t n, float* loss_out, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* all steps of one pass: the data set x [n_rows,91], y [n_rows,28] stays on the device, batch b is the rows
 * order[b * batch_size .. min(n_order, (b + 1) * batch_size)) (int64, device, every entry in [0, n_rows); the last batch may be
 * short, as in DataLoader).  losses_out [ceil(n_order / batch_size)][2] = per-step {loss, reg} (device).  The launches are queued
 * back to back: no host synchronisation between steps.  Bit-identical to the same steps issued through cirs_mlp_train_step.
 * workspace: cirs_mlp_train_workspace_bytes(cfg, min(batch_size, n_order)). */
int cirs_mlp_train_epoch(const cirs_mlp_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                         int64_t step_before, const float* x, const float* y, int64_t n_rows, const int64_t* order,
                         int64_t n_order, int32_t batch_size, float* losses_out, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ranking and list-diversity metrics of top-k lists (csrc/rankmetrics.hip).  No reference counterpart: the reference has the
 * interactive metrics only (evaluation.py); the ground truth here is the fully observed user x item matrix of KuaishouEnv.
 * ---------------------------------------------------------------------------------------------------------- */
/* The k (1..CIRS_TOPK_MAX) best entries of every row of a row-major fp32 score table scores [n, ld], ld >= n_items: value
 * descending, ties -> the lower id first (the strict total order of cirs_actor_topk, the same selection loop).  Entries that are
 * -inf, NaN or masked are never listed.  visited (nullable): uint32 bitmap, bit i of row env_ids[j] (NULL = j) masks item i of
 * row j, (n_items + 31) / 32 words per row, as in cirs_actor_topk (env_ids are trusted as there); skip[j] != 0 (nullable): the
 * row is all fill.  ids_out [n, k] i64, vals_out [n, k] f32 (nullable): the table's own bits; fills are -1 / -inf. */
int cirs_rows_topk(const float* scores, int32_t n, int32_t n_items, int64_t ld, int32_t k, const int32_t* env_ids,
                   const uint32_t* visited, const uint8_t* skip, int64_t* ids_out, float* vals_out, void* stream);

#define CIRS_RANK_NCOL 11 /* n_list, n_rel, hits, precision, recall, hit, mrr, dcg, idcg, ndcg, ild */
#define CIRS_RANK_NSUM 8  /* evaluated rows, error word, mean precision, recall, hit, mrr, ndcg, ild */
#define CIRS_RANK_ERR_ID 1   /* a list id outside [-1, n_items) */
#define CIRS_RANK_ERR_USER 2 /* a user outside [0, n_users)     */
typedef struct cirs_rank_cfg {
    int32_t n_users, n_items; /* rows / used columns of rel */
    int32_t k;                /* 1..CIRS_TOPK_MAX list positions scored */
    int32_t reserved;
    double rel_threshold;     /* an item is relevant iff rel >= rel_threshold */
    double discount[CIRS_TOPK_MAX]; /* 1 / log2(r + 2), computed by the caller: the device takes no logarithm */
} cirs_rank_cfg;
/* Scores n lists against a relevance table.  ids [n, ld_ids] i64 (columns 0..k-1 used, -1 = fill, ld_ids >= k), users [n] i32 =
 * the row of rel f64 [n_users, ld_rel] (ld_rel >= n_items), item_cats [n_items] packed categories (cirs_env_tables.item_cats);
 * visited / env_ids / skip as in cirs_rows_topk: masked items leave n_rel and the ideal list (a list is scored as it stands: it is
 * expected to come from a selection under the same mask).  per_row f64 [n, CIRS_RANK_NCOL]:
 *   n_list = ids >= 0 | n_rel = unmasked items with rel >= rel_threshold | hits = listed items with rel >= rel_threshold
 *   precision = hits / k | recall = hits / n_rel (0 if n_rel = 0) | hit = hits > 0 | mrr = 1 / rank of the first hit (from 1; 0 if none)
 *   dcg = sum over positions r = 0..k-1, in that order, of gain(rel[u, id_r]) * discount[r], gain(x) = x > 0 ? x : 0 (fills add nothing)
 *   idcg = the same sum over the k largest gains of the unmasked items in descending order | ndcg = dcg / idcg (0 if idcg = 0)
 *   ild = 1 - mean Jaccard similarity popc(a & b) / popc(a | b) of the category masks over the pairs of listed items (empty union:
 *         0; fewer than two items: ild = 0); summed per first item a over b = a+1.. ascending, the partial sums then added in ascending a.
 * A skipped row is all zero.  An id outside [-1, n_items) or a user outside [0, n_users) is never used as an index: the row is all
 * zero and its CIRS_RANK_ERR_* bits are or-ed into the error word.  sums f64 [CIRS_RANK_NSUM] = {rows not skipped, error word, means
 * of precision, recall, hit, mrr, ndcg, ild over the rows not skipped (0 if there is none)}: a second launch of one 256-thread
 * workgroup, thread t adds rows t, t + 256, ... in ascending order, then a halving tree over the 256 partials (no float atomics).
 * Lists are assumed duplicate-free.  workspace: cirs_rank_metrics_workspace_bytes(n) (0 for n <= 0). */
int64_t cirs_rank_metrics_workspace_bytes(int32_t n);
int cirs_rank_metrics(const cirs_rank_cfg* cfg, const int64_t* ids, int64_t ld_ids, const int32_t* users, int32_t n, const double* rel,
                      int64_t ld_rel, const uint32_t* item_cats, const int32_t* env_ids, const uint32_t* visited, const uint8_t* skip,
                      double* per_row, double* sums, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIRS_HIP_H */
