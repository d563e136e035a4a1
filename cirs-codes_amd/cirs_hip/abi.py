"""ctypes mirror of include/cirs_hip.h and the loader of libcirs_hip.so.

The HIP library is the product: there is NO CPU fallback.  `lib()` raises if the shared object is missing or
does not export every symbol the header declares.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CIRS_HIP_LIB: an explicit path to another build of the library (same-box A/B runs of tools/ab_step_libs.py, tests against a probe build); default: the in-tree build
LIB_PATH = os.environ.get("CIRS_HIP_LIB") or os.path.join(_HERE, "libcirs_hip.so")

c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_u8p = C.POINTER(C.c_uint8)
c_u32p = C.POINTER(C.c_uint32)
c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)


class EnvCfg(C.Structure):
    _fields_ = [("n_users", C.c_int32), ("n_items", C.c_int32), ("max_turn", C.c_int32),
                ("num_leave_compute", C.c_int32), ("leave_threshold", C.c_int32), ("version", C.c_int32),
                ("use_exposure", C.c_int32), ("has_ab", C.c_int32), ("dist_mode", C.c_int32),
                ("simulated", C.c_int32), ("tau", C.c_double), ("gamma_exposure", C.c_double),
                ("r_decay", C.c_double)]


class EnvTables(C.Structure):
    _fields_ = [("mat", C.c_void_p), ("normed_mat", C.c_void_p), ("dist", C.c_void_p),
                ("item_cats", C.c_void_p), ("alpha_env", C.c_void_p), ("beta_env", C.c_void_p),
                ("pred_online", C.c_void_p), ("pred_minmax", C.c_void_p)]


class EnvState(C.Structure):
    _fields_ = [("user", C.c_void_p), ("turn", C.c_void_p), ("done", C.c_void_p),
                ("hist_action", C.c_void_p), ("cum_reward", C.c_void_p)]


MAX_TRACKER_LAYERS = 4


class TrackerCfg(C.Structure):
    _fields_ = [("n_users", C.c_int32), ("n_items", C.c_int32), ("dim_model", C.c_int32), ("dim_state", C.c_int32),
                ("nhead", C.c_int32), ("d_hid", C.c_int32), ("nlayers", C.c_int32), ("max_len", C.c_int32),
                ("n_env", C.c_int32), ("dropout_p", C.c_float), ("drop_env_base", C.c_int32), ("dropout_seed", C.c_uint64)]


class TrackerLayer(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "lin1_w", "lin1_b",
                                          "lin2_w", "lin2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")]


class TrackerWeights(C.Structure):
    _fields_ = [("emb_user", C.c_void_p), ("emb_item", C.c_void_p), ("ffn_user_w", C.c_void_p),
                ("ffn_user_b", C.c_void_p), ("gate_w", C.c_void_p), ("gate_b", C.c_void_p), ("pe", C.c_void_p),
                ("layer", TrackerLayer * MAX_TRACKER_LAYERS), ("dec_w", C.c_void_p), ("dec_b", C.c_void_p)]


class TrackerState(C.Structure):
    _fields_ = [("x_hist", C.c_void_p), ("kcache", C.c_void_p), ("vcache", C.c_void_p), ("len", C.c_void_p)]


GRU_MAX_LAYERS = 2


class GruCfg(C.Structure):          # cirs_gru_cfg
    _fields_ = [("n_users", C.c_int32), ("n_items", C.c_int32), ("dim_model", C.c_int32), ("dim_state", C.c_int32),
                ("nlayers", C.c_int32), ("max_len", C.c_int32), ("n_env", C.c_int32)]


class GruLayer(C.Structure):        # cirs_gru_layer / cirs_gru_layer_grads
    _fields_ = [(k, C.c_void_p) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]


class GruWeights(C.Structure):      # cirs_gru_weights / cirs_gru_grads (same layout)
    _fields_ = [("emb_user", C.c_void_p), ("emb_item", C.c_void_p), ("ffn_user_w", C.c_void_p), ("ffn_user_b", C.c_void_p),
                ("gate_w", C.c_void_p), ("gate_b", C.c_void_p), ("layer", GruLayer * GRU_MAX_LAYERS), ("dec_w", C.c_void_p),
                ("dec_b", C.c_void_p)]


class GruState(C.Structure):        # cirs_gru_state
    _fields_ = [("x_hist", C.c_void_p), ("h", C.c_void_p), ("len", C.c_void_p)]


LSTM_MAX_LAYERS = 2


class LstmCfg(C.Structure):         # cirs_lstm_cfg
    _fields_ = list(GruCfg._fields_)


class LstmLayer(C.Structure):       # cirs_lstm_layer / cirs_lstm_layer_grads
    _fields_ = [(k, C.c_void_p) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]


class LstmWeights(C.Structure):     # cirs_lstm_weights / cirs_lstm_grads (same layout)
    _fields_ = [("emb_user", C.c_void_p), ("emb_item", C.c_void_p), ("ffn_user_w", C.c_void_p), ("ffn_user_b", C.c_void_p),
                ("gate_w", C.c_void_p), ("gate_b", C.c_void_p), ("layer", LstmLayer * LSTM_MAX_LAYERS), ("dec_w", C.c_void_p),
                ("dec_b", C.c_void_p)]


class LstmState(C.Structure):       # cirs_lstm_state
    _fields_ = [("x_hist", C.c_void_p), ("h", C.c_void_p), ("c", C.c_void_p), ("len", C.c_void_p)]


class AvgCfg(C.Structure):          # cirs_avg_cfg
    _fields_ = [("n_users", C.c_int32), ("n_items", C.c_int32), ("dim_model", C.c_int32), ("dim_state", C.c_int32),
                ("window", C.c_int32), ("max_len", C.c_int32), ("n_env", C.c_int32)]


class AvgWeights(C.Structure):      # cirs_avg_weights / cirs_avg_grads (same layout)
    _fields_ = [(k, C.c_void_p) for k in ("emb_user", "emb_item", "ffn_user_w", "ffn_user_b", "gate_w", "gate_b", "dec_w", "dec_b")]


class AvgState(C.Structure):        # cirs_avg_state
    _fields_ = [("x_hist", C.c_void_p), ("len", C.c_void_p)]


CASER_MAX_HEIGHTS = 4


class CaserCfg(C.Structure):        # cirs_caser_cfg
    _fields_ = list(AvgCfg._fields_) + [("n_heights", C.c_int32), ("heights", C.c_int32 * CASER_MAX_HEIGHTS)]


class CaserWeights(C.Structure):    # cirs_caser_weights / cirs_caser_grads (same layout)
    _fields_ = ([(k, C.c_void_p) for k in ("emb_user", "emb_item", "ffn_user_w", "ffn_user_b", "gate_w", "gate_b")] +
                [("conv_w", C.c_void_p * CASER_MAX_HEIGHTS), ("conv_b", C.c_void_p * CASER_MAX_HEIGHTS)] +
                [(k, C.c_void_p) for k in ("vert_w", "vert_b", "fc_w", "fc_b", "dec_w", "dec_b")])


class CaserState(C.Structure):      # cirs_caser_state
    _fields_ = [("x_hist", C.c_void_p), ("len", C.c_void_p)]


NEXTITNET_MAX_BLOCKS = 4


class NextItNetCfg(C.Structure):    # cirs_nextitnet_cfg
    _fields_ = [("n_users", C.c_int32), ("n_items", C.c_int32), ("dim_model", C.c_int32), ("dim_state", C.c_int32), ("n_blocks", C.c_int32),
                ("max_len", C.c_int32), ("n_env", C.c_int32), ("dilations", C.c_int32 * NEXTITNET_MAX_BLOCKS)]


class NextItNetWeights(C.Structure):    # cirs_nextitnet_weights / cirs_nextitnet_grads (same layout)
    _fields_ = ([(k, C.c_void_p) for k in ("emb_user", "emb_item", "ffn_user_w", "ffn_user_b", "gate_w", "gate_b")] +
                [(k, C.c_void_p * NEXTITNET_MAX_BLOCKS) for k in ("conv_w", "conv_b", "ln_w", "ln_b")] +
                [(k, C.c_void_p) for k in ("dec_w", "dec_b")])


class NextItNetState(C.Structure):  # cirs_nextitnet_state
    _fields_ = [("x_hist", C.c_void_p), ("len", C.c_void_p)]


STAMP_MAX_WINDOW = 16


class StampCfg(C.Structure):        # cirs_stamp_cfg
    _fields_ = list(AvgCfg._fields_)


class StampWeights(C.Structure):    # cirs_stamp_weights / cirs_stamp_grads (same layout)
    _fields_ = [(k, C.c_void_p) for k in ("emb_user", "emb_item", "ffn_user_w", "ffn_user_b", "gate_w", "gate_b", "attn_b", "w1", "w2", "w3", "w0",
                                          "mlp_a_w", "mlp_a_b", "mlp_b_w", "mlp_b_b", "dec_w", "dec_b")]


class StampState(C.Structure):      # cirs_stamp_state
    _fields_ = [("x_hist", C.c_void_p), ("len", C.c_void_p)]


NARM_MAX_LAYERS = 1


class NarmCfg(C.Structure):         # cirs_narm_cfg
    _fields_ = list(GruCfg._fields_)


class NarmWeights(C.Structure):     # cirs_narm_weights / cirs_narm_grads (same layout)
    _fields_ = [(k, C.c_void_p) for k in ("emb_user", "emb_item", "ffn_user_w", "ffn_user_b", "gate_w", "gate_b", "w_ih", "w_hh", "b_ih", "b_hh",
                                          "a1", "a2", "v", "bw", "dec_w", "dec_b")]


class NarmState(C.Structure):       # cirs_narm_state
    _fields_ = [("x_hist", C.c_void_p), ("h", C.c_void_p), ("h_hist", C.c_void_p), ("q_hist", C.c_void_p), ("len", C.c_void_p)]


FMLP_MAX_WINDOW, FMLP_MAX_LAYERS, FMLP_HIDDEN = 16, 2, 128
FMLP_LAYER_MEMBERS = ("cw", "fln_w", "fln_b", "d1_w", "d1_b", "d2_w", "d2_b", "ln_w", "ln_b")


class FmlpCfg(C.Structure):         # cirs_fmlp_cfg
    _fields_ = [("n_users", C.c_int32), ("n_items", C.c_int32), ("dim_model", C.c_int32), ("dim_state", C.c_int32),
                ("window", C.c_int32), ("nlayers", C.c_int32), ("max_len", C.c_int32), ("n_env", C.c_int32)]


class FmlpWeights(C.Structure):     # cirs_fmlp_weights / cirs_fmlp_grads (same layout): every layer member is an array over the layers
    _fields_ = ([(k, C.c_void_p) for k in ("emb_user", "emb_item", "ffn_user_w", "ffn_user_b", "gate_w", "gate_b")] +
                [(k, C.c_void_p * FMLP_MAX_LAYERS) for k in FMLP_LAYER_MEMBERS] + [("dec_w", C.c_void_p), ("dec_b", C.c_void_p)])


class FmlpState(C.Structure):       # cirs_fmlp_state
    _fields_ = [("x_hist", C.c_void_p), ("len", C.c_void_p)]


LRU_MAX_LAYERS, LRU_HIDDEN = 1, 128
LRU_MEMBERS = ("nu_log", "theta_log", "gamma_log", "in_w", "in_b", "out_w", "out_b", "lln_w", "lln_b", "d1_w", "d1_b", "d2_w", "d2_b", "ln_w", "ln_b")


class LruCfg(C.Structure):          # cirs_lru_cfg
    _fields_ = list(GruCfg._fields_)


class LruWeights(C.Structure):      # cirs_lru_weights / cirs_lru_grads (same layout)
    _fields_ = [(k, C.c_void_p) for k in ("emb_user", "emb_item", "ffn_user_w", "ffn_user_b", "gate_w", "gate_b") + LRU_MEMBERS + ("dec_w", "dec_b")]


class LruState(C.Structure):        # cirs_lru_state
    _fields_ = [("x_hist", C.c_void_p), ("h_re", C.c_void_p), ("h_im", C.c_void_p), ("len", C.c_void_p)]


class PolicyCfg(C.Structure):
    _fields_ = [("n_items", C.c_int32), ("dim_state", C.c_int32), ("hidden", C.c_int32)]


class PolicyWeights(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc")]


class PpoCfg(C.Structure):
    _fields_ = [("n_items", C.c_int32), ("dim_state", C.c_int32), ("hidden", C.c_int32), ("norm_adv", C.c_int32),
                ("value_clip", C.c_int32), ("rew_norm", C.c_int32), ("gamma", C.c_float), ("gae_lambda", C.c_float),
                ("eps_clip", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("max_grad_norm", C.c_float),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float), ("dual_clip", C.c_float)]


class PpoBatch(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs", "act", "adv", "ret", "v_s", "logp_old", "row_env", "row_t")]


class DeepFMCfg(C.Structure):
    _fields_ = [("n_user_vocab", C.c_int32), ("n_item_vocab", C.c_int32), ("n_feat_vocab", C.c_int32),
                ("emb_dim", C.c_int32), ("hidden", C.c_int32)]


class DiceCfg(C.Structure):
    _fields_ = [("n_user_vocab", C.c_int32), ("n_item_vocab", C.c_int32), ("n_feat_vocab", C.c_int32),
                ("emb_dim", C.c_int32), ("hidden", C.c_int32)]


DEEPFM_FIELDS = ("emb_user", "emb_item", "emb_feat", "lin_user", "lin_item", "lin_feat", "lin_dense", "w1", "b1", "w2", "b2",
                 "last", "out_bias")


class DeepFMWeights(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in DEEPFM_FIELDS]


class OnlineReward(C.Structure):
    _fields_ = [("cfg", C.POINTER(DeepFMCfg)), ("w", C.POINTER(DeepFMWeights))] + [
        (k, C.c_void_p) for k in ("raw_uid", "raw_pid", "item_feats", "item_dur", "pred_minmax", "uid_buf", "pid_buf",
                                  "feat_buf", "dur_buf", "pred_buf")]


class Traj(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs", "act", "rew", "done", "logp", "value", "ctr")]


class Redraw(C.Structure):      # cirs_redraw
    _fields_ = [("row_env", C.c_void_p), ("row_t", C.c_void_p), ("offsets", C.c_void_p), ("lens", C.c_void_p), ("dropout_seed", C.c_uint64),
                ("env_base0", C.c_int64), ("env_stride", C.c_int64), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class VtbCfg(C.Structure):       # cirs_vtb_cfg
    _fields_ = [(k, C.c_int32) for k in ("n_env", "max_turn", "num_leave_compute", "simulated", "version", "use_exposure", "mmoe_d_in",
                                         "mmoe_dnn_layers", "mmoe_h1", "mmoe_h2", "mmoe_experts", "mmoe_expert_dim", "mmoe_tasks",
                                         "mmoe_task_dim")] + [(k, C.c_double) for k in ("leave_threshold", "tau", "gamma_exposure")]


VTB_WEIGHT_FIELDS = ("gen_w1", "gen_b1", "gen_w2", "gen_b2", "act_w1", "act_b1", "act_w2", "act_b2", "act_w3", "act_b3",
                     "mm_w1", "mm_b1", "mm_w2", "mm_b2", "mm_we", "mm_be", "mm_wg", "mm_wt", "mm_wlin", "mm_bias")


class VtbWeights(C.Structure):   # cirs_vtb_weights
    _fields_ = [(k, C.c_void_p) for k in VTB_WEIGHT_FIELDS]


class VtbState(C.Structure):     # cirs_vtb_state
    _fields_ = [(k, C.c_void_p) for k in ("task_user", "sim_user", "turn", "event", "prev_reward", "cum_reward", "lst_action", "hist")]


VTB_STATIC_STATE_DIM, VTB_STATIC_MAX_DNN, VTB_STATIC_NOISE_COLS = 91, 3, 265


def vtb_static_metrics_bytes(n_traj):    # CIRS_VTB_STATIC_METRICS_BYTES
    return 48 + 4 * int(n_traj)


class VtbMmoeShape(C.Structure):     # cirs_vtb_mmoe_shape
    _fields_ = [("d_in", C.c_int32), ("n_dnn", C.c_int32), ("hidden", C.c_int32 * VTB_STATIC_MAX_DNN), ("experts", C.c_int32),
                ("expert_dim", C.c_int32), ("n_tasks", C.c_int32), ("task_dim", C.c_int32 * 2)]


class VtbMmoeWeights(C.Structure):   # cirs_vtb_mmoe_weights
    _fields_ = [("dnn_w", C.c_void_p * VTB_STATIC_MAX_DNN), ("dnn_b", C.c_void_p * VTB_STATIC_MAX_DNN), ("expert_w", C.c_void_p),
                ("expert_b", C.c_void_p), ("gate_w", C.c_void_p * 2), ("tower_w", C.c_void_p * 2), ("lin_w", C.c_void_p),
                ("bias", C.c_void_p * 2)]


class VtbStaticCfg(C.Structure):     # cirs_vtb_static_cfg
    _fields_ = [("n_traj", C.c_int32), ("max_turn", C.c_int32), ("num_leave_compute", C.c_int32), ("reserved", C.c_int32),
                ("leave_threshold", C.c_double), ("epsilon", C.c_double), ("policy", VtbMmoeShape)]


class VtbStaticOut(C.Structure):     # cirs_vtb_static_out
    _fields_ = [(k, C.c_void_p) for k in ("user", "state", "action", "reward_pred", "reward", "done", "explore", "metrics")]


VTB_RO_MAX_LAYERS, VTB_RO_MAX_HIDDEN = 4, 3


class VtbModelCfg(C.Structure):      # cirs_vtb_model_cfg: the one description of the tracker + actor both stages embed
    _fields_ = [(k, C.c_int32) for k in ("dim_model", "nhead", "d_hid", "nlayers", "dim_state", "max_len", "n_hidden")] + \
        [("hidden", C.c_int32 * VTB_RO_MAX_HIDDEN), ("unbounded", C.c_int32), ("conditioned_sigma", C.c_int32), ("max_action", C.c_float),
         ("dropout_p", C.c_float), ("drop_env_base", C.c_int32), ("dropout_seed", C.c_uint64)]


class VtbRolloutCfg(C.Structure):    # cirs_vtb_rollout_cfg
    _fields_ = [(k, C.c_int32) for k in ("n_env", "max_turn", "force_length", "bound_method", "action_scaling")] + \
        [("model", VtbModelCfg), ("env_seed", C.c_uint64)]


VTB_LAYER_FIELDS = ("in_w", "in_b", "out_w", "out_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")


class VtbPolicyLayer(C.Structure):   # cirs_vtb_policy_layer
    _fields_ = [(k, C.c_void_p) for k in VTB_LAYER_FIELDS]


class VtbPolicyWeights(C.Structure):  # cirs_vtb_policy_weights
    _fields_ = [(k, C.c_void_p) for k in ("user_w", "user_b", "gate_w", "gate_b", "pe")] + [("layer", VtbPolicyLayer * VTB_RO_MAX_LAYERS)] + \
        [("dec_w", C.c_void_p), ("dec_b", C.c_void_p), ("trunk_w", C.c_void_p * VTB_RO_MAX_HIDDEN), ("trunk_b", C.c_void_p * VTB_RO_MAX_HIDDEN)] + \
        [(k, C.c_void_p) for k in ("mu_w", "mu_b", "sigma_w", "sigma_b", "sigma_param", "act_low", "act_high")]


VTB_TRAJ_FIELDS = ("state", "act", "act_mapped", "obs0", "obs", "rew", "done", "ctr", "len", "kcache", "vcache", "lists", "counts", "act_buf",
                   "step_obs", "step_rew", "step_ctr", "step_done")


class VtbTraj(C.Structure):          # cirs_vtb_traj
    _fields_ = [(k, C.c_void_p) for k in VTB_TRAJ_FIELDS]


class VtbLearnCfg(C.Structure):      # cirs_vtb_learn_cfg
    _fields_ = [("n_env", C.c_int32), ("max_turn", C.c_int32), ("model", VtbModelCfg)] + \
        [(k, C.c_int32) for k in ("n_rows", "n_seg", "scale_returns", "whiten_adv", "clip_value", "has_dual", "has_max_norm")] + \
        [(k, C.c_float) for k in ("clip", "dual", "c_value", "c_entropy", "max_norm")] + [(k, C.c_double) for k in ("discount", "lam", "floor")] + \
        [(k, C.c_float) for k in ("lr", "beta1", "beta2", "eps", "t_lr", "t_beta1", "t_beta2", "t_eps")]


VTB_LEARN_BUF_FIELDS = ("tparams", "t_m", "t_v", "pparams", "p_m", "p_v", "pe", "obs0", "obs", "rew", "done", "act", "len", "rows", "boundary",
                        "seg_end", "grad_rows", "grad_start", "rms", "ws", "losses")


class VtbLearnBufs(C.Structure):     # cirs_vtb_learn_bufs
    _fields_ = [(k, C.c_void_p) for k in VTB_LEARN_BUF_FIELDS]


class MmoeTrainCfg(C.Structure):    # cirs_mmoe_train_cfg
    _fields_ = [(k, C.c_int32) for k in ("d_in", "h1", "h2", "n_experts", "expert_dim", "n_tasks", "task_dim")] + \
        [(k, C.c_float) for k in ("l2_linear", "l2_all", "lr", "beta1", "beta2", "eps")]


class MlpTrainCfg(C.Structure):     # cirs_mlp_train_cfg
    _fields_ = [("shape", VtbMmoeShape)] + [(k, C.c_float) for k in ("l2_linear", "l2_all", "lr", "beta1", "beta2", "eps")]


TOPK_MAX, RANK_NCOL, RANK_NSUM = 32, 11, 8      # CIRS_TOPK_MAX, CIRS_RANK_NCOL, CIRS_RANK_NSUM
RANK_COLUMNS = ("n_list", "n_rel", "hits", "precision", "recall", "hit", "mrr", "dcg", "idcg", "ndcg", "ild")
RANK_ERR_ID, RANK_ERR_USER = 1, 2


class RankCfg(C.Structure):         # cirs_rank_cfg
    _fields_ = [("n_users", C.c_int32), ("n_items", C.c_int32), ("k", C.c_int32), ("reserved", C.c_int32), ("rel_threshold", C.c_double),
                ("discount", C.c_double * TOPK_MAX)]


# name -> (restype, argtypes).  Must list every symbol include/cirs_hip.h declares (tests check this).
_P = C.c_void_p
SIGNATURES = {
    "cirs_last_error": (C.c_char_p, []),
    "cirs_version": (C.c_int, []),
    "cirs_env_reset": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvState), _P, _P, C.c_int32, _P, _P]),
    "cirs_env_step": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), _P, _P, C.c_int32,
                                _P, _P, _P, _P, _P, _P]),
    "cirs_dist_jaccard": (C.c_int, [_P, C.c_int32, _P, _P]),
    "cirs_vtb_reset": (C.c_int, [C.POINTER(VtbCfg), C.POINTER(VtbWeights), C.POINTER(VtbState), C.c_uint64, _P, C.c_int32, _P, _P]),
    "cirs_vtb_step": (C.c_int, [C.POINTER(VtbCfg), C.POINTER(VtbWeights), C.POINTER(VtbState), C.c_uint64, _P, _P, C.c_int32,
                                _P, _P, _P, _P, _P, _P]),
    "cirs_vtb_noise": (C.c_int, [C.c_uint64, _P, _P, C.c_int32, _P, _P]),
    "cirs_vtb_mmoe_forward": (C.c_int, [C.POINTER(VtbCfg), C.POINTER(VtbWeights), _P, C.c_int32, _P, _P]),
    "cirs_vtb_static_workspace_bytes": (C.c_int64, [C.POINTER(VtbStaticCfg)]),
    "cirs_vtb_static_eval": (C.c_int, [C.POINTER(VtbStaticCfg), C.POINTER(VtbWeights), C.POINTER(VtbMmoeWeights), C.c_uint64,
                                       C.POINTER(VtbStaticOut), _P, C.c_int64, _P]),
    "cirs_vtb_static_noise": (C.c_int, [C.c_uint64, _P, _P, C.c_int32, _P, _P]),
    "cirs_vtb_rollout_collect": (C.c_int, [C.POINTER(VtbRolloutCfg), C.POINTER(VtbPolicyWeights), C.POINTER(VtbCfg), C.POINTER(VtbWeights),
                                           C.POINTER(VtbState), C.POINTER(VtbTraj), C.c_uint64, C.c_uint32, _P]),
    "cirs_vtb_rollout_noise": (C.c_int, [C.c_uint64, C.c_uint32, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "cirs_vtb_rollout_masks": (C.c_int, [C.c_uint64, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         _P, _P]),
    "cirs_vtb_learn_sizes": (C.c_int, [C.POINTER(VtbLearnCfg), _P]),
    "cirs_vtb_learn_prepare": (C.c_int, [C.POINTER(VtbLearnCfg), C.POINTER(VtbLearnBufs), _P]),
    "cirs_vtb_learn_update": (C.c_int, [C.POINTER(VtbLearnCfg), C.POINTER(VtbLearnBufs), _P, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                        C.c_int64, _P]),
    "cirs_vtb_rollout_collect_redraw": (C.c_int, [C.POINTER(VtbRolloutCfg), C.POINTER(VtbPolicyWeights), C.POINTER(VtbCfg),
                                                  C.POINTER(VtbWeights), C.POINTER(VtbState), C.POINTER(VtbTraj), _P, C.c_uint64, C.c_uint32,
                                                  _P]),
    "cirs_vtb_rollout_collect_greedy": (C.c_int, [C.POINTER(VtbRolloutCfg), C.POINTER(VtbPolicyWeights), C.POINTER(VtbCfg),
                                                  C.POINTER(VtbWeights), C.POINTER(VtbState), C.POINTER(VtbTraj), _P, _P]),
    "cirs_vtb_learn_redraw_sizes": (C.c_int, [C.POINTER(VtbLearnCfg), _P]),
    "cirs_vtb_learn_prepare_redraw": (C.c_int, [C.POINTER(VtbLearnCfg), C.POINTER(VtbLearnBufs), _P]),
    "cirs_vtb_learn_update_redraw": (C.c_int, [C.POINTER(VtbLearnCfg), C.POINTER(VtbLearnBufs), _P, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int64, C.c_int64, _P]),
    "cirs_tracker_init": (C.c_int, [C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState), _P, _P,
                                    C.c_int32, _P, C.c_int64, _P]),
    "cirs_tracker_step": (C.c_int, [C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState), _P, _P,
                                    _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_policy_workspace_bytes": (C.c_int64, [C.POINTER(PolicyCfg), C.c_int32]),
    "cirs_actor_sample": (C.c_int, [C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), _P, C.c_int64, C.c_int32, _P,
                                    C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "cirs_actor_greedy": (C.c_int, [C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), _P, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P,
                                    C.c_int64, _P]),
    "cirs_actor_topk_workspace_bytes": (C.c_int64, [C.POINTER(PolicyCfg), C.c_int32, C.c_int32]),
    "cirs_actor_topk": (C.c_int, [C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                  _P, C.c_int64, _P]),
    "cirs_critic_values": (C.c_int, [C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), _P, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_rollout_steps": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState),
                                     C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState),
                                     C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32,
                                     C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_rollout_collect": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState),
                                       C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState),
                                       C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32,
                                       _P, C.c_uint64, C.c_uint32, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_rollout_steps_greedy": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState),
                                            C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState),
                                            C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32,
                                            C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_rollout_collect_greedy": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState),
                                              C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState),
                                              C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32,
                                              _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_rollout_steps_redraw": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState),
                                            C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState),
                                            C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32,
                                            C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.POINTER(Redraw), _P, C.c_int64, _P]),
    "cirs_rollout_steps_noise": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState),
                                           C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState),
                                           C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32,
                                           C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_rollout_steps_online": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState),
                                            C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState),
                                            C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32,
                                            C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, _P, C.c_int32,
                                            C.POINTER(OnlineReward), _P, C.c_int64, _P]),
    "cirs_ppo_param_count": (C.c_int64, [C.POINTER(PpoCfg)]),
    "cirs_ppo_workspace_bytes": (C.c_int64, [C.POINTER(PpoCfg), C.c_int32]),
    "cirs_ppo_prepare_async": (C.c_int, [C.POINTER(PpoCfg), C.POINTER(Traj), _P, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(PpoBatch), _P, _P]),
    "cirs_ppo_prepare_async_perms": (C.c_int, [C.POINTER(PpoCfg), C.POINTER(Traj), _P, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(PpoBatch), _P, C.c_uint64, C.c_uint64, C.c_int32, _P, C.c_int32, _P]),
    "cirs_ppo_prepare": (C.c_int, [C.POINTER(PpoCfg), C.POINTER(Traj), _P, _P, C.c_int32, C.c_int32, C.c_int32, _P,
                                   C.POINTER(PpoBatch), _P]),
    "cirs_ppo_minibatch": (C.c_int, [C.POINTER(PpoCfg), _P, _P, _P, _P, C.c_int64, C.POINTER(PpoBatch), _P, C.c_int32,
                                     _P, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_ppo_minibatch_dp_chain": (C.c_int, [C.POINTER(PpoCfg), _P, _P, _P, _P, C.c_int64, C.POINTER(PpoBatch), _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P,
                                              _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P]),
    "cirs_ppo_learn_steps": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "cirs_ppo_handoff_status": (C.c_int, [_P, C.c_int32, _P]),
    "cirs_ppo_update_readback": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P]),
    "cirs_ppo_learn": (C.c_int, [C.POINTER(PpoCfg), _P, _P, _P, _P, C.c_int64, C.POINTER(PpoBatch), _P, C.c_int32, C.c_int32, C.c_int32,
                                 _P, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(TrackerCfg), C.c_int32]),
    "cirs_tracker_backward": (C.c_int, [C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState), _P, _P,
                                        _P, _P, _P, _P, _P, C.c_int32, _P, C.POINTER(TrackerWeights), _P, C.c_int64, _P]),
    "cirs_tracker_backward_last": (C.c_int, [C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState), _P, _P,
                                             _P, _P, _P, _P, _P, C.c_int32, _P, C.POINTER(TrackerWeights), _P, C.c_int64, _P]),
    "cirs_tracker_prefix_states": (C.c_int, [C.POINTER(TrackerCfg), C.POINTER(TrackerWeights), C.POINTER(TrackerState), _P, _P, _P, _P, C.c_int32, _P,
                                            C.c_int64, _P, C.c_int64, _P]),
    "cirs_gru_tracker_init": (C.c_int, [C.POINTER(GruCfg), C.POINTER(GruWeights), C.POINTER(GruState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_gru_tracker_step": (C.c_int, [C.POINTER(GruCfg), C.POINTER(GruWeights), C.POINTER(GruState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_gru_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(GruCfg), C.c_int32]),
    "cirs_gru_tracker_backward": (C.c_int, [C.POINTER(GruCfg), C.POINTER(GruWeights), C.POINTER(GruState), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                            C.POINTER(GruWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_gru": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(GruCfg), C.POINTER(GruWeights),
                                           C.POINTER(GruState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                           C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_lstm_tracker_init": (C.c_int, [C.POINTER(LstmCfg), C.POINTER(LstmWeights), C.POINTER(LstmState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_lstm_tracker_step": (C.c_int, [C.POINTER(LstmCfg), C.POINTER(LstmWeights), C.POINTER(LstmState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_lstm_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(LstmCfg), C.c_int32]),
    "cirs_lstm_tracker_backward": (C.c_int, [C.POINTER(LstmCfg), C.POINTER(LstmWeights), C.POINTER(LstmState), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                             C.POINTER(LstmWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_lstm": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(LstmCfg), C.POINTER(LstmWeights),
                                            C.POINTER(LstmState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                            C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_avg_tracker_init": (C.c_int, [C.POINTER(AvgCfg), C.POINTER(AvgWeights), C.POINTER(AvgState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_avg_tracker_step": (C.c_int, [C.POINTER(AvgCfg), C.POINTER(AvgWeights), C.POINTER(AvgState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_avg_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(AvgCfg), C.c_int32]),
    "cirs_avg_tracker_backward": (C.c_int, [C.POINTER(AvgCfg), C.POINTER(AvgWeights), C.POINTER(AvgState), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                            C.POINTER(AvgWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_avg": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(AvgCfg), C.POINTER(AvgWeights),
                                           C.POINTER(AvgState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                           C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_caser_tracker_init": (C.c_int, [C.POINTER(CaserCfg), C.POINTER(CaserWeights), C.POINTER(CaserState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_caser_tracker_step": (C.c_int, [C.POINTER(CaserCfg), C.POINTER(CaserWeights), C.POINTER(CaserState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_caser_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(CaserCfg), C.c_int32]),
    "cirs_caser_tracker_backward": (C.c_int, [C.POINTER(CaserCfg), C.POINTER(CaserWeights), C.POINTER(CaserState), _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                            C.POINTER(CaserWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_caser": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(CaserCfg), C.POINTER(CaserWeights),
                                             C.POINTER(CaserState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                             C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_nextitnet_tracker_init": (C.c_int, [C.POINTER(NextItNetCfg), C.POINTER(NextItNetWeights), C.POINTER(NextItNetState), _P, _P, C.c_int32, _P,
                                              C.c_int64, _P]),
    "cirs_nextitnet_tracker_step": (C.c_int, [C.POINTER(NextItNetCfg), C.POINTER(NextItNetWeights), C.POINTER(NextItNetState), _P, _P, _P, _P, C.c_int32,
                                              _P, C.c_int64, _P]),
    "cirs_nextitnet_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(NextItNetCfg), C.c_int32]),
    "cirs_nextitnet_tracker_backward": (C.c_int, [C.POINTER(NextItNetCfg), C.POINTER(NextItNetWeights), C.POINTER(NextItNetState), _P, _P, _P, _P, _P, _P,
                                                  _P, C.c_int32, _P, C.POINTER(NextItNetWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_nextitnet": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(NextItNetCfg),
                                                 C.POINTER(NextItNetWeights), C.POINTER(NextItNetState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights),
                                                 C.POINTER(Traj), C.c_int32, _P, C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_stamp_tracker_init": (C.c_int, [C.POINTER(StampCfg), C.POINTER(StampWeights), C.POINTER(StampState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_stamp_tracker_step": (C.c_int, [C.POINTER(StampCfg), C.POINTER(StampWeights), C.POINTER(StampState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_stamp_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(StampCfg), C.c_int32]),
    "cirs_stamp_tracker_backward": (C.c_int, [C.POINTER(StampCfg), C.POINTER(StampWeights), C.POINTER(StampState), _P, _P, _P, _P, _P, _P, _P, C.c_int32,
                                              _P, C.POINTER(StampWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_stamp": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(StampCfg), C.POINTER(StampWeights),
                                             C.POINTER(StampState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                             C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_narm_tracker_init": (C.c_int, [C.POINTER(NarmCfg), C.POINTER(NarmWeights), C.POINTER(NarmState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_narm_tracker_step": (C.c_int, [C.POINTER(NarmCfg), C.POINTER(NarmWeights), C.POINTER(NarmState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_narm_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(NarmCfg), C.c_int32]),
    "cirs_narm_tracker_backward": (C.c_int, [C.POINTER(NarmCfg), C.POINTER(NarmWeights), C.POINTER(NarmState), _P, _P, _P, _P, _P, _P, _P, C.c_int32,
                                             _P, C.POINTER(NarmWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_narm": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(NarmCfg), C.POINTER(NarmWeights),
                                            C.POINTER(NarmState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                            C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_fmlp_tracker_init": (C.c_int, [C.POINTER(FmlpCfg), C.POINTER(FmlpWeights), C.POINTER(FmlpState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_fmlp_tracker_step": (C.c_int, [C.POINTER(FmlpCfg), C.POINTER(FmlpWeights), C.POINTER(FmlpState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_fmlp_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(FmlpCfg), C.c_int32]),
    "cirs_fmlp_tracker_backward": (C.c_int, [C.POINTER(FmlpCfg), C.POINTER(FmlpWeights), C.POINTER(FmlpState), _P, _P, _P, _P, _P, _P, _P, C.c_int32,
                                             _P, C.POINTER(FmlpWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_fmlp": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(FmlpCfg), C.POINTER(FmlpWeights),
                                            C.POINTER(FmlpState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                            C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_lru_tracker_init": (C.c_int, [C.POINTER(LruCfg), C.POINTER(LruWeights), C.POINTER(LruState), _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_lru_tracker_step": (C.c_int, [C.POINTER(LruCfg), C.POINTER(LruWeights), C.POINTER(LruState), _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_lru_tracker_backward_workspace_bytes": (C.c_int64, [C.POINTER(LruCfg), C.c_int32]),
    "cirs_lru_tracker_backward": (C.c_int, [C.POINTER(LruCfg), C.POINTER(LruWeights), C.POINTER(LruState), _P, _P, _P, _P, _P, _P, _P, C.c_int32,
                                            _P, C.POINTER(LruWeights), _P, C.c_int64, _P]),
    "cirs_rollout_collect_lru": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), C.POINTER(LruCfg), C.POINTER(LruWeights),
                                           C.POINTER(LruState), C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), C.POINTER(Traj), C.c_int32, _P,
                                           C.c_uint64, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_embedding_scatter_workspace_bytes": (C.c_int64, [C.c_int64]),
    "cirs_embedding_scatter": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_deepfm_forward": (C.c_int, [C.POINTER(DeepFMCfg), C.POINTER(DeepFMWeights), _P, _P, _P, _P, C.c_int32, _P, _P]),
    "cirs_actor_shard_partials": (C.c_int, [C.POINTER(PolicyCfg), C.POINTER(PolicyWeights), _P, C.c_int64, C.c_int32, C.c_uint64, C.c_uint32,
                                            _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, _P]),
    "cirs_actor_merge_shards": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "cirs_gather_rows": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, _P]),
    "cirs_gather_fm": (C.c_int, [C.POINTER(DeepFMCfg), C.POINTER(DeepFMWeights), _P, C.c_int64, _P, _P]),
    "cirs_deepfm_sweep_workspace_bytes": (C.c_int64, [C.POINTER(DeepFMCfg), C.c_int32, C.c_int32]),
    "cirs_deepfm_sweep": (C.c_int, [C.POINTER(DeepFMCfg), C.POINTER(DeepFMWeights), _P, C.c_int32, _P, _P, _P, C.c_int32,
                                    _P, _P, C.c_int32, _P, C.c_int64, _P]),
    "cirs_normed_reward": (C.c_int, [_P, C.c_int64, _P, _P, _P]),
    "cirs_ppo_minibatch_dp": (C.c_int, [C.POINTER(PpoCfg), _P, _P, _P, _P, C.c_int64, C.POINTER(PpoBatch), _P, C.c_int32, _P,
                                        C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P]),
    "cirs_ppo_tp_exchange_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "cirs_ppo_minibatch_tp": (C.c_int, [C.POINTER(PpoCfg), _P, _P, _P, _P, C.c_int64, C.POINTER(PpoBatch), _P, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P]),
    "cirs_ppo_shard_stat_floats": (C.c_int32, []),
    "cirs_ppo_shard_norm": (C.c_int, [C.POINTER(PpoCfg), _P, C.c_int64, C.c_int64, _P, _P]),
    "cirs_ppo_shard_adam": (C.c_int, [C.POINTER(PpoCfg), _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int32, _P, _P]),
    "cirs_deepfm_train_param_count": (C.c_int64, [C.POINTER(DeepFMCfg)]),
    "cirs_deepfm_train_workspace_bytes": (C.c_int64, [C.POINTER(DeepFMCfg), C.c_int32]),
    "cirs_deepfm_train_step": (C.c_int, [C.POINTER(DeepFMCfg), _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32,
                                         C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         _P, _P, C.c_int64, _P]),
    "cirs_deepfm_train_epoch": (C.c_int, [C.POINTER(DeepFMCfg), _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64,
                                          _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.c_float, C.c_float, _P, _P, C.c_int64, _P]),
    "cirs_dice_train_param_count": (C.c_int64, [C.POINTER(DiceCfg)]),
    "cirs_dice_train_workspace_bytes": (C.c_int64, [C.POINTER(DiceCfg), C.c_int32]),
    "cirs_dice_train_epoch": (C.c_int, [C.POINTER(DiceCfg), _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64,
                                        _P, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                        _P, _P, C.c_int64, _P]),
    "cirs_dice_forward": (C.c_int, [C.POINTER(DiceCfg), _P, _P, _P, _P, _P, C.c_int64, _P, _P]),
    "cirs_deepfm_validate_workspace_bytes": (C.c_int64, [C.POINTER(DeepFMCfg), C.c_int64]),
    "cirs_deepfm_validate": (C.c_int, [C.POINTER(DeepFMCfg), C.POINTER(DeepFMWeights), _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P]),
    "cirs_dice_validate_workspace_bytes": (C.c_int64, [C.POINTER(DiceCfg), C.c_int64]),
    "cirs_dice_validate": (C.c_int, [C.POINTER(DiceCfg), _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P]),
    "cirs_linucb_update": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "cirs_linucb_solve": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "cirs_linucb_score": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_double, _P, _P, _P, _P, _P, _P]),
    "cirs_linucb_predict": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    "cirs_mmoe_train_param_count": (C.c_int64, [C.POINTER(MmoeTrainCfg)]),
    "cirs_mmoe_train_workspace_bytes": (C.c_int64, [C.POINTER(MmoeTrainCfg), C.c_int32]),
    "cirs_mmoe_train_step": (C.c_int, [C.POINTER(MmoeTrainCfg), _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_mmoe_train_epoch": (C.c_int, [C.POINTER(MmoeTrainCfg), _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P, C.c_int64, C.c_int32,
                                        _P, _P, C.c_int64, _P]),
    "cirs_vtb_exposure_history": (C.c_int, [_P, _P, C.c_int64, C.c_double, _P, _P, _P]),
    "cirs_mlp_train_param_count": (C.c_int64, [C.POINTER(MlpTrainCfg)]),
    "cirs_mlp_train_workspace_bytes": (C.c_int64, [C.POINTER(MlpTrainCfg), C.c_int32]),
    "cirs_mlp_train_step": (C.c_int, [C.POINTER(MlpTrainCfg), _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int32, _P, _P, C.c_int64, _P]),
    "cirs_mlp_train_epoch": (C.c_int, [C.POINTER(MlpTrainCfg), _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, C.c_int32,
                                       _P, _P, C.c_int64, _P]),
    "cirs_exposure_history": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int32, C.c_double, _P, _P]),
    "cirs_find_negative": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, C.c_int64, _P, _P]),
    "cirs_item_bin_counts": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "cirs_item_bin_gather": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P]),
    "cirs_select_items": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_float, _P, C.c_uint64, C.c_uint32,
                                    _P, _P, _P]),
    "cirs_rollout_static": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(EnvTables), C.POINTER(EnvState), _P, C.c_int64, _P, C.POINTER(Traj),
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_uint32, _P, C.c_int32, _P, _P]),
    "cirs_hash_ids": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P]),
    "cirs_random_permutation": (C.c_int, [C.c_int64, C.c_uint64, C.c_uint64, _P, _P]),
    "cirs_random_permutations": (C.c_int, [C.c_int64, C.c_uint64, C.c_uint64, C.c_int32, _P, _P]),
    "cirs_prof_start": (C.c_int, [C.c_int32, C.c_int32]),
    "cirs_prof_stop": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "cirs_eval_coverage": (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "cirs_adam_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_float,
                                 C.c_float, _P, C.c_int32, _P]),
    "cirs_rows_topk": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "cirs_rank_metrics_workspace_bytes": (C.c_int64, [C.c_int32]),
    "cirs_rank_metrics": (C.c_int, [C.POINTER(RankCfg), _P, C.c_int64, _P, C.c_int32, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
}

_lib = None


class CirsHipError(RuntimeError):
    pass


def lib():
    """Load libcirs_hip.so (built in-tree by `__graft_entry__.build()` / `cirs_hip.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CirsHipError(
            f"{LIB_PATH} not found: the HIP extension is the only implementation of this path (no CPU fallback). "
            "Build it with `python __graft_entry__.py build` (hipcc --offload-arch=gfx950).")
    # torch first: its bundled HIP runtime must be the one this process uses.  Loading libcirs_hip.so before torch pulls in
    # the system libamdhip64 instead, and launches on torch's device pointers then fail ("no ROCm-capable device").
    import torch  # noqa: F401
    handle = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as exc:
            raise CirsHipError(f"libcirs_hip.so does not export {name}") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().cirs_last_error()
        raise CirsHipError(f"{what} failed rc={rc}: {msg.decode() if msg else ''}")


def ptr(t):
    """Device (or host) pointer of a torch tensor / numpy array as an int, 0 for None."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data
