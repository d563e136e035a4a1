// deepfm_train.hip -- one optimiser step of the pairwise DeepFM user model:
//   UserModel_Pairwise.get_loss (reference core/user_model_pairwise.py:134-151), loss_kuaishou_pairwise
//   (CIRS-UserModel-kuaishou.py:262-278), get_regularization_loss (core/user_model.py:401-417), total_loss.backward() and
//   optim.step() (Adam) of fit_data's inner loop (core/user_model.py:150-170).
//
//   train_rows_kernel   one wavefront per sample: DeepFM forward of the positive and the negative pair (activations in LDS),
//                       the sample's loss terms and d loss / d y, then the backward of both pairs down to the embedding rows:
//                       per-row DNN pre-activation gradients / inputs go to global memory for the weight-gradient GEMMs,
//                       per-row embedding contributions (FM + DNN input gradient + linear term + alpha/beta) to the
//                       contribution tables.
// This file holds the model's own parts: the parameter layout, the linear term and the contribution rows around the tower, the three
// losses, the workspace carve and the entry points.  Shared with dice_train.hip:
//   deepfm_tower.h      the tower (FM cross term + DNN) forward / backward of one row, the feature contribution rows, the row lookup,
//                       the loss means, the tower's weight-gradient GEMMs (dw_gemm of small_gemm.h: fp32 MFMA row-slab partials,
//                       fixed-order sums)
//   table_step.h        the workspace allocator, the sorted scatter (user rows: [d emb_user | d lin_user | d alpha], item rows:
//                       [d emb_item | d lin_item | d beta], feature rows: [d emb_feat | d lin_feat]; padding row 0 of emb_feat gets no
//                       gradient), regulariser + Adam
// All reductions have a fixed order: two runs give identical bits.
//
// train_rows_kernel takes the loss as a compile-time kind (the pair forward / backward, the GEMMs, the scatter and Adam are shared):
//   0  loss_kuaishou_pairwise          exposure-discounted regression + BPR + alpha/beta penalty (above)
//   1  loss_kuaishou_IPS_pairwise      DeepFM-IPS-pairwise.py:249-258: mean((yp - y)^2 w) + mean(-log sigmoid(yp - yn) w), w = score
//   2  loss_kuaishou_PD_pairwise       PD-pairwise.py:242-251: mean((yp pop - y)^2) + mean(-log sigmoid(yp - yn)), pop = score
// and reads sample i of a step at row order[r0 + i] of a device-resident data set (r0 + i when order is null), so that
// cirs_deepfm_train_epoch queues every step of a pass back to back without a gather launch or a host round trip.
#include "deepfm_tower.h"

namespace cirs {

struct TrainLayout {  // offsets (floats) into the flat parameter / gradient / moment buffers
    long emb_user, emb_item, emb_feat, lin_user, lin_item, lin_feat, lin_dense;
    TowerNet net;
    long alpha_u, beta_i, lm_user, lm_item, lm_feat, lm_dense, total;
};
__host__ __device__ inline TrainLayout train_layout(const cirs_deepfm_cfg& c) {
    const long U = c.n_user_vocab, I = c.n_item_vocab, F = c.n_feat_vocab, E = c.emb_dim, K = 6 * E + 1;
    TrainLayout L;
    long o = 0;
    L.emb_user = o; o += U * E; L.emb_item = o; o += I * E; L.emb_feat = o; o += F * E;
    L.lin_user = o; o += U; L.lin_item = o; o += I; L.lin_feat = o; o += F; L.lin_dense = o; o += 1;
    L.net = tower_net(o, K);
    L.alpha_u = o; o += U; L.beta_i = o; o += I;
    L.lm_user = o; o += U; L.lm_item = o; o += I; L.lm_feat = o; o += F; L.lm_dense = o; o += 1;
    L.total = o;
    return L;
}

struct TrainRows {  // per-pair-row outputs of train_rows_kernel, R = 2n rows (positives first)
    TowerRows t;                                // the tower's GEMM operands
    float* DUR;                                 // [R]
    float *CU, *CI, *CF;                        // contributions [R,E+2] [R,E+2] [4R,E+1]
    int32_t *KU, *KI, *KF;                      // keys [R] [R] [4R]
    float* LP;                                  // [n,4] per-sample loss terms {sq err, bpr, (alpha-1)^2, (beta-1)^2}
};

// the workspace of a step on n samples: the size query runs this carve without a base pointer, the launch on the caller's workspace
struct TrainWs { TrainRows o; StepScratch x; };
static TrainWs train_carve(Bump& w, int E, size_t n) {
    const size_t R = 2 * n;
    const int K = 6 * E + 1;
    TrainWs t;
    t.o.t = tower_rows(w, R, K); t.o.DUR = w.take(R);
    t.o.CU = w.take(R * (E + 2)); t.o.CI = w.take(R * (E + 2)); t.o.CF = w.take(4 * R * (E + 1));
    t.o.KU = (int32_t*)w.take(R); t.o.KI = (int32_t*)w.take(R); t.o.KF = (int32_t*)w.take(4 * R);
    t.o.LP = w.take(4 * n + 8);
    t.x = step_scratch(w, tower_partial_floats(R, K), 4 * R);
    return t;
}

// forward of one (user, item) pair by one wavefront; x / S / a1 / a2 stay in LDS for the backward
__device__ __forceinline__ float pair_forward(const float* __restrict__ P, const TrainLayout& L, int E, int K, long u, long p,
                                              const int32_t* f4, float dur, int lane, float* x, float* S, float* a1, float* a2) {
    for (int k = lane; k < 6 * E; k += CIRS_WAVE) {
        const int fld = k / E, e = k % E;
        float v;
        if (fld == 0) v = P[L.emb_user + u * E + e];
        else if (fld == 1) v = P[L.emb_item + p * E + e];
        else v = P[L.emb_feat + (long)f4[fld - 2] * E + e];
        x[k] = v;
    }
    if (lane == 0) x[6 * E] = dur;
    __builtin_amdgcn_wave_barrier();
    float logit = P[L.lin_user + u] + P[L.lin_item + p];
#pragma unroll
    for (int q = 0; q < 4; ++q) logit += P[L.lin_feat + f4[q]];
    logit += dur * P[L.lin_dense];
    const TowerOut t = tower_forward(P, L.net, 6, E, K, lane, x, S, a1, a2);
    logit += 0.5f * t.cross;
    return logit + t.dnn;
}

// backward of one pair row r given dy; writes the row's GEMM operands and embedding contributions
__device__ __forceinline__ void pair_backward(const float* __restrict__ P, const TrainLayout& L, int E, int K, long u, long p,
                                              const int32_t* f4, float dur, float dy, float dalpha, float dbeta, int lane, int r,
                                              const float* x, const float* S, const float* a1, const float* a2, float* t64,
                                              float* dxs, const TrainRows& o) {
    tower_backward(P, L.net, 6, E, K, dy, lane, (size_t)r, x, S, a1, a2, t64, dxs, o.t);
    if (lane == 0) { o.DUR[r] = dur; o.KU[r] = (int32_t)u; o.KI[r] = (int32_t)p; }
    const int WU = E + 2;
    for (int e = lane; e < WU; e += CIRS_WAVE) {
        o.CU[(size_t)r * WU + e] = e < E ? dxs[e] : (e == E ? dy : dalpha);
        o.CI[(size_t)r * WU + e] = e < E ? dxs[E + e] : (e == E ? dy : dbeta);
    }
    write_feat_contrib(o.CF, o.KF, (size_t)r, E, f4, dxs, 2, dy, lane);
    __builtin_amdgcn_wave_barrier();
}

struct TrainCols {  // the batch (or the whole data set) in column form; exposure = the score column of the loss kind
    const int64_t *uid_pos, *pid_pos; const int32_t* feats_pos; const float* dur_pos;
    const int64_t *uid_neg, *pid_neg; const int32_t* feats_neg; const float* dur_neg;
    const float *y, *exposure;
};

constexpr int kLossPairwise = 0, kLossIPS = 1, kLossPD = 2;

template <int KIND>
__global__ __launch_bounds__(256) void train_rows_kernel(cirs_deepfm_cfg cfg, const float* __restrict__ P, TrainCols c,
                                                         const int64_t* __restrict__ order, long r0, long n_rows, int n, int use_ab,
                                                         float lambda_ab, TrainRows o) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int E = cfg.emb_dim, K = 6 * E + 1;
    const TrainLayout L = train_layout(cfg);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= n) return;
    const int per_pair = K + 1 + E + 2 * kTowerH;
    float* base = smem + (size_t)wv * (2 * per_pair + kTowerH + 6 * E + 8);
    float *xp = base, *Sp = xp + K + 1, *a1p = Sp + E, *a2p = a1p + kTowerH;
    float *xn = base + per_pair, *Sn = xn + K + 1, *a1n = Sn + E, *a2n = a1n + kTowerH;
    float* t64 = base + 2 * per_pair;
    float* dxs = t64 + kTowerH;
    bool bad_row;
    const long row = step_row(order, r0, i, n_rows, bad_row);
    const long up = c.uid_pos[row], pp = c.pid_pos[row], un = c.uid_neg[row], pn = c.pid_neg[row];
    int32_t fp[4], fn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { fp[q] = c.feats_pos[(size_t)row * 4 + q]; fn[q] = c.feats_neg[(size_t)row * 4 + q]; }
    const float dp = c.dur_pos[row], dn = c.dur_neg[row];
    const float yp = pair_forward(P, L, E, K, up, pp, fp, dp, lane, xp, Sp, a1p, a2p);
    const float yn = pair_forward(P, L, E, K, un, pn, fn, dn, lane, xn, Sn, a1n, a2n);
    // ---- the loss on this sample; every mean is over the n samples of the batch -----------------------------------
    const float inv_n = 1.0f / (float)n;
    const float ex = c.exposure[row];
    const float sg = 1.0f / (1.0f + expf(-(yp - yn)));   // sigmoid(y_pos - y_neg)
    float dyp, dyn, dalpha = 0.f, dbeta = 0.f, lp4[4];
    if constexpr (KIND == kLossPairwise) {
        float alpha = 1.f, beta = 1.f;
        if (use_ab) { alpha = P[L.alpha_u + up]; beta = P[L.beta_i + pp]; }
        const float ex_new = use_ab ? ex * alpha * beta : ex;
        const float inv1 = 1.0f / (1.0f + ex_new);
        const float y_exp = inv1 * yp;
        const float err = y_exp - c.y[row];
        dyp = 2.0f * inv_n * err * inv1 - inv_n * (1.0f - sg);
        dyn = inv_n * (1.0f - sg);
        if (use_ab) {
            const float dex = 2.0f * inv_n * err * (-yp * inv1 * inv1);   // d loss_y / d exposure_new
            dalpha = dex * ex * beta + lambda_ab * 2.0f * inv_n * (alpha - 1.0f);
            dbeta = dex * ex * alpha + lambda_ab * 2.0f * inv_n * (beta - 1.0f);
        }
        lp4[0] = err * err;
        lp4[1] = -logf(sg);
        lp4[2] = use_ab ? (alpha - 1.0f) * (alpha - 1.0f) : 0.f;
        lp4[3] = use_ab ? (beta - 1.0f) * (beta - 1.0f) : 0.f;
    } else if constexpr (KIND == kLossIPS) {   // ex = the inverse-propensity weight of the sample
        const float err = yp - c.y[row];
        dyp = inv_n * ex * (2.0f * err - (1.0f - sg));
        dyn = inv_n * ex * (1.0f - sg);
        lp4[0] = ex * (err * err);
        lp4[1] = -(ex * logf(sg));
        lp4[2] = 0.f; lp4[3] = 0.f;
    } else {                                   // ex = popularity^gamma of the sample's item in its time bin
        const float err = yp * ex - c.y[row];
        dyp = 2.0f * inv_n * err * ex - inv_n * (1.0f - sg);
        dyn = inv_n * (1.0f - sg);
        lp4[0] = err * err;
        lp4[1] = -logf(sg);
        lp4[2] = 0.f; lp4[3] = 0.f;
    }
    if (lane == 0) {
        float* lp = o.LP + (size_t)i * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) lp[q] = lp4[q];
        if (bad_row) lp[0] = __builtin_nanf("");
    }
    pair_backward(P, L, E, K, up, pp, fp, dp, dyp, dalpha, dbeta, lane, i, xp, Sp, a1p, a2p, t64, dxs, o);
    pair_backward(P, L, E, K, un, pn, fn, dn, dyn, 0.f, 0.f, lane, n + i, xn, Sn, a1n, a2n, t64, dxs, o);
}

// batch loss terms -> {loss, loss_y, bpr, loss_ab}
__global__ __launch_bounds__(256) void train_loss_kernel(const float* __restrict__ LP, int n, float lambda_ab, float* __restrict__ loss_out) {
    float m[4];
    loss_means4(LP, n, m);
    if (threadIdx.x == 0) {
        const float ly = m[0], bpr = m[1], lab = m[2] + m[3];
        loss_out[0] = ly + bpr + lambda_ab * lab;
        loss_out[1] = ly; loss_out[2] = bpr; loss_out[3] = lab;
    }
}

}  // namespace cirs

extern "C" int64_t cirs_deepfm_train_param_count(const cirs_deepfm_cfg* cfg) {
    if (!cfg) return 0;
    return cirs::train_layout(*cfg).total;
}

extern "C" int64_t cirs_deepfm_train_workspace_bytes(const cirs_deepfm_cfg* cfg, int32_t n) {
    if (!cfg || n <= 0) return 0;
    cirs::Bump w{nullptr};
    cirs::train_carve(w, cfg->emb_dim, n);
    return (int64_t)(w.used * sizeof(float));
}

namespace cirs {

struct TrainHyper { int use_ab; float lambda_ab; TableHyper t; };

static int train_check_cfg(const cirs_deepfm_cfg* cfg) {
    if (cfg->hidden != kTowerH) return fail(CIRS_E_UNSUPPORTED, "deepfm train: hidden == 64 only");
    CIRS_REQUIRE(cfg->emb_dim >= 1 && cfg->emb_dim <= 64, "emb_dim out of range");
    return CIRS_OK;
}

// the launches of one step on the n samples order[r0 .. r0 + n) of the columns (rows r0 .. r0 + n - 1 when order is null)
static int train_launch_step(const cirs_deepfm_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t step_before,
                             const TrainCols& c, const int64_t* order, long r0, long n_rows, int n, int kind, const TrainHyper& h,
                             float* loss_out, void* workspace, hipStream_t s) {
    const int use_ab = h.use_ab;
    const float lambda_ab = h.lambda_ab;
    const int E = cfg->emb_dim, K = 6 * E + 1, R = 2 * n;
    const TrainLayout L = train_layout(*cfg);
    Bump w{(float*)workspace};
    const TrainWs ws = train_carve(w, E, n);
    const TrainRows& o = ws.o;
    // the data gradient is written sparsely (touched table rows, dense layers): start from zero
    CIRS_HIP(hipMemsetAsync(grads, 0, sizeof(float) * (size_t)L.total, s));
    const size_t shmem = sizeof(float) * 4 * (2 * (size_t)(K + 1 + E + 2 * kTowerH) + kTowerH + 6 * E + 8);
    const dim3 grid(cdiv(n, 4));
    switch (kind) {
    case kLossPairwise:
        hipLaunchKernelGGL(train_rows_kernel<kLossPairwise>, grid, dim3(256), shmem, s, *cfg, (const float*)params, c, order, r0, n_rows, n, use_ab,
                           lambda_ab, o);
        break;
    case kLossIPS:
        hipLaunchKernelGGL(train_rows_kernel<kLossIPS>, grid, dim3(256), shmem, s, *cfg, (const float*)params, c, order, r0, n_rows, n, use_ab,
                           lambda_ab, o);
        break;
    default:
        hipLaunchKernelGGL(train_rows_kernel<kLossPD>, grid, dim3(256), shmem, s, *cfg, (const float*)params, c, order, r0, n_rows, n, use_ab,
                           lambda_ab, o);
    }
    CIRS_CHECK_LAUNCH("train_rows_kernel");
    hipLaunchKernelGGL(train_loss_kernel, dim3(1), dim3(256), 0, s, (const float*)o.LP, (int)n, lambda_ab, loss_out);
    // dense layers: dW = dY^T X over the 2n pair rows
    launch_tower_dw(o.t, R, K, grads, L.net, true, ws.x.partial, s);
    launch_dw_gemm(o.t.DY, 1, o.DUR, 1, R, 1, 1, grads + L.lin_dense, nullptr, ws.x.partial, s);
    CIRS_CHECK_LAUNCH("deepfm train dW");
    // table rows
    ScatterDst du{{grads + L.emb_user, grads + L.lin_user, use_ab ? grads + L.alpha_u : nullptr}, {E, 1, 1}};
    ScatterDst di{{grads + L.emb_item, grads + L.lin_item, use_ab ? grads + L.beta_i : nullptr}, {E, 1, 1}};
    ScatterDst df{{grads + L.emb_feat, grads + L.lin_feat, nullptr}, {E, 1, 0}};
    if (int rc = train_scatter(o.KU, o.CU, R, E + 2, cfg->n_user_vocab, du, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    if (int rc = train_scatter(o.KI, o.CI, R, E + 2, cfg->n_item_vocab, di, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    if (int rc = train_scatter(o.KF, o.CF, 4 * R, E + 1, cfg->n_feat_vocab, df, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    L2Segs segs;
    segs.n = 4;
    segs.end[0] = L.lin_user;  segs.c[0] = h.t.l2_embedding + h.t.l2_all;   // embedding_dict.*            (core/user_model.py:60-63)
    segs.end[1] = L.lm_user;   segs.c[1] = h.t.l2_all;                        // linear.*, dnn, last, out.bias, alpha_u, beta_i
    segs.end[2] = L.total;     segs.c[2] = h.t.l2_linear + h.t.l2_all;      // linear_model.* (unused in forward, still decays)
    segs.end[3] = L.total;     segs.c[3] = h.t.l2_linear + h.t.l2_all;
    return table_adam_step(params, grads, adam_m, adam_v, L.total, segs, h.t, step_before, ws.x.regp, loss_out, 4, s);
}

}  // namespace cirs

extern "C" int cirs_deepfm_train_step(const cirs_deepfm_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                                      int64_t step_before, const int64_t* uid_pos, const int64_t* pid_pos, const int32_t* feats_pos,
                                      const float* dur_pos, const int64_t* uid_neg, const int64_t* pid_neg, const int32_t* feats_neg,
                                      const float* dur_neg, const float* y, const float* exposure, int32_t n, int32_t use_ab,
                                      float lambda_ab, float l2_embedding, float l2_linear, float l2_all, float lr, float beta1,
                                      float beta2, float eps, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(cfg && params && grads && adam_m && adam_v && loss_out && workspace, "null argument");
    if (int rc = train_check_cfg(cfg)) return rc;
    CIRS_REQUIRE(n >= 1, "empty batch");
    CIRS_REQUIRE(uid_pos && pid_pos && feats_pos && dur_pos && uid_neg && pid_neg && feats_neg && dur_neg && y && exposure, "null batch column");
    CIRS_REQUIRE(workspace_bytes >= cirs_deepfm_train_workspace_bytes(cfg, n), "workspace too small");
    const TrainCols c{uid_pos, pid_pos, feats_pos, dur_pos, uid_neg, pid_neg, feats_neg, dur_neg, y, exposure};
    const TrainHyper h{(int)use_ab, lambda_ab, {l2_embedding, l2_linear, l2_all, lr, beta1, beta2, eps}};
    return train_launch_step(cfg, params, grads, adam_m, adam_v, step_before, c, nullptr, 0, n, n, kLossPairwise, h, loss_out, workspace,
                             (hipStream_t)stream);
}

extern "C" int cirs_deepfm_train_epoch(const cirs_deepfm_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                                       int64_t step_before, const int64_t* uid_pos, const int64_t* pid_pos, const int32_t* feats_pos,
                                       const float* dur_pos, const int64_t* uid_neg, const int64_t* pid_neg, const int32_t* feats_neg,
                                       const float* dur_neg, const float* y, const float* score, int64_t n_rows, const int64_t* order,
                                       int64_t n_order, int32_t batch_size, int32_t loss_kind, int32_t use_ab, float lambda_ab,
                                       float l2_embedding, float l2_linear, float l2_all, float lr, float beta1, float beta2, float eps,
                                       float* losses_out, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(cfg, "null argument");
    if (int rc = train_check_cfg(cfg)) return rc;
    CIRS_REQUIRE(loss_kind == kLossPairwise || loss_kind == kLossIPS || loss_kind == kLossPD, "deepfm train: unknown loss kind (0 pairwise, 1 IPS, 2 PD)");
    CIRS_REQUIRE(loss_kind == kLossPairwise || !use_ab, "deepfm train: the IPS and PD losses take no alpha/beta (their models are built without ab_columns)");
    const int64_t bmax = batch_size < n_order ? batch_size : n_order;
    const TrainCols c{uid_pos, pid_pos, feats_pos, dur_pos, uid_neg, pid_neg, feats_neg, dur_neg, y, score};
    const TrainHyper h{(int)use_ab, loss_kind == kLossPairwise ? lambda_ab : 0.f, {l2_embedding, l2_linear, l2_all, lr, beta1, beta2, eps}};
    return tstep::run_steps(params, grads, adam_m, adam_v, losses_out, workspace,
                            uid_pos && pid_pos && feats_pos && dur_pos && uid_neg && pid_neg && feats_neg && dur_neg && y && score, "null data column",
                            n_rows >= 1 && n_order >= 1 && batch_size >= 1 && (order || n_order <= n_rows), "empty data set, index array or batch",
                            step_before, workspace_bytes, cirs_deepfm_train_workspace_bytes(cfg, (int32_t)bmax), n_order, batch_size,
                            [&](int64_t st, int64_t r0, int nb) {
                                return train_launch_step(cfg, params, grads, adam_m, adam_v, step_before + st, c, order, r0, n_rows, nb, loss_kind, h,
                                                         losses_out + 5 * st, workspace, (hipStream_t)stream);
                            });
}
