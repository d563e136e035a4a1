// dice_train.hip -- one optimiser step of the DICE debiasing baseline (UserModel_DICE):
//   UserModel_DICE.get_loss / _deepfm / forward (reference core/user_model_DICE.py:122-192), loss_kuaishou_DICE (DICE.py:273-286),
//   get_regularization_loss (core/user_model.py:401-417), total_loss.backward() and optim.step() (Adam) of fit_data's inner loop
//   (core/user_model.py:150-170).
//
// The model is two DeepFM networks over five shared embedding tables:
//   main  8 sparse fields [user_int, user_con, photo_int, photo_con, feat0..3] + the dense duration; linear_main, FM over 8 fields,
//         dnn_main [64, 8E+1] [64, 64], last_main, out_main.bias.  Run on the positive and on the negative row.
//   ui    2 sparse fields; linear_ui (tables user_int, photo_int only), FM over 2 fields, dnn_ui [64, 2E] [64, 64], last_ui,
//         out_ui.bias.  Run four times: (user_int, photo_int) and (user_con, photo_con) embeddings on the positive and the negative
//         item; the two linear_ui tables are indexed with the ids of the columns the call was given (the con ids in the con calls).
//
//   dice_rows_kernel    one wavefront per sample: the six forwards (activations in LDS), the four loss terms and d loss / d y of each
//                       forward, then the backward of all six: per-row DNN operands to global memory for the weight-gradient GEMMs
//                       (dnn_main on 2n rows, dnn_ui on 4n rows), the sample's embedding / linear contributions, summed per key in a
//                       fixed order in LDS, to the contribution tables.
// This file holds the model's own parts: the parameter layout, the linear terms around the two towers, the six-forward / six-backward
// sequence with its per-key sums, the loss, the workspace carve and the entry points.  Shared with deepfm_train.hip:
//   deepfm_tower.h      the tower (FM cross term + DNN) forward / backward of one row, the feature contribution rows, the row lookup,
//                       the loss means, a tower's weight-gradient GEMMs (dw_gemm of small_gemm.h: fp32 MFMA row-slab partials,
//                       fixed-order sums)
//   table_step.h        the workspace allocator, the ordered scatter of the contributions (five key spaces), regulariser + Adam
// All reductions have a fixed order: two runs give identical bits.
#include "deepfm_tower.h"

namespace cirs {

struct DiceLayout {  // offsets (floats) into the flat parameter / gradient / moment buffers
    long emb_user_int, emb_user_con, emb_photo_int, emb_photo_con, emb_feat;
    long lm_user_int, lm_user_con, lm_photo_int, lm_photo_con, lm_feat, lm_dense;   // linear_main
    long lu_user, lu_photo;                                                         // linear_ui
    TowerNet main, ui;
    long unused, total;                                                             // linear_model.* (no data gradient)
};
__host__ __device__ inline DiceLayout dice_layout(const cirs_dice_cfg& c) {
    const long U = c.n_user_vocab, I = c.n_item_vocab, F = c.n_feat_vocab, E = c.emb_dim;
    DiceLayout L;
    long o = 0;
    L.emb_user_int = o; o += U * E; L.emb_user_con = o; o += U * E; L.emb_photo_int = o; o += I * E; L.emb_photo_con = o; o += I * E;
    L.emb_feat = o; o += F * E;
    L.lm_user_int = o; o += U; L.lm_user_con = o; o += U; L.lm_photo_int = o; o += I; L.lm_photo_con = o; o += I; L.lm_feat = o; o += F;
    L.lm_dense = o; o += 1;
    L.lu_user = o; o += U; L.lu_photo = o; o += I;
    L.main = tower_net(o, 8 * E + 1);
    L.ui = tower_net(o, 2 * E);
    L.unused = o; o += 2 * U + 2 * I + F + 2;
    L.total = o;
    return L;
}

struct DiceOut {
    TowerRows m, u;                      // main: 2n rows (positives first); ui: 4n rows (int pos | int neg | con pos | con neg)
    float* DUR;                          // [2n]
    float *CUI, *CUC, *CPI, *CPC, *CF;   // contributions [n,E+2] [n,E+2] [2n,E+2] [2n,E+2] [8n,E+1]
    int32_t *KUI, *KUC, *KPI, *KPC, *KF; // keys [n] [n] [2n] [2n] [8n]
    float* LP;                           // [n,4] per-sample loss terms {sq err, bpr_click, bpr_con, bpr_int}
};

// the main DeepFM (is_main=True) on one row: ids[0..3] = user_int, user_con, photo_int, photo_con
__device__ __forceinline__ float dice_main_forward(const float* __restrict__ P, const DiceLayout& L, int E, const long* ids, const int32_t* f4,
                                                   float dur, int lane, float* x, float* S, float* a1, float* a2) {
    const int K = 8 * E + 1;
    for (int k = lane; k < 8 * E; k += CIRS_WAVE) {
        const int fld = k / E, e = k % E;
        float v;
        if (fld == 0) v = P[L.emb_user_int + ids[0] * E + e];
        else if (fld == 1) v = P[L.emb_user_con + ids[1] * E + e];
        else if (fld == 2) v = P[L.emb_photo_int + ids[2] * E + e];
        else if (fld == 3) v = P[L.emb_photo_con + ids[3] * E + e];
        else v = P[L.emb_feat + (long)f4[fld - 4] * E + e];
        x[k] = v;
    }
    if (lane == 0) x[8 * E] = dur;
    __builtin_amdgcn_wave_barrier();
    float logit = (P[L.lm_user_int + ids[0]] + P[L.lm_user_con + ids[1]]) + (P[L.lm_photo_int + ids[2]] + P[L.lm_photo_con + ids[3]]);
#pragma unroll
    for (int q = 0; q < 4; ++q) logit += P[L.lm_feat + f4[q]];
    logit += dur * P[L.lm_dense];
    const TowerOut t = tower_forward(P, L.main, 8, E, K, lane, x, S, a1, a2);
    return logit + (0.5f * t.cross + t.dnn);
}

// the UI DeepFM (is_main=False) on one (user, photo) pair: embeddings from the tables at emb_u / emb_p, linear_ui indexed with the same ids
__device__ __forceinline__ float dice_ui_forward(const float* __restrict__ P, const DiceLayout& L, int E, long emb_u, long emb_p, long u, long p,
                                                 int lane, float* x, float* S, float* a1, float* a2) {
    for (int k = lane; k < 2 * E; k += CIRS_WAVE) x[k] = k < E ? P[emb_u + u * E + k] : P[emb_p + p * E + (k - E)];
    __builtin_amdgcn_wave_barrier();
    const float logit = P[L.lu_user + u] + P[L.lu_photo + p];
    const TowerOut t = tower_forward(P, L.ui, 2, E, 2 * E, lane, x, S, a1, a2);
    return logit + (0.5f * t.cross + t.dnn);
}

struct DiceCols {  // the data set in column form (x16 of the reference split by column; feats [n_rows,4])
    const int64_t *uid_int, *uid_con, *pid_int, *pid_con; const int32_t* feats_pos; const float* dur_pos;
    const int64_t *pid_int_neg, *pid_con_neg; const int32_t* feats_neg; const float* dur_neg;
    const float *y, *score;
};

// LDS floats of one wavefront
__host__ __device__ inline int dice_main_lds(int E) { return (8 * E + 2) + E + 2 * kTowerH; }
__host__ __device__ inline int dice_ui_lds(int E) { return 2 * E + E + 2 * kTowerH; }
__host__ __device__ inline int dice_wave_lds(int E) { return 2 * dice_main_lds(E) + 4 * dice_ui_lds(E) + kTowerH + 8 * E + 6 * E + 8; }

__global__ __launch_bounds__(256) void dice_rows_kernel(cirs_dice_cfg cfg, const float* __restrict__ P, DiceCols c, const int64_t* __restrict__ order,
                                                        long r0, long n_rows, int n, DiceOut o) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int E = cfg.emb_dim, Km = 8 * E + 1, Ku = 2 * E;
    const DiceLayout L = dice_layout(cfg);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= n) return;
    float* base = smem + (size_t)wv * dice_wave_lds(E);
    float *xm[2], *Sm[2], *a1m[2], *a2m[2], *xu[4], *Su[4], *a1u[4], *a2u[4];
#pragma unroll
    for (int q = 0; q < 2; ++q) { xm[q] = base; Sm[q] = xm[q] + 8 * E + 2; a1m[q] = Sm[q] + E; a2m[q] = a1m[q] + kTowerH; base += dice_main_lds(E); }
#pragma unroll
    for (int q = 0; q < 4; ++q) { xu[q] = base; Su[q] = xu[q] + 2 * E; a1u[q] = Su[q] + E; a2u[q] = a1u[q] + kTowerH; base += dice_ui_lds(E); }
    float* t64 = base;
    float* dxs = t64 + kTowerH;
    float* acc = dxs + 8 * E;   // [6, E]: user_int | user_con | photo_int pos | photo_con pos | photo_int neg | photo_con neg
    bool bad_row;
    const long row = step_row(order, r0, i, n_rows, bad_row);
    const long idp[4] = {(long)c.uid_int[row], (long)c.uid_con[row], (long)c.pid_int[row], (long)c.pid_con[row]};
    const long idn[4] = {idp[0], idp[1], (long)c.pid_int_neg[row], (long)c.pid_con_neg[row]};
    int32_t fp[4], fn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { fp[q] = c.feats_pos[(size_t)row * 4 + q]; fn[q] = c.feats_neg[(size_t)row * 4 + q]; }
    const float dp = c.dur_pos[row], dn = c.dur_neg[row];
    const float yp = dice_main_forward(P, L, E, idp, fp, dp, lane, xm[0], Sm[0], a1m[0], a2m[0]);
    const float yn = dice_main_forward(P, L, E, idn, fn, dn, lane, xm[1], Sm[1], a1m[1], a2m[1]);
    const float ypi = dice_ui_forward(P, L, E, L.emb_user_int, L.emb_photo_int, idp[0], idp[2], lane, xu[0], Su[0], a1u[0], a2u[0]);
    const float yni = dice_ui_forward(P, L, E, L.emb_user_int, L.emb_photo_int, idn[0], idn[2], lane, xu[1], Su[1], a1u[1], a2u[1]);
    const float ypc = dice_ui_forward(P, L, E, L.emb_user_con, L.emb_photo_con, idp[1], idp[3], lane, xu[2], Su[2], a1u[2], a2u[2]);
    const float ync = dice_ui_forward(P, L, E, L.emb_user_con, L.emb_photo_con, idn[1], idn[3], lane, xu[3], Su[3], a1u[3], a2u[3]);
    // ---- loss_kuaishou_DICE on this sample; every mean is over the n samples of the batch ------------------------------
    const float inv_n = 1.0f / (float)n;
    const float sc = c.score[row];
    const float w_int = sc < 0.f ? 1.0f : 0.0f;
    const float sg = 1.0f / (1.0f + expf(-(yp - yn)));      // sigmoid(y_pos - y_neg)
    const float sgc = 1.0f / (1.0f + expf(-(ypc - ync)));
    const float sgi = 1.0f / (1.0f + expf(-(ypi - yni)));
    const float err = yp - c.y[row];
    const float dyn = inv_n * (1.0f - sg);
    const float dyp = 2.0f * inv_n * err - dyn;
    const float dyc = inv_n * sc * (1.0f - sgc);            // d / d y_neg_con; the positive takes the opposite sign
    const float dyi = inv_n * w_int * (1.0f - sgi);
    if (lane == 0) {
        float* lp = o.LP + (size_t)i * 4;
        lp[0] = bad_row ? __builtin_nanf("") : err * err;
        lp[1] = -logf(sg);
        lp[2] = -(logf(sgc) * sc);
        lp[3] = -(logf(sgi) * w_int);
    }
    // ---- backward of the six forwards; the embedding rows one key receives from several forwards are added here, in this order ----
    const size_t nn = (size_t)n;
    tower_backward(P, L.main, 8, E, Km, dyp, lane, (size_t)i, xm[0], Sm[0], a1m[0], a2m[0], t64, dxs, o.m);
    for (int e = lane; e < 4 * E; e += CIRS_WAVE) acc[e] = dxs[e];                        // user_int, user_con, photo_int pos, photo_con pos
    write_feat_contrib(o.CF, o.KF, (size_t)i, E, fp, dxs, 4, dyp, lane);
    __builtin_amdgcn_wave_barrier();
    tower_backward(P, L.main, 8, E, Km, dyn, lane, nn + i, xm[1], Sm[1], a1m[1], a2m[1], t64, dxs, o.m);
    for (int e = lane; e < 2 * E; e += CIRS_WAVE) { acc[e] += dxs[e]; acc[4 * E + e] = dxs[2 * E + e]; }
    write_feat_contrib(o.CF, o.KF, nn + i, E, fn, dxs, 4, dyn, lane);
    if (lane == 0) { o.DUR[i] = dp; o.DUR[nn + i] = dn; }
    __builtin_amdgcn_wave_barrier();
    tower_backward(P, L.ui, 2, E, Ku, -dyi, lane, (size_t)i, xu[0], Su[0], a1u[0], a2u[0], t64, dxs, o.u);
    for (int e = lane; e < E; e += CIRS_WAVE) { acc[e] += dxs[e]; acc[2 * E + e] += dxs[E + e]; }
    __builtin_amdgcn_wave_barrier();
    tower_backward(P, L.ui, 2, E, Ku, dyi, lane, nn + i, xu[1], Su[1], a1u[1], a2u[1], t64, dxs, o.u);
    for (int e = lane; e < E; e += CIRS_WAVE) { acc[e] += dxs[e]; acc[4 * E + e] += dxs[E + e]; }
    __builtin_amdgcn_wave_barrier();
    tower_backward(P, L.ui, 2, E, Ku, -dyc, lane, 2 * nn + i, xu[2], Su[2], a1u[2], a2u[2], t64, dxs, o.u);
    for (int e = lane; e < E; e += CIRS_WAVE) { acc[E + e] += dxs[e]; acc[3 * E + e] += dxs[E + e]; }
    __builtin_amdgcn_wave_barrier();
    tower_backward(P, L.ui, 2, E, Ku, dyc, lane, 3 * nn + i, xu[3], Su[3], a1u[3], a2u[3], t64, dxs, o.u);
    for (int e = lane; e < E; e += CIRS_WAVE) { acc[E + e] += dxs[e]; acc[5 * E + e] += dxs[E + e]; }
    __builtin_amdgcn_wave_barrier();
    // contribution rows: [d embedding row | d linear_main weight | d linear_ui weight]
    const int W = E + 2;
    const float dym = dyp + dyn;   // both main rows read the same user ids
    for (int e = lane; e < W; e += CIRS_WAVE) {
        o.CUI[(size_t)i * W + e] = e < E ? acc[e] : (e == E ? dym : 0.f);              // linear_ui[user_int]: -dyi + dyi
        o.CUC[(size_t)i * W + e] = e < E ? acc[E + e] : (e == E ? dym : 0.f);          // linear_ui[user_con]: -dyc + dyc
        o.CPI[(size_t)i * W + e] = e < E ? acc[2 * E + e] : (e == E ? dyp : -dyi);
        o.CPC[(size_t)i * W + e] = e < E ? acc[3 * E + e] : (e == E ? dyp : -dyc);
        o.CPI[(nn + i) * W + e] = e < E ? acc[4 * E + e] : (e == E ? dyn : dyi);
        o.CPC[(nn + i) * W + e] = e < E ? acc[5 * E + e] : (e == E ? dyn : dyc);
    }
    if (lane == 0) {
        o.KUI[i] = (int32_t)idp[0]; o.KUC[i] = (int32_t)idp[1];
        o.KPI[i] = (int32_t)idp[2]; o.KPC[i] = (int32_t)idp[3];
        o.KPI[nn + i] = (int32_t)idn[2]; o.KPC[nn + i] = (int32_t)idn[3];
    }
}

// batch loss terms -> {loss, loss_y, bpr_click, bpr_con, bpr_int}
__global__ __launch_bounds__(256) void dice_loss_kernel(const float* __restrict__ LP, int n, float* __restrict__ loss_out) {
    float m[4];
    loss_means4(LP, n, m);
    if (threadIdx.x == 0) {
        const float ly = m[0], click = m[1], con = m[2], in = m[3];
        loss_out[0] = ((ly + click) + con) + in;
        loss_out[1] = ly; loss_out[2] = click; loss_out[3] = con; loss_out[4] = in;
    }
}

// UserModel_DICE.forward: the main DeepFM with the user and the photo id in both of their columns
__global__ __launch_bounds__(256) void dice_forward_kernel(cirs_dice_cfg cfg, const float* __restrict__ P, const int64_t* __restrict__ uid,
                                                           const int64_t* __restrict__ pid, const int32_t* __restrict__ feats,
                                                           const float* __restrict__ dur, long n, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int E = cfg.emb_dim;
    const DiceLayout L = dice_layout(cfg);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 4 + wv;
    if (i >= n) return;
    float* x = smem + (size_t)wv * dice_main_lds(E);
    float *S = x + 8 * E + 2, *a1 = S + E, *a2 = a1 + kTowerH;
    long u = uid[i], p = pid[i];
    int32_t f4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) f4[q] = feats[(size_t)i * 4 + q];
    // an id outside its table is not read: the row's prediction is NaN
    bool bad = u < 0 || u >= cfg.n_user_vocab || p < 0 || p >= cfg.n_item_vocab;
#pragma unroll
    for (int q = 0; q < 4; ++q) bad = bad || f4[q] < 0 || f4[q] >= cfg.n_feat_vocab;
    if (bad) {
        u = 0; p = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) f4[q] = 0;
    }
    const long ids[4] = {u, u, p, p};
    const float y = dice_main_forward(P, L, E, ids, f4, dur[i], lane, x, S, a1, a2);
    if (lane == 0) out[i] = bad ? __builtin_nanf("") : y;
}

// the workspace of a step on n samples: the size query runs this carve without a base pointer, the launch on the caller's workspace
struct DiceWs { DiceOut o; StepScratch x; };
static DiceWs dice_carve(Bump& w, int E, size_t n) {
    const size_t Rm = 2 * n, Ru = 4 * n;
    const int Km = 8 * E + 1, Ku = 2 * E;
    DiceWs t;
    DiceOut& o = t.o;
    o.m = tower_rows(w, Rm, Km); o.DUR = w.take(Rm);
    o.u = tower_rows(w, Ru, Ku);
    o.CUI = w.take(n * (E + 2)); o.CUC = w.take(n * (E + 2)); o.CPI = w.take(Rm * (E + 2)); o.CPC = w.take(Rm * (E + 2));
    o.CF = w.take(8 * n * (E + 1));
    o.KUI = (int32_t*)w.take(n); o.KUC = (int32_t*)w.take(n); o.KPI = (int32_t*)w.take(Rm); o.KPC = (int32_t*)w.take(Rm);
    o.KF = (int32_t*)w.take(8 * n);
    o.LP = w.take(4 * n + 8);
    const size_t pm = tower_partial_floats(Rm, Km), pu = tower_partial_floats(Ru, Ku);
    t.x = step_scratch(w, pm > pu ? pm : pu, 8 * n);
    return t;
}

static int dice_check_cfg(const cirs_dice_cfg* cfg) {
    if (cfg->hidden != kTowerH) return fail(CIRS_E_UNSUPPORTED, "dice: hidden == 64 only");
    if (cfg->emb_dim != 8 && cfg->emb_dim != 16 && cfg->emb_dim != 32) return fail(CIRS_E_UNSUPPORTED, "dice: emb_dim must be 8, 16 or 32");
    CIRS_REQUIRE(cfg->n_user_vocab >= 1 && cfg->n_item_vocab >= 1 && cfg->n_feat_vocab >= 1, "dice: empty vocabulary");
    return CIRS_OK;
}

// the launches of one step on the n samples order[r0 .. r0 + n) of the columns (rows r0 .. r0 + n - 1 when order is null)
static int dice_launch_step(const cirs_dice_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t step_before,
                            const DiceCols& c, const int64_t* order, long r0, long n_rows, int n, const TableHyper& h, float* loss_out,
                            void* workspace, hipStream_t s) {
    const int E = cfg->emb_dim, Km = 8 * E + 1, Ku = 2 * E, Rm = 2 * n, Ru = 4 * n;
    const DiceLayout L = dice_layout(*cfg);
    Bump w{(float*)workspace};
    const DiceWs ws = dice_carve(w, E, n);
    const DiceOut& o = ws.o;
    float* partial = ws.x.partial;
    // the data gradient is written sparsely (touched table rows, dense layers): start from zero
    CIRS_HIP(hipMemsetAsync(grads, 0, sizeof(float) * (size_t)L.total, s));
    const size_t shmem = sizeof(float) * 4 * (size_t)dice_wave_lds(E);
    hipLaunchKernelGGL(dice_rows_kernel, dim3(cdiv(n, 4)), dim3(256), shmem, s, *cfg, (const float*)params, c, order, r0, n_rows, n, o);
    CIRS_CHECK_LAUNCH("dice_rows_kernel");
    hipLaunchKernelGGL(dice_loss_kernel, dim3(1), dim3(256), 0, s, (const float*)o.LP, n, loss_out);
    // dense layers: dW = dY^T X over the 2n main rows and the 4n ui rows
    launch_tower_dw(o.m, Rm, Km, grads, L.main, true, partial, s);
    launch_dw_gemm(o.m.DY, 1, o.DUR, 1, Rm, 1, 1, grads + L.lm_dense, nullptr, partial, s);
    // out_ui.bias is in both forwards of every BPR difference: its data gradient is identically zero (the reference's cancels exactly),
    // so it is not summed from rounded terms -- Adam would turn that noise into +-lr steps
    launch_tower_dw(o.u, Ru, Ku, grads, L.ui, false, partial, s);
    CIRS_CHECK_LAUNCH("dice train dW");
    // table rows; linear_ui's two tables take the int pass, then the con pass on top of it
    const int U = cfg->n_user_vocab, I = cfg->n_item_vocab;
    ScatterDst dui{{grads + L.emb_user_int, grads + L.lm_user_int, grads + L.lu_user}, {E, 1, 1}, {0, 0, 0}};
    ScatterDst duc{{grads + L.emb_user_con, grads + L.lm_user_con, grads + L.lu_user}, {E, 1, 1}, {0, 0, 1}};
    ScatterDst dpi{{grads + L.emb_photo_int, grads + L.lm_photo_int, grads + L.lu_photo}, {E, 1, 1}, {0, 0, 0}};
    ScatterDst dpc{{grads + L.emb_photo_con, grads + L.lm_photo_con, grads + L.lu_photo}, {E, 1, 1}, {0, 0, 1}};
    ScatterDst df{{grads + L.emb_feat, grads + L.lm_feat, nullptr}, {E, 1, 0}, {0, 0, 0}};
    if (int rc = train_scatter(o.KUI, o.CUI, n, E + 2, U, dui, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    if (int rc = train_scatter(o.KUC, o.CUC, n, E + 2, U, duc, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    if (int rc = train_scatter(o.KPI, o.CPI, Rm, E + 2, I, dpi, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    if (int rc = train_scatter(o.KPC, o.CPC, Rm, E + 2, I, dpc, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    if (int rc = train_scatter(o.KF, o.CF, 8 * n, E + 1, cfg->n_feat_vocab, df, ws.x.sort, ws.x.sort_bytes, s)) return rc;
    L2Segs segs;
    segs.n = 3;
    for (int q = 0; q < 6; ++q) { segs.end[q] = L.total; segs.c[q] = h.l2_linear + h.l2_all; }
    segs.end[0] = L.lm_user_int;  segs.c[0] = h.l2_embedding + h.l2_all;   // embedding_dict.*            (core/user_model.py:57)
    segs.end[1] = L.unused;       segs.c[1] = h.l2_all;                      // linear_main, linear_ui, both towers (user_model_DICE.py:94)
    segs.end[2] = L.total;        segs.c[2] = h.l2_linear + h.l2_all;      // linear_model.* (unused in forward, still decays; :58)
    return table_adam_step(params, grads, adam_m, adam_v, L.total, segs, h, step_before, ws.x.regp, loss_out, 5, s);
}

}  // namespace cirs

extern "C" int64_t cirs_dice_train_param_count(const cirs_dice_cfg* cfg) {
    if (!cfg) return 0;
    return cirs::dice_layout(*cfg).total;
}

extern "C" int64_t cirs_dice_train_workspace_bytes(const cirs_dice_cfg* cfg, int32_t n) {
    if (!cfg || n <= 0) return 0;
    cirs::Bump w{nullptr};
    cirs::dice_carve(w, cfg->emb_dim, n);
    return (int64_t)(w.used * sizeof(float));
}

extern "C" int cirs_dice_train_epoch(const cirs_dice_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t step_before,
                                     const int64_t* uid_int, const int64_t* uid_con, const int64_t* pid_int, const int64_t* pid_con,
                                     const int32_t* feats_pos, const float* dur_pos, const int64_t* pid_int_neg, const int64_t* pid_con_neg,
                                     const int32_t* feats_neg, const float* dur_neg, const float* y, const float* score, int64_t n_rows,
                                     const int64_t* order, int64_t n_order, int32_t batch_size, float l2_embedding, float l2_linear,
                                     float l2_all, float lr, float beta1, float beta2, float eps, float* losses_out, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(cfg, "null argument");
    if (int rc = dice_check_cfg(cfg)) return rc;
    const int64_t bmax = batch_size < n_order ? batch_size : n_order;
    const DiceCols c{uid_int, uid_con, pid_int, pid_con, feats_pos, dur_pos, pid_int_neg, pid_con_neg, feats_neg, dur_neg, y, score};
    const TableHyper h{l2_embedding, l2_linear, l2_all, lr, beta1, beta2, eps};
    return tstep::run_steps(params, grads, adam_m, adam_v, losses_out, workspace,
                            uid_int && uid_con && pid_int && pid_con && feats_pos && dur_pos && pid_int_neg && pid_con_neg && feats_neg && dur_neg &&
                                y && score, "null data column",
                            n_rows >= 1 && n_order >= 1 && batch_size >= 1 && (order || n_order <= n_rows), "empty data set, index array or batch",
                            step_before, workspace_bytes, cirs_dice_train_workspace_bytes(cfg, (int32_t)bmax), n_order, batch_size,
                            [&](int64_t st, int64_t r0, int nb) {
                                return dice_launch_step(cfg, params, grads, adam_m, adam_v, step_before + st, c, order, r0, n_rows, nb, h,
                                                        losses_out + 6 * st, workspace, (hipStream_t)stream);
                            });
}

extern "C" int cirs_dice_forward(const cirs_dice_cfg* cfg, const float* params, const int64_t* uid, const int64_t* pid, const int32_t* feats,
                                 const float* dur, int64_t n, float* out, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(cfg && params && uid && pid && feats && dur && out, "null argument");
    if (int rc = dice_check_cfg(cfg)) return rc;
    CIRS_REQUIRE(n >= 0 && n <= (int64_t)4 * 0x7fffffff, "dice forward: row count out of range");
    if (n == 0) return CIRS_OK;
    const size_t shmem = sizeof(float) * 4 * (size_t)dice_main_lds(cfg->emb_dim);
    hipLaunchKernelGGL(dice_forward_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), shmem, (hipStream_t)stream, *cfg, params, uid, pid, feats, dur,
                       (long)n, out);
    CIRS_CHECK_LAUNCH("dice_forward_kernel");
    return CIRS_OK;
}
