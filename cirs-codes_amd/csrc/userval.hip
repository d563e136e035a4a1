// userval.hip -- the validation pass of the Kuaishou user models: forward over a resident data set fused with the error sums.
//   replaces  core/user_model.py:351-359 (evaluate_data), :361-399 (predict_data: the batch loop over the validation set and the
//             concatenation of the predictions) and the metric lambdas of the scripts (CIRS-UserModel-kuaishou.py:204-207,
//             DICE.py:236-239: mae / mse over all rows), for UserModel_Pairwise.forward (core/user_model_pairwise.py:98-129) and
//             UserModel_DICE.forward (core/user_model_DICE.py:189-192).
//
// validate_kernel<NF, E>   NF sparse fields of width E + the dense duration; NF = 6: the pairwise DeepFM (cirs_deepfm_weights), NF = 8:
//                          the main DeepFM of DICE with the user and the photo id in both of their columns (flat DICE buffer).
//   workgroup  4 wavefronts; W1 [64, NF E + 1], W2 [64, 64], b1, b2, last are staged into LDS once, then every wavefront walks its
//              tiles of 32 rows (tile = wave id + k * waves of the grid).
//   tile       field by field: the 32 embedding rows of the field are gathered once into LDS [32, E] and are the B operand of
//              H1^T [64, 32 rows] += W1[:, field] X_field^T on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, W1 from LDS as the A
//              operand); the same pass adds the field to the FM sums.  The next field's rows are in flight during the MFMAs.
//              H1^T leaves the matrix cores with the row on the lane and the 64 features in registers: relu(H1^T) is the B operand
//              of H2^T = W2 H1^T as it stands (contraction index relabelled like sweep_kernel of deepfm.hip, no LDS round trip).
//              last . relu(H2), linear logit, FM term, bias and the error terms are lane-local (one row per lane, two lane halves).
//   sums       e = (double)pred - y; every wavefront adds |e| and e^2 of its rows per lane in tile order, reduces them with the
//              butterfly once and writes one pair; validate_final_kernel adds the pairs in index order.  No atomics: two runs give
//              the same bits.
// Work: 2 * 64 * (NF E + 1 + 64) FLOP per row on the matrix cores (E = 16: 20.6 kFLOP pairwise, 24.7 kFLOP DICE) against the same
// count of scalar FMAs per wavefront and row, each with its own W load, in the per-row kernels; HBM: the id columns, y and (if asked
// for) 4 B of prediction per row.
#include "common.h"

namespace cirs {

constexpr int vH = 64;
constexpr int vTile = 32;
constexpr int vWaves = 4;
constexpr int vMaxBlocks = 1536;     // 6 per CU: a whole number of rounds at 1, 2 or 3 resident workgroups
constexpr int vFinalThreads = 256;
typedef float v_f32x16 __attribute__((ext_vector_type(16)));

template <int NF>
struct ValNet {
    const float* emb[NF];      // embedding table of sparse field f [V, E]
    const float* lin[NF];      // linear table of sparse field f [V]
    const float *lin_dense, *w1, *b1, *w2, *b2, *last, *out_bias;
};

// LDS floats: W1 [64][K] (K odd: conflict-free rows), W2 [64][65], b1, b2, last, per wave X [32][E + 1] and ids [32][NF]
template <int NF, int E>
constexpr int val_lds_floats() { return vH * (NF * E + 1) + vH * (vH + 1) + 3 * vH + vWaves * (vTile * (E + 1) + vTile * NF); }

template <int NF, int E>
__global__ __launch_bounds__(256) void validate_kernel(ValNet<NF> w, const int64_t* __restrict__ uid, const int64_t* __restrict__ pid,
                                                       const int32_t* __restrict__ feats, const float* __restrict__ dur,
                                                       const double* __restrict__ y, long n, float* __restrict__ pred_out,
                                                       double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int K = NF * E + 1, XL = E + 1, W2L = vH + 1, PER = vTile * E / CIRS_WAVE;   // PER: gathered values per lane and field
    float* sW1 = smem;
    float* sW2 = sW1 + vH * K;
    float* sB1 = sW2 + vH * W2L;
    float* sB2 = sB1 + vH;
    float* sLast = sB2 + vH;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int hi = lane >> 5, lo = lane & 31;
    float* sX = sLast + vH + wv * (vTile * XL + vTile * NF);
    int* sId = reinterpret_cast<int*>(sX + vTile * XL);
    for (int i = threadIdx.x; i < vH * K; i += blockDim.x) sW1[i] = w.w1[i];
    for (int i = threadIdx.x; i < vH * vH; i += blockDim.x) sW2[(i >> 6) * W2L + (i & 63)] = w.w2[i];
    if (threadIdx.x < vH) { sB1[threadIdx.x] = w.b1[threadIdx.x]; sB2[threadIdx.x] = w.b2[threadIdx.x]; sLast[threadIdx.x] = w.last[threadIdx.x]; }
    __syncthreads();
    const float w_dur = sW1[lo * K + K - 1], w_dur2 = sW1[(32 + lo) * K + K - 1];   // the duration column of W1, rows lo and 32 + lo
    const float lin_dense = w.lin_dense[0], out_bias = w.out_bias[0];
    const long n_tiles = (n + vTile - 1) / vTile;
    const long waves = (long)gridDim.x * vWaves;
    double sum_abs = 0.0, sum_sq = 0.0;
    for (long tile = (long)blockIdx.x * vWaves + wv; tile < n_tiles; tile += waves) {
        const long row0 = tile * vTile;
        // ids of the tile's rows (a row past the end repeats the last one: read and computed, never written or summed)
        for (int i = lane; i < vTile * NF; i += CIRS_WAVE) {
            const int r = i / NF, c = i % NF;
            const long row = row0 + r < n ? row0 + r : n - 1;
            const int src = NF == 6 ? c : (c < 2 ? 0 : (c < 4 ? 1 : c - 2));
            sId[i] = src == 0 ? (int)uid[row] : (src == 1 ? (int)pid[row] : feats[(size_t)row * 4 + (src - 2)]);
        }
        __builtin_amdgcn_wave_barrier();
        const long my_row = row0 + lo < n ? row0 + lo : n - 1;
        const float d = dur[my_row];
        float nxt[PER];
        // lane's gather slots: value q of the field is element (lane + 64 q) of the [32, E] block
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = lane + CIRS_WAVE * q;
            nxt[q] = w.emb[0][(size_t)sId[(i / E) * NF] * E + (i % E)];
        }
        v_f32x16 acc0, acc1;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int o = (s & 3) + 8 * (s >> 2) + 4 * hi;
            acc0[s] = sB1[o];
            acc1[s] = sB1[32 + o];
        }
        float fs[E / 2], fq = 0.f, logit = 0.f;
#pragma unroll
        for (int e = 0; e < E / 2; ++e) fs[e] = 0.f;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int i = lane + CIRS_WAVE * q;
                sX[(i / E) * XL + (i % E)] = nxt[q];
            }
            __builtin_amdgcn_wave_barrier();
            if (f + 1 < NF) {
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const int i = lane + CIRS_WAVE * q;
                    nxt[q] = w.emb[f + 1 < NF ? f + 1 : f][(size_t)sId[(i / E) * NF + f + 1] * E + (i % E)];
                }
            }
            logit += w.lin[f][sId[lo * NF + f]];
            // FM sums of row lo: lane half hi owns e in [hi E/2, (hi + 1) E/2)
#pragma unroll
            for (int e = 0; e < E / 2; ++e) {
                const float v = sX[lo * XL + hi * (E / 2) + e];
                fs[e] += v;
                fq = __builtin_fmaf(v, v, fq);
            }
            // H1^T[o][row] += W1[o][f E + k] X[row][k]: lane (lo, hi) gives A[o = lo (+32)][k = 2 t + hi], B[k = 2 t + hi][row = lo]
#pragma unroll
            for (int t = 0; t < E / 2; ++t) {
                const float b = sX[lo * XL + 2 * t + hi];
                const float a0 = sW1[lo * K + f * E + 2 * t + hi];
                const float a1 = sW1[(32 + lo) * K + f * E + 2 * t + hi];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // the dense column: k = K - 1 on lane half 0, nothing on half 1
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(hi ? 0.f : w_dur, hi ? 0.f : d, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(hi ? 0.f : w_dur2, hi ? 0.f : d, acc1, 0, 0, 0);
        // second layer: k-step t of lane half hi is feature o(t, hi) = 32 (t >> 4) + (s & 3) + 8 (s >> 2) + 4 hi, s = t & 15 -- the
        // feature register s of acc0 / acc1 holds for this lane's row
        v_f32x16 h0, h1;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int o = (s & 3) + 8 * (s >> 2) + 4 * hi;
            h0[s] = sB2[o];
            h1[s] = sB2[32 + o];
        }
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int s = t & 15;
            const int k = 32 * (t >> 4) + (s & 3) + 8 * (s >> 2) + 4 * hi;
            const float b = fmaxf(t < 16 ? acc0[s] : acc1[s], 0.f);
            h0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sW2[lo * W2L + k], b, h0, 0, 0, 0);
            h1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sW2[(32 + lo) * W2L + k], b, h1, 0, 0, 0);
        }
        float part = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int o = (s & 3) + 8 * (s >> 2) + 4 * hi;
            part = __builtin_fmaf(sLast[o], fmaxf(h0[s], 0.f), part);
            part = __builtin_fmaf(sLast[32 + o], fmaxf(h1[s], 0.f), part);
        }
        float cross = -fq;
#pragma unroll
        for (int e = 0; e < E / 2; ++e) cross = __builtin_fmaf(fs[e], fs[e], cross);
        part += __shfl_xor(part, 32, CIRS_WAVE);
        cross += __shfl_xor(cross, 32, CIRS_WAVE);
        logit += d * lin_dense;
        const float pred = (logit + 0.5f * cross) + (part + out_bias);
        if (hi == 0 && row0 + lo < n) {
            if (pred_out) pred_out[row0 + lo] = pred;
            if (partial) {
                const double e = (double)pred - y[row0 + lo];
                sum_abs += fabs(e);
                sum_sq += e * e;
            }
        }
    }
    if (partial) {
        sum_abs = wave_sum_f64(sum_abs);
        sum_sq = wave_sum_f64(sum_sq);
        if (lane == 0) {
            const size_t slot = (size_t)blockIdx.x * vWaves + wv;
            partial[2 * slot] = sum_abs;
            partial[2 * slot + 1] = sum_sq;
        }
    }
}

// {sum |e|, sum e^2} over the per-wavefront pairs: thread i adds the pairs i, i + 256, ... in index order, then a fixed tree
__global__ __launch_bounds__(vFinalThreads) void validate_final_kernel(const double* __restrict__ partial, long n_slots, double* __restrict__ sums) {
    __shared__ double sa[vFinalThreads], sq[vFinalThreads];
    const int tid = threadIdx.x;
    double a = 0.0, q = 0.0;
    for (long i = tid; i < n_slots; i += vFinalThreads) { a += partial[2 * i]; q += partial[2 * i + 1]; }
    sa[tid] = a; sq[tid] = q;
    __syncthreads();
    for (int s = vFinalThreads / 2; s > 0; s >>= 1) {
        if (tid < s) { sa[tid] += sa[tid + s]; sq[tid] += sq[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { sums[0] = sa[0]; sums[1] = sq[0]; }
}

static long val_blocks(long n) {
    const long b = (n + vTile * vWaves - 1) / (vTile * vWaves);
    return b < vMaxBlocks ? b : vMaxBlocks;
}

static int64_t val_workspace_bytes(long n) { return n < 1 ? 0 : (int64_t)(val_blocks(n) * vWaves * 2 * sizeof(double)); }

template <int NF, int E>
static int val_launch(const ValNet<NF>& w, const int64_t* uid, const int64_t* pid, const int32_t* feats, const float* dur, const double* y, long n,
                      float* pred_out, double* partial, hipStream_t s) {
    constexpr size_t shmem = sizeof(float) * (size_t)val_lds_floats<NF, E>();
    static_assert(shmem <= 160 * 1024, "the staged weights and the four tiles must fit the CU's LDS");
    static bool lds_set = false;   // W1 alone can exceed the 64 KB a kernel gets by default
    if (!lds_set) {
        CIRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&validate_kernel<NF, E>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        lds_set = true;
    }
    hipLaunchKernelGGL((validate_kernel<NF, E>), dim3((unsigned)val_blocks(n)), dim3(64 * vWaves), shmem, s, w, uid, pid, feats, dur, y, n, pred_out,
                       partial);
    CIRS_CHECK_LAUNCH("validate_kernel");
    return CIRS_OK;
}

template <int NF>
static int val_run(int E, const ValNet<NF>& w, const int64_t* uid, const int64_t* pid, const int32_t* feats, const float* dur, const double* y,
                   int64_t n, float* pred_out, double* sums_out, void* workspace, int64_t workspace_bytes, void* stream) {
    CIRS_REQUIRE(n >= 1, "validate: empty data set");
    CIRS_REQUIRE(uid && pid && feats && dur, "validate: null data column");
    CIRS_REQUIRE(pred_out || sums_out, "validate: neither predictions nor sums asked for");
    CIRS_REQUIRE(!sums_out || y, "validate: the sums need y");
    CIRS_REQUIRE(!sums_out || (workspace && workspace_bytes >= val_workspace_bytes(n)), "validate: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    double* partial = sums_out ? (double*)workspace : nullptr;
    int rc;
    switch (E) {
        case 8: rc = val_launch<NF, 8>(w, uid, pid, feats, dur, y, n, pred_out, partial, s); break;
        case 16: rc = val_launch<NF, 16>(w, uid, pid, feats, dur, y, n, pred_out, partial, s); break;
        case 32: rc = val_launch<NF, 32>(w, uid, pid, feats, dur, y, n, pred_out, partial, s); break;
        default:
            if constexpr (NF == 6) { rc = val_launch<NF, 64>(w, uid, pid, feats, dur, y, n, pred_out, partial, s); break; }
            return fail(CIRS_E_UNSUPPORTED, "validate: emb_dim not supported");
    }
    if (rc) return rc;
    if (sums_out) {
        hipLaunchKernelGGL(validate_final_kernel, dim3(1), dim3(vFinalThreads), 0, s, (const double*)partial, val_blocks(n) * vWaves, sums_out);
        CIRS_CHECK_LAUNCH("validate_final_kernel");
    }
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int64_t cirs_deepfm_validate_workspace_bytes(const cirs_deepfm_cfg* cfg, int64_t n) {
    return cfg ? cirs::val_workspace_bytes(n) : 0;
}

extern "C" int cirs_deepfm_validate(const cirs_deepfm_cfg* cfg, const cirs_deepfm_weights* w, const int64_t* uid, const int64_t* pid,
                                    const int32_t* feats, const float* dur, const double* y, int64_t n, float* pred_out, double* sums_out,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(cfg && w, "deepfm cfg/weights null");
    if (cfg->hidden != vH) return fail(CIRS_E_UNSUPPORTED, "deepfm: hidden == 64 only");
    if (!(cfg->emb_dim == 8 || cfg->emb_dim == 16 || cfg->emb_dim == 32 || cfg->emb_dim == 64))
        return fail(CIRS_E_UNSUPPORTED, "deepfm: emb_dim must be 8, 16, 32 or 64");
    CIRS_REQUIRE(w->emb_user && w->emb_item && w->emb_feat && w->lin_user && w->lin_item && w->lin_feat && w->lin_dense && w->w1 && w->b1 && w->w2 &&
                     w->b2 && w->last && w->out_bias, "deepfm weight pointer null");
    const ValNet<6> net{{w->emb_user, w->emb_item, w->emb_feat, w->emb_feat, w->emb_feat, w->emb_feat},
                        {w->lin_user, w->lin_item, w->lin_feat, w->lin_feat, w->lin_feat, w->lin_feat},
                        w->lin_dense, w->w1, w->b1, w->w2, w->b2, w->last, w->out_bias};
    return val_run<6>(cfg->emb_dim, net, uid, pid, feats, dur, y, n, pred_out, sums_out, workspace, workspace_bytes, stream);
}

extern "C" int64_t cirs_dice_validate_workspace_bytes(const cirs_dice_cfg* cfg, int64_t n) {
    return cfg ? cirs::val_workspace_bytes(n) : 0;
}

extern "C" int cirs_dice_validate(const cirs_dice_cfg* cfg, const float* params, const int64_t* uid, const int64_t* pid, const int32_t* feats,
                                  const float* dur, const double* y, int64_t n, float* pred_out, double* sums_out, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(cfg && params, "dice cfg/params null");
    if (cfg->hidden != vH) return fail(CIRS_E_UNSUPPORTED, "dice: hidden == 64 only");
    if (cfg->emb_dim != 8 && cfg->emb_dim != 16 && cfg->emb_dim != 32) return fail(CIRS_E_UNSUPPORTED, "dice: emb_dim must be 8, 16 or 32");
    CIRS_REQUIRE(cfg->n_user_vocab >= 1 && cfg->n_item_vocab >= 1 && cfg->n_feat_vocab >= 1, "dice: empty vocabulary");
    // the head of the flat buffer, in the order of dice_layout() (dice_train.hip; include/cirs_hip.h lists it)
    const long U = cfg->n_user_vocab, I = cfg->n_item_vocab, F = cfg->n_feat_vocab, E = cfg->emb_dim;
    const float* p = params;
    auto take = [&](long cnt) { const float* r = p; p += cnt; return r; };
    const float *eui = take(U * E), *euc = take(U * E), *epi = take(I * E), *epc = take(I * E), *ef = take(F * E);
    const float *lui = take(U), *luc = take(U), *lpi = take(I), *lpc = take(I), *lf = take(F), *ld = take(1);
    take(U + I);   // linear_ui
    const float *w1 = take(vH * (8 * E + 1)), *b1 = take(vH), *w2 = take(vH * vH), *b2 = take(vH), *last = take(vH), *ob = take(1);
    const ValNet<8> net{{eui, euc, epi, epc, ef, ef, ef, ef}, {lui, luc, lpi, lpc, lf, lf, lf, lf}, ld, w1, b1, w2, b2, last, ob};
    return val_run<8>(cfg->emb_dim, net, uid, pid, feats, dur, y, n, pred_out, sums_out, workspace, workspace_bytes, stream);
}
