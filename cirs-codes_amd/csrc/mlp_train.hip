// mlp_train.hip -- training of the VirtualTaobao two-task MLP baselines (MLP-taobao.py, MLP-epsilonGreedy-taobao.py) on the device:
//   cirs_mlp_train_step / _epoch    one optimiser step of UserModel_MMOE.fit_data's inner loop (reference core/user_model.py:150-170,
//                                   core/user_model_mmoe.py:144-233, loss_taobao of MLP-taobao.py:137-155) for the all-dense build with
//                                   the two regression tasks feat_item (27) and y (1), the SHAPE A RUN-TIME ARGUMENT (cirs_vtb_mmoe_shape:
//                                   everything cirs_vtb_static_eval plays can be trained).
//
// The step is TWO launches, like the one-task step of mmoe_train.hip:
//   mlp_rows_kernel        one workgroup per tile of 16 batch rows, activations in LDS.  Every dense product runs on the fp32 matrix
//                          cores (v_mfma_f32_16x16x4_f32, one 16-row tile = the M of the instruction): the hidden layers, the
//                          expert | gate | gate pass (ONE [ED + 2E, H] matrix), the two towers (a block-diagonal [2D, 28] operand), the
//                          linear term, and backwards d mix, d h_last and the pre-activation gradients of every hidden layer.  Widths
//                          that are no multiple of 16 are zero columns of the LDS planes (the whole LDS image is zeroed at entry);
//                          weight loads are predicated on the matrix's own bounds.  Soft-max, mix and the loss are per-row VALU code.
//                          Per-row operands of the weight gradients go to the workspace, the tile's two loss sums (fp64) to a partial.
//                          Eight more workgroups compute the regulariser of the CURRENT parameters as 64 fixed chunks (fp64).
//   grad_adam_kernel       (train_step.h, shared with mmoe_train.hip) dW = dZ^T A of the run-time job table built in launch_step on
//                          the matrix cores, bias gradients, g += 2 l2 p and torch.optim.Adam; its last workgroup decays the unused
//                          duplicate `linear_model.weight` and sums the two loss partials (A / 27 n + B / n) and the regulariser's.
// Every sum has a fixed order and there are no float atomics: two runs from one state give identical bits, and an epoch (the same two
// launches per step, queued back to back without host synchronisation) equals the step-by-step loop bit for bit.
#include "common.h"
#include "train_step.h"

namespace cirs {
namespace mlt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIn = CIRS_VTB_STATIC_STATE_DIM, kAct = 27, kOut = 28, kMaxL = CIRS_VTB_STATIC_MAX_DNN, kMaxH = 256, kMaxED = 64;
constexpr int kTile = 16, kThreads = 256;
static_assert(kThreads == tstep::kThreads, "reg_chunks runs in the row kernel's workgroups");
constexpr int kLdX = 100, kLdH = kMaxH + 4, kLdE = 3 * kMaxED + 4, kLdM = 2 * kMaxED + 4, kLdP = 36;   // LDS row strides (floats, multiples of 4)

struct Layout {  // offsets (floats) into the flat parameter / gradient / moment buffers
    int w[kMaxL], weg, b[kMaxL], be, wt, ob, lin_model, lin_task, total;
};
static Layout layout(const cirs_vtb_mmoe_shape& s) {
    Layout L{};
    int o = 0;
    const int n = s.n_dnn, ED = s.experts * s.expert_dim;
    for (int l = 1; l < n; ++l) { L.w[l] = o; o += s.hidden[l] * s.hidden[l - 1]; }
    L.weg = o; o += (ED + 2 * s.experts) * s.hidden[n - 1];
    L.w[0] = o; o += kIn * s.hidden[0];
    for (int l = 0; l < n; ++l) { L.b[l] = o; o += s.hidden[l]; }
    L.be = o; o += ED;
    L.wt = o; o += kOut * s.expert_dim;
    L.ob = o; o += kOut;
    L.lin_model = o; o += kIn;
    L.lin_task = o; o += kIn;
    L.total = o;
    return L;
}

struct Rows {  // per-row outputs of mlp_rows_kernel
    float *X, *H[kMaxL], *DZ[kMaxL], *DEG, *MIX, *DP;   // [n,91] [n,H_l] [n,H_l] [n,ED+2E] [n,2D] [n,28]
    double *loss_part, *reg_part;                       // [tiles][2] [tstep::kRegChunks]
};

struct RowsArgs {
    const float* P;
    cirs_vtb_mmoe_shape sh;
    Layout L;
    const float *x, *y;        // data rows [N,91], [N,28]
    const int64_t* idx;        // batch row r is data row idx[r0 + r] (null: r0 + r); rows outside [0, N) read row 0
    long r0, N;
    int n, n_tiles;
    float l2_linear, l2_all;
    Rows out;
};

// ---- B operands: loadB(k4, o) -> B[k4 .. k4 + 3][o], zero outside the matrix ------------------------------------------------------------
struct LoadNT {   // B[k][o] = W[o * K + k] (torch layout, forward); rows in float4 pieces where K and the base allow it
    const float* __restrict__ W;
    int K, O;
    bool vec;
    __device__ LoadNT(const float* w, int k, int o) : W(w), K(k), O(o), vec((k & 3) == 0 && ((uintptr_t)w & 15) == 0) {}
    __device__ __forceinline__ float4 operator()(int k4, int o) const {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < O && k4 < K) {
            const float* p = W + (size_t)o * K + k4;
            if (vec) {
                r = *reinterpret_cast<const float4*>(p);
            } else {
                r.x = p[0];
                if (k4 + 1 < K) r.y = p[1];
                if (k4 + 2 < K) r.z = p[2];
                if (k4 + 3 < K) r.w = p[3];
            }
        }
        return r;
    }
};
struct LoadNN {   // B[k][o] = W[k * ld + o]: lanes o read consecutive dwords
    const float* __restrict__ W;
    int ld, K, O;
    __device__ __forceinline__ float4 operator()(int k4, int o) const {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < O) {
            const float* p = W + (size_t)k4 * ld + o;
            if (k4 < K) r.x = p[0];
            if (k4 + 1 < K) r.y = p[ld];
            if (k4 + 2 < K) r.z = p[2 * ld];
            if (k4 + 3 < K) r.w = p[3 * ld];
        }
        return r;
    }
};
// the two towers as one block-diagonal operand: T[k][c], k over [mix_0 (D) | mix_1 (D)], c over the 28 outputs;
// Wt = tower_network.0.weight [27][D] | tower_network.1.weight [1][D]
__device__ __forceinline__ float tower_at(const float* __restrict__ Wt, int D, int k, int c) {
    if (k < D) return c < kAct ? Wt[c * D + k] : 0.f;
    return (k < 2 * D && c == kAct) ? Wt[kAct * D + (k - D)] : 0.f;
}
struct LoadTower {     // forward: B[k][c] = T[k][c]
    const float* __restrict__ Wt;
    int D;
    __device__ __forceinline__ float4 operator()(int k4, int c) const {
        if (c >= kOut) return make_float4(0.f, 0.f, 0.f, 0.f);
        return make_float4(tower_at(Wt, D, k4, c), tower_at(Wt, D, k4 + 1, c), tower_at(Wt, D, k4 + 2, c), tower_at(Wt, D, k4 + 3, c));
    }
};
struct LoadTowerT {    // backward: B[c][k] = T[k][c]
    const float* __restrict__ Wt;
    int D;
    __device__ __forceinline__ float at(int c, int k) const { return c < kOut ? tower_at(Wt, D, k, c) : 0.f; }
    __device__ __forceinline__ float4 operator()(int c4, int k) const {
        if (k >= 2 * D) return make_float4(0.f, 0.f, 0.f, 0.f);
        return make_float4(at(c4, k), at(c4 + 1, k), at(c4 + 2, k), at(c4 + 3, k));
    }
};

// D[16][O] = A[16][K] B on v_mfma_f32_16x16x4_f32; epi(row, col, value) for col < O; ends on a barrier.
// A: LDS rows of stride lda (a multiple of 4), columns [K, round16(K)) are zero.  The wave w owns the column tiles w, w + 4, w + 8, w + 12
// (O <= 256: four independent accumulators).  Lane (j = lane & 15, q = lane >> 4) supplies A[j][.] and B[.][16 ct + j]; of a block of 16
// contraction indices it holds 4 q .. 4 q + 3 (one ds_read_b128), MFMA i of the block contracts {i, 4 + i, 8 + i, 12 + i}: a fixed order.
template <class LB, class EP>
__device__ __forceinline__ void tile_mm(const float* A, int lda, int K, int O, LB loadB, EP epi) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int n_ct = (O + 15) >> 4, Kp = (K + 15) & ~15;
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < Kp; kk += 16) {
        const float4 a = *reinterpret_cast<const float4*>(A + j * lda + kk + 4 * q);
        float4 b[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = (wave + 4 * c < n_ct) ? loadB(kk + 4 * q, (wave + 4 * c) * 16 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (wave + 4 * c < n_ct) {   // wave-uniform
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[c].x, acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[c].y, acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[c].z, acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[c].w, acc[c], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int col = (wave + 4 * c) * 16 + j;
        if (col < O) {
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(4 * q + r, col, acc[c][r]);
        }
    }
    __syncthreads();
}

struct alignas(16) RowsSmem {
    float x[kTile * kLdX];
    float h[kMaxL][kTile * kLdH];               // layer outputs; overwritten in place by the pre-activation gradients on the way back
    float eg[kTile * kLdE], deg[kTile * kLdE];  // experts (column d * E + e) | gate logits of task 0 | of task 1;  their gradients
    float gate[kTile * 2 * kMaxED];             // soft-max weights [row][task * E + e]
    float mix[kTile * kLdM], dmix[kTile * kLdM];   // [row][task * D + d]
    float pred[kTile * kLdP], dpred[kTile * kLdP];
    float y[kTile * kOut], lin[kTile];
    double term[kTile * kOut];
};
static_assert(sizeof(RowsSmem) <= 160 * 1024, "one workgroup per CU");

__global__ __launch_bounds__(kThreads) void mlp_rows_kernel(RowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    RowsSmem& S = *reinterpret_cast<RowsSmem*>(smem_raw);
    const int tid = threadIdx.x;
    const float* __restrict__ P = a.P;
    const Layout& L = a.L;
    if ((int)blockIdx.x >= a.n_tiles) {
        tstep::reg_chunks(P, L.total, L.lin_model, L.lin_task, a.l2_linear, a.l2_all, a.n_tiles, reinterpret_cast<double*>(smem_raw), a.out.reg_part);
        return;
    }
    const cirs_vtb_mmoe_shape& sh = a.sh;
    const int nL = sh.n_dnn, E = sh.experts, D = sh.expert_dim, ED = E * D, EG = ED + 2 * E, HL = sh.hidden[nL - 1];
    const int n = a.n, row0 = blockIdx.x * kTile;
    {   // the padding columns of every MFMA operand plane must be zero: clear the whole image
        float4* z = reinterpret_cast<float4*>(smem_raw);
        for (int i = tid; i < (int)(sizeof(RowsSmem) / 16); i += kThreads) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    for (int i = tid; i < kTile * (kIn + kOut); i += kThreads) {
        const int s = i / (kIn + kOut), k = i % (kIn + kOut);
        if (row0 + s < n) {
            long src = a.idx ? (long)a.idx[a.r0 + row0 + s] : a.r0 + row0 + s;
            if (src < 0 || src >= a.N) src = 0;
            if (k < kIn) {
                const float v = a.x[src * kIn + k];
                a.out.X[(size_t)(row0 + s) * kIn + k] = v;
                S.x[s * kLdX + k] = v;
            } else {
                S.y[s * kOut + (k - kIn)] = a.y[src * kOut + (k - kIn)];
            }
        }
    }
    __syncthreads();
    // ---- forward ------------------------------------------------------------------------------------------------------------------------
    {
        const float* A = S.x;
        int lda = kLdX, K = kIn;
        for (int l = 0; l < nL; ++l) {
            const int O = sh.hidden[l];
            float* plane = S.h[l];
            float* Hout = a.out.H[l];
            const float* bias = P + L.b[l];
            auto epi = [&](int r, int c, float v) {
                v = fmaxf(v + bias[c], 0.f);
                plane[r * kLdH + c] = v;
                if (row0 + r < n) Hout[(size_t)(row0 + r) * O + c] = v;
            };
            if (l == 0) tile_mm(A, lda, K, O, LoadNN{P + L.w[0], O, K, O}, epi);     // layer 0 is stored transposed [91][H_0]
            else tile_mm(A, lda, K, O, LoadNT(P + L.w[l], K, O), epi);
            A = plane; lda = kLdH; K = O;
        }
        // experts and both gates' logits in one pass: the three matrices are one [ED + 2E][H_last] block of the parameter buffer
        tile_mm(A, lda, K, EG, LoadNT(P + L.weg, K, EG), [&](int r, int c, float v) { S.eg[r * kLdE + c] = c < ED ? v + P[L.be + c] : v; });
    }
    if (tid < kTile * 2) {   // gate soft-max per (row, task)
        const int r = tid >> 1, t = tid & 1;
        const float* gl = S.eg + r * kLdE + ED + t * E;
        float* g = S.gate + r * 2 * kMaxED + t * E;
        float mx = gl[0];
        for (int e = 1; e < E; ++e) mx = fmaxf(mx, gl[e]);
        float sum = 0.f;
        for (int e = 0; e < E; ++e) { const float p = expf(gl[e] - mx); g[e] = p; sum += p; }
        for (int e = 0; e < E; ++e) g[e] = g[e] / sum;
    }
    __syncthreads();
    for (int u = tid; u < kTile * 2 * D; u += kThreads) {   // mix[t][d] = sum_e experts[d][e] gate_t[e]
        const int c = u % (2 * D), r = u / (2 * D), t = c / D, d = c % D;
        const float* ex = S.eg + r * kLdE + d * E;
        const float* g = S.gate + r * 2 * kMaxED + t * E;
        float md = 0.f;
        for (int e = 0; e < E; ++e) md = __builtin_fmaf(ex[e], g[e], md);
        S.mix[r * kLdM + c] = md;
        if (row0 + r < n) a.out.MIX[(size_t)(row0 + r) * 2 * D + c] = md;
    }
    __syncthreads();
    tile_mm(S.mix, kLdM, 2 * D, kOut, LoadTower{P + L.wt, D}, [&](int r, int c, float v) { S.pred[r * kLdP + c] = v; });
    tile_mm(S.x, kLdX, kIn, 1, LoadNN{P + L.lin_task, 1, kIn, 1}, [&](int r, int, float v) { S.lin[r] = v; });   // linear_model_task: the dim-1 task only
    // ---- loss terms and d loss / d y_pred ---------------------------------------------------------------------------------------------
    for (int u = tid; u < kTile * kOut; u += kThreads) {
        const int r = u / kOut, c = u % kOut;
        float dp = 0.f;
        double term = 0.0;
        if (row0 + r < n) {
            const float click = S.y[r * kOut + kAct];
            if (c < kAct) {   // mse(click * pred, click * y) over n * 27 entries
                const float yp = S.pred[r * kLdP + c] + P[L.ob + c];
                const float diff = click * yp - click * S.y[r * kOut + c];
                term = (double)(diff * diff);
                dp = 2.0f * diff * click / (float)(kAct * n);
            } else {          // mse(pred, click) over n entries
                const float yp = (S.lin[r] + S.pred[r * kLdP + c]) + P[L.ob + c];
                const float diff = yp - click;
                term = (double)(diff * diff);
                dp = 2.0f * diff / (float)n;
            }
            a.out.DP[(size_t)(row0 + r) * kOut + c] = dp;
        }
        S.dpred[r * kLdP + c] = dp;
        S.term[u] = term;
    }
    __syncthreads();
    // ---- backward ---------------------------------------------------------------------------------------------------------------------
    tile_mm(S.dpred, kLdP, kOut, 2 * D, LoadTowerT{P + L.wt, D}, [&](int r, int c, float v) { S.dmix[r * kLdM + c] = v; });
    if (tid == 64) {   // the tile's loss sums: the 27 action columns row by row, the click column
        double ta = 0.0, tb = 0.0;
        for (int r = 0; r < kTile; ++r) {
            double row = 0.0;
            for (int c = 0; c < kAct; ++c) row += S.term[r * kOut + c];
            ta += row;
            tb += S.term[r * kOut + kAct];
        }
        a.out.loss_part[2 * blockIdx.x] = ta;
        a.out.loss_part[2 * blockIdx.x + 1] = tb;
    }
    for (int u = tid; u < kTile * ED; u += kThreads) {   // d experts[d][e] = sum_t d mix_t[d] gate_t[e]
        const int r = u / ED, c = u % ED, d = c / E, e = c % E;
        const float* g = S.gate + r * 2 * kMaxED;
        const float v = __builtin_fmaf(S.dmix[r * kLdM + D + d], g[E + e], S.dmix[r * kLdM + d] * g[e]);
        S.deg[r * kLdE + c] = v;
        if (row0 + r < n) a.out.DEG[(size_t)(row0 + r) * EG + c] = v;
    }
    if (tid < kTile * 2) {   // d gate logits per (row, task): soft-max backward of d gate_t[e] = sum_d d mix_t[d] experts[d][e]
        const int r = tid >> 1, t = tid & 1;
        const float* g = S.gate + r * 2 * kMaxED + t * E;
        const float* dm = S.dmix + r * kLdM + t * D;
        const float* ex = S.eg + r * kLdE;
        float dot = 0.f;
        for (int e = 0; e < E; ++e) {
            float dg = 0.f;
            for (int d = 0; d < D; ++d) dg = __builtin_fmaf(dm[d], ex[d * E + e], dg);
            dot = __builtin_fmaf(g[e], dg, dot);
        }
        for (int e = 0; e < E; ++e) {
            float dg = 0.f;
            for (int d = 0; d < D; ++d) dg = __builtin_fmaf(dm[d], ex[d * E + e], dg);
            const float v = g[e] * (dg - dot);
            S.deg[r * kLdE + ED + t * E + e] = v;
            if (row0 + r < n) a.out.DEG[(size_t)(row0 + r) * EG + ED + t * E + e] = v;
        }
    }
    __syncthreads();
    {   // d h_last = [d experts | d gate 0 | d gate 1] [We; Wg0; Wg1], then layer by layer; each through its relu, in place
        const float* A = S.deg;
        int lda = kLdE, K = EG;
        const float* W = P + L.weg;
        for (int l = nL - 1; l >= 0; --l) {
            const int O = sh.hidden[l];
            float* plane = S.h[l];
            float* DZout = a.out.DZ[l];
            tile_mm(A, lda, K, O, LoadNN{W, O, K, O}, [&](int r, int c, float v) {
                v = plane[r * kLdH + c] > 0.f ? v : 0.f;
                plane[r * kLdH + c] = v;
                if (row0 + r < n) DZout[(size_t)(row0 + r) * O + c] = v;
            });
            A = plane; lda = kLdH; K = O;
            W = P + L.w[l];     // torch layout [H_l][H_{l-1}]: the contraction runs over its rows
        }
    }
}

static int check_cfg(const cirs_mlp_train_cfg* cfg) {
    CIRS_REQUIRE(cfg, "null cfg");
    const cirs_vtb_mmoe_shape& s = cfg->shape;
    const char* what = "mlp train: only the static baselines' model is supported (all-dense UserModel_MMOE: 91 inputs, 1 to 3 hidden layers of "
                       "1 to 256, experts * expert_dim <= 64, the two regression tasks feat_item (27) and y (1))";
    if (s.d_in != kIn || s.n_dnn < 1 || s.n_dnn > kMaxL) return fail(CIRS_E_UNSUPPORTED, what);
    for (int l = 0; l < s.n_dnn; ++l)
        if (s.hidden[l] < 1 || s.hidden[l] > kMaxH) return fail(CIRS_E_UNSUPPORTED, what);
    if (s.experts < 1 || s.expert_dim < 1 || (long)s.experts * s.expert_dim > kMaxED) return fail(CIRS_E_UNSUPPORTED, what);
    if (s.n_tasks != 2 || s.task_dim[0] != kAct || s.task_dim[1] != 1) return fail(CIRS_E_UNSUPPORTED, what);
    return CIRS_OK;
}

static size_t pad4(size_t c) { return (c + 3) & ~(size_t)3; }

static size_t ws_floats(const cirs_vtb_mmoe_shape& s, long n) {
    const long tiles = (n + kTile - 1) / kTile;
    size_t t = pad4((size_t)n * kIn);
    for (int l = 0; l < s.n_dnn; ++l) t += 2 * pad4((size_t)n * s.hidden[l]);
    t += pad4((size_t)n * (s.experts * s.expert_dim + 2 * s.experts)) + pad4((size_t)n * 2 * s.expert_dim) + pad4((size_t)n * kOut);
    return t + pad4(4 * (size_t)tiles) + 2 * tstep::kRegChunks + 64;
}

// the two launches of one step on batch rows r0 .. r0 + n - 1 of the index array (or of the data when idx is null)
static int launch_step(const cirs_mlp_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v, int64_t step_before,
                       const float* x, const float* y, const int64_t* idx, long r0, long N, int n, float* loss_out, void* workspace,
                       hipStream_t s) {
    static bool lds_set = false;   // the tile's LDS image exceeds the 64 KB a kernel gets by default
    if (!lds_set) {
        CIRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)sizeof(RowsSmem)));
        lds_set = true;
    }
    const cirs_vtb_mmoe_shape& sh = cfg->shape;
    const Layout L = layout(sh);
    const int nL = sh.n_dnn, E = sh.experts, D = sh.expert_dim, ED = E * D, EG = ED + 2 * E, HL = sh.hidden[nL - 1];
    const int tiles = (n + kTile - 1) / kTile;
    float* p = (float*)workspace;
    auto take = [&](size_t cnt) { float* r = p; p += pad4(cnt); return r; };
    RowsArgs ra{};
    Rows& o = ra.out;
    o.X = take((size_t)n * kIn);
    for (int l = 0; l < nL; ++l) { o.H[l] = take((size_t)n * sh.hidden[l]); o.DZ[l] = take((size_t)n * sh.hidden[l]); }
    o.DEG = take((size_t)n * EG); o.MIX = take((size_t)n * 2 * D); o.DP = take((size_t)n * kOut);
    o.loss_part = (double*)take(4 * (size_t)tiles); o.reg_part = (double*)take(2 * tstep::kRegChunks);
    ra.P = params; ra.sh = sh; ra.L = L; ra.x = x; ra.y = y; ra.idx = idx; ra.r0 = r0; ra.N = N; ra.n = n; ra.n_tiles = tiles;
    ra.l2_linear = cfg->l2_linear; ra.l2_all = cfg->l2_all;
    hipLaunchKernelGGL(mlp_rows_kernel, dim3(tiles + tstep::kRegBlocks), dim3(kThreads), sizeof(RowsSmem), s, ra);
    CIRS_CHECK_LAUNCH("mlp_rows_kernel");
    tstep::Jobs jobs{};
    const int H0 = sh.hidden[0];
    tstep::add_job(jobs, o.DZ[0], H0, H0, o.X, kIn, kIn, L.w[0], 1, H0, L.b[0], H0);          // layer 0 is stored transposed: (o, k) at k * H_0 + o
    for (int l = 1; l < nL; ++l)
        tstep::add_job(jobs, o.DZ[l], sh.hidden[l], sh.hidden[l], o.H[l - 1], sh.hidden[l - 1], sh.hidden[l - 1], L.w[l], sh.hidden[l - 1], 1, L.b[l], sh.hidden[l]);
    tstep::add_job(jobs, o.DEG, EG, EG, o.H[nL - 1], HL, HL, L.weg, HL, 1, L.be, ED);         // experts | gate 0 | gate 1; only the experts have a bias
    tstep::add_job(jobs, o.DP, kOut, kAct, o.MIX, 2 * D, D, L.wt, D, 1, L.ob, kAct);          // tower 0 and out.0.bias
    tstep::add_job(jobs, o.DP + kAct, kOut, 1, o.MIX + D, 2 * D, D, L.wt + kAct * D, D, 1, L.ob + kAct, 1);   // tower 1 and out.1.bias
    tstep::add_job(jobs, o.DP + kAct, kOut, 1, o.X, kIn, kIn, L.lin_task, 0, 1, -1, 0);       // linear_model_task of the dim-1 task
    const tstep::Tail tail{L.lin_model, kIn, tiles, 2, {(double)n * kAct, (double)n}, o.loss_part, o.reg_part, loss_out};
    return tstep::launch_grad_adam(params, grads, adam_m, adam_v, jobs, n,
                                   tstep::adam_args(cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->l2_linear, cfg->l2_all, step_before), tail, s);
}

}  // namespace mlt
}  // namespace cirs

extern "C" int64_t cirs_mlp_train_param_count(const cirs_mlp_train_cfg* cfg) {
    if (cirs::mlt::check_cfg(cfg) != CIRS_OK) return 0;
    return cirs::mlt::layout(cfg->shape).total;
}

extern "C" int64_t cirs_mlp_train_workspace_bytes(const cirs_mlp_train_cfg* cfg, int32_t n) {
    if (n <= 0 || cirs::mlt::check_cfg(cfg) != CIRS_OK) return 0;
    return (int64_t)cirs::mlt::ws_floats(cfg->shape, n) * 4;
}

extern "C" int cirs_mlp_train_step(const cirs_mlp_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                                   int64_t step_before, const float* x, const float* y, int32_t n, float* loss_out, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = mlt::check_cfg(cfg)) return rc;
    return tstep::run_steps(params, grads, adam_m, adam_v, loss_out, workspace, x && y, "null batch column", n >= 1, "empty batch", step_before,
                            workspace_bytes, cirs_mlp_train_workspace_bytes(cfg, n), n, n, [&](int64_t, int64_t, int nb) {
                                return mlt::launch_step(cfg, params, grads, adam_m, adam_v, step_before, x, y, nullptr, 0, nb, nb, loss_out, workspace,
                                                        (hipStream_t)stream);
                            });
}

extern "C" int cirs_mlp_train_epoch(const cirs_mlp_train_cfg* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                                    int64_t step_before, const float* x, const float* y, int64_t n_rows, const int64_t* order,
                                    int64_t n_order, int32_t batch_size, float* losses_out, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    using namespace cirs;
    if (int rc = mlt::check_cfg(cfg)) return rc;
    const int64_t bmax = batch_size < n_order ? batch_size : n_order;
    return tstep::run_steps(params, grads, adam_m, adam_v, losses_out, workspace, x && y && order, "null data column or index array",
                            n_rows >= 1 && n_order >= 1 && batch_size >= 1, "empty data set, index array or batch", step_before, workspace_bytes,
                            cirs_mlp_train_workspace_bytes(cfg, (int32_t)bmax), n_order, batch_size, [&](int64_t st, int64_t r0, int nb) {
                                return mlt::launch_step(cfg, params, grads, adam_m, adam_v, step_before + st, x, y, order, r0, n_rows, nb,
                                                        losses_out + 2 * st, workspace, (hipStream_t)stream);
                            });
}
