// vtb_mmoe.h -- UserModel_MMOE.forward (reference core/user_model_mmoe.py:232-262 over core/layers.py MMOELayer) for an all-dense
// model whose SHAPE IS A RUN-TIME ARGUMENT (cirs_vtb_mmoe_shape): 1..3 ReLU layers of width <= 256, experts * expert_dim <= 64, two
// regression tasks.  A device function over a tile of ROWS rows held in LDS, for kernels that run the model inside a longer chain
// (vtb_static.hip: one evaluation per launch).  mmoe_tile of virtualtb.hip stays the fixed-shape forward of the env step.
//
// Arithmetic: as mmoe_tile -- fp32 operands, every product and sum in fp64, one rounding to fp32 per layer output; the gate
// soft-max, the expert mix, the towers and the linear term in fp64, one rounding at the end.  The trunk is shared by the two tasks,
// so the click prediction's fp64 sums are the action features' sums too: there is no cheaper half to put on the matrix cores.
//
// A layer is a chain of K dependent fmas per output and nothing else runs meanwhile (one wavefront per SIMD), so a narrow layer
// (O * ROWS / 4 < 256 units) is split along K into S slices whose fp64 partial sums go through LDS and are added in slice order:
// the order of every sum is a function of the shape alone, never of timing.
#pragma once
#include "vtb_tile.h"

namespace cirs {
namespace {

constexpr int kMmMaxHidden = 256, kMmMaxED = 64, kMmOut = 28;   // 27 item features + 1 click prediction

template <int ROWS>
struct MmoeScratch {
    double part[kThreads * 4];          // split-K partial sums: [slice][row][column]
    double gate[ROWS][2][kMmMaxED];     // soft-max weights of the experts
    double mix[ROWS][2][kMmMaxED];      // experts @ gate
};

struct DenseSeg {
    const float* W;   // [K][O]
    const float* b;   // [O] or null
    int O;
};

// Y[r][c] = act(b[c] + sum_k X[r][k] W[k][c]) over the concatenated columns of up to three weight matrices that share the input.
template <int ROWS>
__device__ __forceinline__ void mmoe_dense(const DenseSeg (&seg)[3], int n_seg, const float* X, int ldx, int K, float* Y, int ldy,
                                           bool relu, double* part) {
    static_assert(ROWS % 4 == 0, "rows come in groups of four");
    constexpr int G = ROWS / 4;
    int O = 0;
    for (int i = 0; i < n_seg; ++i) O += seg[i].O;
    int S = 1;
    while (S < 8 && O * G * (2 * S) <= kThreads && K / (2 * S) >= 8) S *= 2;
    const int Kc = (K + S - 1) / S;
    for (int u = threadIdx.x; u < O * G * S; u += kThreads) {
        const int c = u % O, g = (u / O) % G, sl = u / (O * G);
        int o = c, si = 0;
        while (si + 1 < n_seg && o >= seg[si].O) { o -= seg[si].O; ++si; }
        const float* __restrict__ W = seg[si].W;
        const int ldw = seg[si].O;
        const float* x = X + 4 * g * ldx;
        const int k0 = sl * Kc, k1 = min(K, k0 + Kc);
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 8
        for (int k = k0; k < k1; ++k) {
            const double w = (double)W[(long)k * ldw + o];
            a0 = fma((double)x[k], w, a0);
            a1 = fma((double)x[ldx + k], w, a1);
            a2 = fma((double)x[2 * ldx + k], w, a2);
            a3 = fma((double)x[3 * ldx + k], w, a3);
        }
        if (S == 1) {
            const double bias = seg[si].b ? (double)seg[si].b[o] : 0.0;
            const float v[4] = {(float)(a0 + bias), (float)(a1 + bias), (float)(a2 + bias), (float)(a3 + bias)};
#pragma unroll
            for (int i = 0; i < 4; ++i) Y[(4 * g + i) * ldy + c] = relu ? fmaxf(v[i], 0.f) : v[i];
        } else {
            double* p = part + ((long)sl * ROWS + 4 * g) * O + c;
            p[0] = a0; p[O] = a1; p[2 * O] = a2; p[3 * O] = a3;
        }
    }
    __syncthreads();
    if (S == 1) return;
    for (int u = threadIdx.x; u < O * ROWS; u += kThreads) {
        const int c = u % O, r = u / O;
        int o = c, si = 0;
        while (si + 1 < n_seg && o >= seg[si].O) { o -= seg[si].O; ++si; }
        double a = part[(long)r * O + c];
        for (int sl = 1; sl < S; ++sl) a += part[((long)sl * ROWS + r) * O + c];
        const float v = (float)(a + (seg[si].b ? (double)seg[si].b[o] : 0.0));
        Y[r * ldy + c] = relu ? fmaxf(v, 0.f) : v;
    }
    __syncthreads();
}

// x: the ROWS inputs in LDS (row stride ldx, not modified); xa / xb: kLd-strided scratch rows; out[r][0..28) = the two tasks' logits
// in y_columns order.  Every thread of the workgroup calls it; it ends on a barrier.
template <int ROWS>
__device__ void mmoe_forward_tile(const cirs_vtb_mmoe_shape& sh, const cirs_vtb_mmoe_weights& w, const float* x, int ldx, float* xa,
                                  float* xb, MmoeScratch<ROWS>& S, float* out, int ldo) {
    const float* h = x;
    int ldh = ldx, K = sh.d_in;
    float* nxt = xa;
    for (int l = 0; l < sh.n_dnn; ++l) {
        const DenseSeg seg[3] = {{w.dnn_w[l], w.dnn_b[l], sh.hidden[l]}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
        mmoe_dense<ROWS>(seg, 1, h, ldh, K, nxt, kLd, true, S.part);
        h = nxt; ldh = kLd; K = sh.hidden[l];
        nxt = nxt == xa ? xb : xa;
    }
    const int E = sh.experts, D = sh.expert_dim, ED = E * D;
    {   // expert network and the two gates: one pass over the trunk's output
        const DenseSeg seg[3] = {{w.expert_w, w.expert_b, ED}, {w.gate_w[0], nullptr, E}, {w.gate_w[1], nullptr, E}};
        mmoe_dense<ROWS>(seg, 3, h, ldh, K, nxt, kLd, false, S.part);
    }
    const float* eg = nxt;
    if (threadIdx.x < ROWS * 2) {
        const int r = threadIdx.x >> 1, t = threadIdx.x & 1;
        const float* gl = eg + r * kLd + ED + t * E;
        float m = gl[0];
        for (int e = 1; e < E; ++e) m = fmaxf(m, gl[e]);
        double sum = 0.0;
        for (int e = 0; e < E; ++e) { const double p = exp((double)(gl[e] - m)); S.gate[r][t][e] = p; sum += p; }
        for (int e = 0; e < E; ++e) S.gate[r][t][e] /= sum;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < ROWS * 2 * D; u += kThreads) {
        const int d = u % D, t = (u / D) & 1, r = u / (2 * D);
        const float* ex = eg + r * kLd;
        double md = 0.0;
        for (int e = 0; e < E; ++e) md = fma((double)ex[d * E + e], S.gate[r][t][e], md);   // experts reshaped [expert_dim][experts]
        S.mix[r][t][d] = md;
    }
    __syncthreads();
    const int n0 = sh.task_dim[0], n_out = n0 + sh.task_dim[1];
    for (int u = threadIdx.x; u < ROWS * n_out; u += kThreads) {
        const int c = u % n_out, r = u / n_out;
        const int t = c >= n0, o = t ? c - n0 : c, dim = sh.task_dim[t];
        const float* wt = w.tower_w[t];
        double tower = 0.0;
        for (int d = 0; d < D; ++d) tower = fma(S.mix[r][t][d], (double)wt[d * dim + o], tower);
        if (dim == 1) {   // linear_model_task exists on the dim-1 task only
            double lin = 0.0;
            const float* xr = x + r * ldx;
            for (int k = 0; k < sh.d_in; ++k) lin = fma((double)xr[k], (double)w.lin_w[k], lin);
            tower = lin + tower;
        }
        out[r * ldo + c] = (float)(tower + (double)w.bias[t][o]);
    }
    __syncthreads();
}

}  // namespace
}  // namespace cirs
