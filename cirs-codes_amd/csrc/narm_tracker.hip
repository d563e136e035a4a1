// narm_tracker.hip -- StateTrackerNARM for gfx950: a GRU encoder whose hidden states are then attended over (NARM, Li et al., CIKM 2017).
//
// The reference has no counterpart; the model is defined here, in include/cirs_hip.h and in DESIGN.md 7.9:
//   inputs     the GRU tracker's slots, unchanged: x_0 = ffn_user(Emb_user[u]), x_k = sigmoid(fnn_gate([r_k, a_k])) * a_k
//   encoder    h_p = GRU cell(x_p, h_{p-1}), h_{-1} = 0: torch.nn.GRU(32, 32, 1), gate order r, z, n, both bias vectors
//   attention  for position p over j = 0 .. p (the whole session so far, position 0 and p itself included):
//                q_j = A2 h_j,  a_p = A1 h_p,  alpha_{p,j} = v . sigmoid(a_p + q_j)  (a scalar; no softmax),  c_p = sum_j alpha_{p,j} h_j
//   read-out   m_p = Bw [h_p ; c_p]  (Bw: 32 x 64; global = h_p, local = c_p);  s_p = decoder(m_p)
// One encoder layer: the cfg keeps the GRU tracker's nlayers member (one layout for both), any value but CIRS_NARM_MAX_LAYERS = 1 is refused.
//
// The j-walk (the same in the step kernel and in the three row kernels of the backward): a wavefront is (half, feature d) and takes TWO keys per pass,
// j = 2 i in half 0 and j = 2 i + 1 in half 1.  A lane reads q_j[d] and h_j[d] (one coalesced 128-byte row per half and array), forms v[d] sigmoid(a_p[d] +
// q_j[d]), the 32 lanes of the half add theirs with a five-step xor butterfly (every lane of the half ends with the same bits), and c[d] takes
// alpha h_j[d] with one fma.  A half adds its keys in ascending j; the two halves are joined at the end (half 0 + half 1, then -- in the step kernel --
// the new position's own term last).  Cost per position p: ceil((p + 1) / 2) passes of two loads, one sigmoid, five shuffles and one fma; the loads of
// four passes are issued together, so a dependent memory round trip is paid once per eight keys.
//
// Step (one launch appends one position for n envs): one env per wavefront, four per workgroup.  A workgroup stages the cell's two matrices and biases
// ([k][97] as in gru_tracker.hip), A1, A2 ([row][33]) and Bw ([row][65]) in LDS once -- 43 392 bytes, three workgroups per CU -- and walks several groups
// of four envs beyond 4 x 3 x CUs envs.  Per env: the slot, the cell on the carried h, a_p | q_p (one matrix per half), h_p and q_p appended to h_hist /
// q_hist (A2 is applied once per position, not once per pair), the j-walk over the stored positions, the read-out (h_p's columns of Bw in half 0, c_p's in
// half 1) and the decoder.  The time of a step grows linearly with the position (DESIGN.md 7.9 has the numbers).
//
// Backward (recompute-based over the buffer rows (env b, position p < len_b), env-major):
//   A  X = gather(x_hist);  Gi = X W_ih^T + b_ih                                  (rows_gemm)
//   B  gru_seq_fwd (gru_seq.h, the GRU tracker's) -> H and r, z, n, W_hn h + b_hn, h_prev per row
//   C  A_ = H A1^T,  Q = H A2^T                                                   (rows_gemm)
//   D  narm_attn_fwd, one row p per wavefront: c_p by the j-walk;  HC = [H | C];  M = HC Bw^T (rows_gemm)
//   E  G = gather(dstate);  dM = G W_dec and the decoder's gradients;  dHC = dM Bw and dBw = dM^T HC   (two rows_gemm + dw_gemm launches)
//   F  the attention's backward with e_{p,j} = sigmoid(a_p + q_j) recomputed, dalpha_{p,j} = dC_p . h_j, dpre_{p,j} = dalpha_{p,j} v * e (1 - e):
//        narm_attn_bwd_query, one query row p per wavefront, j ascending per half:  dA_p = sum_j dpre_{p,j};  DV_p = sum_j dalpha_{p,j} e_{p,j}
//        narm_attn_bwd_key,   one key row j per wavefront, p ascending per half:    dQ_j = sum_{p>=j} dpre_{p,j};  dHk_j = sum_{p>=j} alpha_{p,j} dC_p
//      dv = the column sums of DV (a 1 x 32 problem over a column of ones, through the slab partials);  dA1 = dA_^T H,  dA2 = dQ^T H
//   G  dH = dHC[:, :32] + dHk (written by the key kernel) + dA_ A1 + dQ A2        (two accumulating rows_gemm, each with its dw_gemm)
//   H  gru_seq_bwd(dH) -> dGi, dGh;  dW_ih, db_ih, dW_hh, db_hh (dw_batch);  dX = dGi W_ih;  the slot stage of the recurrent trackers (slot_tracker.h)
// Nothing per (p, j) pair is stored: the workspace is O(rows).  The pair kernels are plain fma, not MFMA tiles: the sigmoid of every (p, j, d) has to be
// formed lane by lane whichever way the products around it run, and it, not the 32-term dots, is what a pair costs.
// No floating-point atomics; every reduction has a fixed order.
#include <algorithm>
#include "gru_seq.h"

namespace cirs {

constexpr int nEnvsPerWg = 4;                              // one env (or buffer row) per wavefront
constexpr int nWgPerCu = 3;                                // 43 392 bytes of LDS per workgroup of the step kernel: three fit in a CU's 160 KB
constexpr int nLds = tD + 1;                               // LDS stride of a row of A1 / A2: 33
constexpr int nBwLds = 2 * tD + 1;                         // LDS stride of a row of Bw: 65
constexpr int nCellFloats = 2 * kGruMat + 2 * gG;          // W_ih^T | W_hh^T | b_ih | b_hh, as a layer of gru_step_kernel
constexpr int nBatch = 4;                                  // passes of the j-walk whose loads are issued together: eight keys in flight per wavefront

// the sum over the 32 lanes of a half-wavefront (xor 1 .. 16 stay inside the half): the same order, so the same bits, in every lane
__device__ __forceinline__ float narm_half_sum(float s) {
#pragma unroll
    for (int sft = 1; sft <= 16; sft <<= 1) s += __shfl_xor(s, sft, CIRS_WAVE);
    return s;
}

// (256, 3): three wavefronts per SIMD, what the LDS admits
__global__ __launch_bounds__(256, 3) void narm_step_kernel(cirs_narm_cfg cfg, cirs_narm_weights w, cirs_narm_state st, const int32_t* __restrict__ users,
                                                           const int64_t* __restrict__ items, const double* __restrict__ rew,
                                                           const int32_t* __restrict__ env_ids, const uint8_t* __restrict__ skip, int n,
                                                           float* __restrict__ state_out, long state_stride, int walks) {
    __shared__ float sCell[nCellFloats];
    __shared__ float sA[2 * tD * nLds];                    // A1, A2: [row][33]
    __shared__ float sBw[tD * nBwLds];                     // [row][65]
    __shared__ float sVec[nEnvsPerWg * 64];                // per wave: [0, 32) the vector under a product, [32, 64) its second half (previous h; c_p)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int d = lane & (tD - 1), half = lane >> 5;
    const int B = cfg.n_env, L = cfg.max_len, S = cfg.dim_state;
    // ---- once per workgroup: coalesced reads of the row-major matrices; the cell's are stored transposed ----
    for (int q = threadIdx.x; q < 2 * gG * tD; q += 256) {
        const int m = q >= gG * tD, i = q - m * gG * tD, o = i >> 5, k = i & 31;
        sCell[m * kGruMat + k * kGruLds + o] = (m ? w.w_hh : w.w_ih)[i];
    }
    for (int q = threadIdx.x; q < 2 * gG; q += 256) sCell[2 * kGruMat + q] = q < gG ? w.b_ih[q] : w.b_hh[q - gG];
    for (int q = threadIdx.x; q < 2 * tD * tD; q += 256) {
        const int m = q >= tD * tD, i = q - m * tD * tD;
        sA[m * tD * nLds + (i >> 5) * nLds + (i & 31)] = (m ? w.a2 : w.a1)[i];
    }
    for (int q = threadIdx.x; q < 2 * tD * tD; q += 256) sBw[(q >> 6) * nBwLds + (q & 63)] = w.bw[q];
    __syncthreads();
    float* vec = sVec + wv * 64;
    const bool is_init = users != nullptr;
    const float vd = w.v[d];
    for (int it_w = 0; it_w < walks; ++it_w) {
        const long j = ((long)blockIdx.x * walks + it_w) * nEnvsPerWg + wv;
        if (j >= n) break;                                 // wave-uniform, as every refusal below: only wave barriers follow
        const int e = env_ids ? env_ids[j] : (int)j;
        if (e < 0 || e >= B) continue;
        if (skip && skip[j]) continue;
        // ---- 1. the new input slot ----
        int pos = 0;
        float x;
        if (is_init) {
            const int u = users[j];
            if (u < 0 || u >= cfg.n_users) continue;
            if (lane < tD) vec[lane] = w.emb_user[(size_t)u * tD + lane];
            __builtin_amdgcn_wave_barrier();
            const float* fr = w.ffn_user_w + (size_t)d * tD;
            float acc = w.ffn_user_b[d];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(fr[k], vec[k], acc);
            x = acc;
        } else {
            const long it = items[j];
            if (it < 0 || it >= cfg.n_items) continue;      // act = -1: the env finished earlier in this rollout
            pos = st.len[e];
            if (pos < 1 || pos >= L) continue;              // never initialised / history full
            const float r = (float)rew[j];
            const float a = w.emb_item[(size_t)it * tD + d];
            if (lane < tD) vec[lane] = a;
            __builtin_amdgcn_wave_barrier();
            const float* gw = w.gate_w + (size_t)d * (tD + 1);      // input order [r, a_0..a_31]
            float acc = __builtin_fmaf(gw[0], r, w.gate_b[d]);
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(gw[1 + k], vec[k], acc);
            x = cell_sigmoid(acc) * a;
        }
        __builtin_amdgcn_wave_barrier();
        const size_t hist = ((size_t)e * L + pos) * tD + d;
        if (lane < tD) st.x_hist[hist] = x;
        // ---- 2. the cell (gru_step_kernel's): half 0 forms the three input dots of feature d, half 1 the three hidden dots ----
        float hnew;
        {
            float* hp = st.h + (size_t)e * tD;
            const float hprev = is_init ? 0.f : hp[d];
            vec[lane] = half ? hprev : x;
            __builtin_amdgcn_wave_barrier();
            const float* Wl = sCell + half * kGruMat + d;
            const float* bl = sCell + 2 * kGruMat + half * gG + d;
            const float* v = vec + half * tD;
            float g0 = bl[0], g1 = bl[tD], g2 = bl[2 * tD];
#pragma unroll
            for (int k = 0; k < tD; ++k) {
                const float vk = v[k];
                g0 = __builtin_fmaf(Wl[k * kGruLds], vk, g0);
                g1 = __builtin_fmaf(Wl[k * kGruLds + tD], vk, g1);
                g2 = __builtin_fmaf(Wl[k * kGruLds + 2 * tD], vk, g2);
            }
            const float o0 = __shfl_xor(g0, 32, CIRS_WAVE), o1 = __shfl_xor(g1, 32, CIRS_WAVE), o2 = __shfl_xor(g2, 32, CIRS_WAVE);
            const float gi_r = half ? o0 : g0, gh_r = half ? g0 : o0, gi_z = half ? o1 : g1, gh_z = half ? g1 : o1;
            const float gi_n = half ? o2 : g2, gh_n = half ? g2 : o2;
            const float r = cell_sigmoid(gi_r + gh_r), z = cell_sigmoid(gi_z + gh_z);
            const float nn = tanhf(gi_n + r * gh_n);
            hnew = (1.0f - z) * nn + z * hprev;
            __builtin_amdgcn_wave_barrier();
            if (lane < tD) hp[d] = hnew;
        }
        // ---- 3. a_p = A1 h_p in half 0, q_p = A2 h_p in half 1; both appended to the histories ----
        if (lane < tD) vec[lane] = hnew;
        __builtin_amdgcn_wave_barrier();
        float ap, qp;
        {
            const float* mat = sA + half * tD * nLds + d * nLds;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mat[k], vec[k], acc);
            const float other = __shfl_xor(acc, 32, CIRS_WAVE);
            ap = half ? other : acc;
            qp = half ? acc : other;
        }
        if (lane < tD) { st.h_hist[hist] = hnew; st.q_hist[hist] = qp; }
        // ---- 4. the j-walk over the stored positions j < p, two per pass; then the halves, then the new position's own term ----
        float c = 0.f;
        {
            const float* hh = st.h_hist + (size_t)e * L * tD + d;
            const float* qh = st.q_hist + (size_t)e * L * tD + d;
            for (int j0 = 0; j0 < pos; j0 += 2 * nBatch) {     // the loads of nBatch passes in flight, then their arithmetic in pass order
                float qv[nBatch], hv[nBatch];
#pragma unroll
                for (int u = 0; u < nBatch; ++u) {
                    const int jj = j0 + 2 * u + half;
                    qv[u] = jj < pos ? qh[(size_t)jj * tD] : 0.f;
                    hv[u] = jj < pos ? hh[(size_t)jj * tD] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < nBatch; ++u) {
                    if (j0 + 2 * u >= pos) break;          // wave-uniform
                    const float al = narm_half_sum(vd * cell_sigmoid(ap + qv[u]));
                    c = j0 + 2 * u + half < pos ? __builtin_fmaf(al, hv[u], c) : c;
                }
            }
            c += __shfl_xor(c, 32, CIRS_WAVE);             // a + b == b + a: both halves hold the same bits
            c = __builtin_fmaf(narm_half_sum(vd * cell_sigmoid(ap + qp)), hnew, c);
        }
        // ---- 5. m_p = Bw [h_p ; c_p]: h_p's columns in half 0, c_p's in half 1 ----
        if (lane < tD) vec[tD + lane] = c;
        __builtin_amdgcn_wave_barrier();
        float m;
        {
            const float* mat = sBw + d * nBwLds + half * tD;
            const float* v = vec + half * tD;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(mat[k], v[k], acc);
            m = acc + __shfl_xor(acc, 32, CIRS_WAVE);
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < tD) vec[lane] = m;
        __builtin_amdgcn_wave_barrier();
        // ---- 6. decoder ----
        if (lane < S) {
            const float* dr = w.dec_w + (size_t)lane * tD;
            float acc = w.dec_b[lane];
#pragma unroll
            for (int k = 0; k < tD; ++k) acc = __builtin_fmaf(dr[k], vec[k], acc);
            state_out[(size_t)j * state_stride + lane] = acc;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) st.len[e] = pos + 1;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// The three row kernels: one buffer row per wavefront, four per workgroup, lane (half, d); rows of an env are contiguous from offsets[b].

// (D) c_p by the j-walk over j = 0 .. p;  HC[r] = [h_p | c_p]
__global__ __launch_bounds__(256) void narm_attn_fwd(const float* __restrict__ A_, const float* __restrict__ Q, const float* __restrict__ H,
                                                     const float* __restrict__ v, const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t,
                                                     const int32_t* __restrict__ offsets, int R, float* __restrict__ HC) {
    const int lane = threadIdx.x & 63, d = lane & (tD - 1), half = lane >> 5;
    const long r = blockIdx.x * (long)nEnvsPerWg + (threadIdx.x >> 6);
    if (r >= R) return;
    const int p = row_t[r];
    const size_t base = (size_t)offsets[row_env[r]];
    const float ap = A_[(size_t)r * tD + d], vd = v[d];
    float c = 0.f;
    for (int j0 = 0; j0 <= p; j0 += 2 * nBatch) {
        float qv[nBatch], hv[nBatch];
#pragma unroll
        for (int u = 0; u < nBatch; ++u) {
            const int jj = j0 + 2 * u + half;
            const size_t o = (base + (jj <= p ? jj : 0)) * tD + d;
            qv[u] = Q[o]; hv[u] = H[o];
        }
#pragma unroll
        for (int u = 0; u < nBatch; ++u) {
            if (j0 + 2 * u > p) break;                     // wave-uniform
            const float al = narm_half_sum(vd * cell_sigmoid(ap + qv[u]));
            c = j0 + 2 * u + half <= p ? __builtin_fmaf(al, hv[u], c) : c;
        }
    }
    c += __shfl_xor(c, 32, CIRS_WAVE);
    HC[(size_t)r * 2 * tD + lane] = half ? c : H[(size_t)r * tD + d];
}

// (F, by query row p) dA_p = sum_j dpre_{p,j},  DV_p = sum_j dalpha_{p,j} e_{p,j};  ones[r] = 1 (the column the dv problem contracts DV with)
__global__ __launch_bounds__(256) void narm_attn_bwd_query(const float* __restrict__ A_, const float* __restrict__ Q, const float* __restrict__ H,
                                                           const float* __restrict__ v, const float* __restrict__ dHC,
                                                           const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t,
                                                           const int32_t* __restrict__ offsets, int R, float* __restrict__ dA, float* __restrict__ DV,
                                                           float* __restrict__ ones) {
    const int lane = threadIdx.x & 63, d = lane & (tD - 1), half = lane >> 5;
    const long r = blockIdx.x * (long)nEnvsPerWg + (threadIdx.x >> 6);
    if (r >= R) return;
    const int p = row_t[r];
    const size_t base = (size_t)offsets[row_env[r]];
    const float ap = A_[(size_t)r * tD + d], vd = v[d], dc = dHC[(size_t)r * 2 * tD + tD + d];
    float acc_a = 0.f, acc_v = 0.f;
    for (int j0 = 0; j0 <= p; j0 += 2 * nBatch) {
        float qv[nBatch], hv[nBatch];
#pragma unroll
        for (int u = 0; u < nBatch; ++u) {
            const int jj = j0 + 2 * u + half;
            const size_t o = (base + (jj <= p ? jj : 0)) * tD + d;
            qv[u] = Q[o]; hv[u] = H[o];
        }
#pragma unroll
        for (int u = 0; u < nBatch; ++u) {
            if (j0 + 2 * u > p) break;                     // wave-uniform
            const bool in = j0 + 2 * u + half <= p;
            const float e = cell_sigmoid(ap + qv[u]);
            const float da = narm_half_sum(dc * hv[u]);
            acc_a = in ? __builtin_fmaf(da * vd, e * (1.0f - e), acc_a) : acc_a;
            acc_v = in ? __builtin_fmaf(da, e, acc_v) : acc_v;
        }
    }
    acc_a += __shfl_xor(acc_a, 32, CIRS_WAVE);
    acc_v += __shfl_xor(acc_v, 32, CIRS_WAVE);
    (half ? DV : dA)[(size_t)r * tD + d] = half ? acc_v : acc_a;
    if (lane == 0) ones[r] = 1.0f;
}

// (F, by key row j) dQ_j = sum_{p >= j} dpre_{p,j},  dH_j = dHC[j, :32] + sum_{p >= j} alpha_{p,j} dC_p  (the read-out's and the context's share of dH)
__global__ __launch_bounds__(256) void narm_attn_bwd_key(const float* __restrict__ A_, const float* __restrict__ Q, const float* __restrict__ H,
                                                         const float* __restrict__ v, const float* __restrict__ dHC,
                                                         const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t,
                                                         const int32_t* __restrict__ offsets, const int32_t* __restrict__ lens, int R,
                                                         float* __restrict__ dQ, float* __restrict__ dH) {
    const int lane = threadIdx.x & 63, d = lane & (tD - 1), half = lane >> 5;
    const long r = blockIdx.x * (long)nEnvsPerWg + (threadIdx.x >> 6);
    if (r >= R) return;
    const int b = row_env[r], j = row_t[r], len = lens[b];
    const size_t base = (size_t)offsets[b];
    const float qj = Q[(size_t)r * tD + d], hj = H[(size_t)r * tD + d], vd = v[d];
    float acc_q = 0.f, acc_h = 0.f;
    for (int p0 = j; p0 < len; p0 += 2 * nBatch) {
        float av[nBatch], cv[nBatch];
#pragma unroll
        for (int u = 0; u < nBatch; ++u) {
            const int pp = p0 + 2 * u + half;
            const size_t row = base + (pp < len ? pp : j);
            av[u] = A_[row * tD + d]; cv[u] = dHC[row * 2 * tD + tD + d];
        }
#pragma unroll
        for (int u = 0; u < nBatch; ++u) {
            if (p0 + 2 * u >= len) break;                  // wave-uniform
            const bool in = p0 + 2 * u + half < len;
            const float e = cell_sigmoid(av[u] + qj);
            const float al = narm_half_sum(vd * e), da = narm_half_sum(cv[u] * hj);
            acc_q = in ? __builtin_fmaf(da * vd, e * (1.0f - e), acc_q) : acc_q;
            acc_h = in ? __builtin_fmaf(al, cv[u], acc_h) : acc_h;
        }
    }
    acc_q += __shfl_xor(acc_q, 32, CIRS_WAVE);
    acc_h += __shfl_xor(acc_h, 32, CIRS_WAVE);
    if (half) dQ[(size_t)r * tD + d] = acc_q;
    else dH[(size_t)r * tD + d] = dHC[(size_t)r * 2 * tD + d] + acc_h;
}

struct NarmScratch : SlotScratch {
    float *X, *Gi, *A_, *Q, *HC, *M, *G, *dM, *dHC, *dA, *dQ, *DV, *ones, *dH, *dGi, *dGh, *dX;
    GruRows rows;
};

// the pass's list: decoder (S <= 32), bilinear, attn.a1, attn.a2, attn.v, gru.weight_ih (+ bias), gru.weight_hh (+ bias), ffn_user, gate -- nine problems
static size_t narm_partial_floats(long R) {
    return dw_list_floats(R, 32, tD) + dw_list_floats(R, tD, 2 * tD) + 2 * dw_list_floats(R, tD, tD) + dw_list_floats(R, 1, tD) +
           2 * dw_list_floats(R, gG, tD) + dw_list_floats(R, tD, tD) + dw_list_floats(R, tD, tD + 1);
}

static NarmScratch carve_narm(void* ws, const cirs_narm_cfg* cfg, long R, size_t* total_floats) {
    Carver c(ws);
    NarmScratch s;
    s.X = c.take((size_t)R * tD); s.Gi = c.take((size_t)R * gG);
    GruRows& g = s.rows;
    g.r = c.take((size_t)R * tD); g.z = c.take((size_t)R * tD); g.n = c.take((size_t)R * tD); g.hn = c.take((size_t)R * tD);
    g.h = c.take((size_t)R * tD); g.hp = c.take((size_t)R * tD);
    s.A_ = c.take((size_t)R * tD); s.Q = c.take((size_t)R * tD); s.HC = c.take((size_t)R * 2 * tD); s.M = c.take((size_t)R * tD);
    s.G = c.take((size_t)R * 32); s.dM = c.take((size_t)R * tD); s.dHC = c.take((size_t)R * 2 * tD);
    s.dA = c.take((size_t)R * tD); s.dQ = c.take((size_t)R * tD); s.DV = c.take((size_t)R * tD); s.ones = c.take(R);
    s.dH = c.take((size_t)R * tD); s.dGi = c.take((size_t)R * gG); s.dGh = c.take((size_t)R * gG); s.dX = c.take((size_t)R * tD);
    carve_slots(c, s, R, cfg->n_env, narm_partial_floats(R));
    *total_floats = c.total();
    return s;
}

// the cfg first and on its own: a cfg outside the fixed sizes is refused before any pointer is read
static int validate_narm_cfg(const cirs_narm_cfg* cfg) {
    CIRS_SLOT_REQUIRE(cfg, "narm tracker", "cfg/weights null");
    if (int rc = validate_slot_dim_model(cfg, "narm tracker")) return rc;
    if (cfg->nlayers != CIRS_NARM_MAX_LAYERS) return slot_fail(CIRS_E_UNSUPPORTED, "narm tracker", "nlayers must be 1 (one encoder layer)");
    return validate_slot_sizes(cfg, "narm tracker");
}

static int validate_narm(const cirs_narm_cfg* cfg, const cirs_narm_weights* w) {
    if (int rc = validate_narm_cfg(cfg)) return rc;
    CIRS_SLOT_REQUIRE(w, "narm tracker", "cfg/weights null");
    if (int rc = validate_slot_weights(w, "narm tracker")) return rc;
    CIRS_SLOT_REQUIRE(w->w_ih && w->w_hh && w->b_ih && w->b_hh, "narm tracker", "encoder weight pointer null (w_ih / w_hh / b_ih / b_hh)");
    CIRS_SLOT_REQUIRE(w->a1 && w->a2 && w->v && w->bw, "narm tracker", "attention / read-out weight pointer null (a1 / a2 / v / bw)");
    return CIRS_OK;
}

static int launch_narm_step(const cirs_narm_cfg* cfg, const cirs_narm_weights* w, cirs_narm_state* st, const int32_t* users, const int64_t* items,
                            const double* rew, const int32_t* env_ids, const uint8_t* skip, int n, float* state_out, long state_stride, hipStream_t s) {
    CIRS_SLOT_REQUIRE(st && st->x_hist && st->h && st->h_hist && st->q_hist && st->len, "narm tracker", "state pointer null");
    // 43 392 bytes of LDS (42 KB of it the staged matrices): three workgroups per CU, three wavefronts per SIMD.  Up to 4 x 3 x CUs envs every env has a
    // wavefront of its own, beyond that a workgroup walks several groups of four and what it staged serves them all.  Chosen from the structure, not tuned.
    const int walks = slot_walks(n, nEnvsPerWg, nWgPerCu);
    hipLaunchKernelGGL(narm_step_kernel, dim3(cdiv(n, (long)nEnvsPerWg * walks)), dim3(256), 0, s, *cfg, *w, *st, users, items, rew, env_ids, skip, n,
                       state_out, state_stride, walks);
    CIRS_CHECK_LAUNCH("narm_step_kernel");
    return CIRS_OK;
}

}  // namespace cirs

extern "C" int cirs_narm_tracker_init(const cirs_narm_cfg* cfg, const cirs_narm_weights* w, cirs_narm_state* st, const int32_t* users,
                                      const int32_t* env_ids, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_init(cirs::validate_narm, cirs::launch_narm_step, cfg, w, st, users, env_ids, n, state_out, state_stride, stream);
}

extern "C" int cirs_narm_tracker_step(const cirs_narm_cfg* cfg, const cirs_narm_weights* w, cirs_narm_state* st, const int64_t* items, const double* rew,
                                      const int32_t* env_ids, const uint8_t* skip, int32_t n, float* state_out, int64_t state_stride, void* stream) {
    return cirs::slot_tracker_step(cirs::validate_narm, cirs::launch_narm_step, cfg, w, st, items, rew, env_ids, skip, n, state_out, state_stride, stream);
}

extern "C" int64_t cirs_narm_tracker_backward_workspace_bytes(const cirs_narm_cfg* cfg, int32_t n_rows) {
    return cirs::slot_tracker_workspace_bytes(cirs::validate_narm_cfg, cirs::carve_narm, cfg, n_rows);
}

extern "C" int cirs_narm_tracker_backward(const cirs_narm_cfg* cfg, const cirs_narm_weights* w, const cirs_narm_state* st, const int32_t* users,
                                          const int64_t* act, const double* rew, const int32_t* row_env, const int32_t* row_t, const int32_t* offsets,
                                          const int32_t* lens, int32_t n_rows, const float* dstate, const cirs_narm_grads* grads, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    if (int rc = validate_narm(cfg, w)) return rc;
    CIRS_REQUIRE(st && st->x_hist && users && act && rew && row_env && row_t && offsets && lens && dstate && grads && workspace, "null argument");
    CIRS_REQUIRE(n_rows > 0, "n_rows must be positive");
    if (int rc = validate_slot_grads(grads, "narm tracker")) return rc;
    CIRS_SLOT_REQUIRE(grads->w_ih && grads->w_hh && grads->b_ih && grads->b_hh && grads->a1 && grads->a2 && grads->v && grads->bw, "narm tracker",
                      "encoder / attention / read-out gradient pointer null");
    CIRS_REQUIRE(workspace_bytes >= cirs_narm_tracker_backward_workspace_bytes(cfg, n_rows), "workspace too small");
    CIRS_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = n_rows, B = cfg->n_env, S = cfg->dim_state, L = cfg->max_len;
    size_t total = 0;
    NarmScratch sc = carve_narm(workspace, cfg, R, &total);
    const dim3 rows_grid(cdiv(R, nEnvsPerWg));
    // ---- forward recompute: the encoder (A, B), the attention (C, D), the read-out ----
    hipLaunchKernelGGL(gather_x, dim3(cdiv((long)R * tD, 256)), dim3(256), 0, s, (const float*)st->x_hist, row_env, row_t, R, L, sc.X);
    launch_rows_gemm(true, sc.X, tD, w->w_ih, tD, w->b_ih, R, tD, gG, 0, nullptr, 0, sc.Gi, gG, s);
    hipLaunchKernelGGL(gru_seq_fwd, dim3(B), dim3(64), 0, s, (const float*)sc.Gi, w->w_hh, w->b_hh, offsets, lens, sc.rows);
    const float* H = sc.rows.h;
    launch_rows_gemm(true, H, tD, w->a1, tD, nullptr, R, tD, tD, 0, nullptr, 0, sc.A_, tD, s);
    launch_rows_gemm(true, H, tD, w->a2, tD, nullptr, R, tD, tD, 0, nullptr, 0, sc.Q, tD, s);
    hipLaunchKernelGGL(narm_attn_fwd, rows_grid, dim3(256), 0, s, (const float*)sc.A_, (const float*)sc.Q, H, w->v, row_env, row_t, offsets, R, sc.HC);
    launch_rows_gemm(true, sc.HC, 2 * tD, w->bw, 2 * tD, nullptr, R, 2 * tD, tD, 0, nullptr, 0, sc.M, tD, s);
    CIRS_CHECK_LAUNCH("narm tracker forward recompute");
    // ---- backward: decoder and read-out (E) ----
    DwList dwl{};
    hipLaunchKernelGGL(gather_dstate, dim3(cdiv((long)R * S, 256)), dim3(256), 0, s, dstate, row_env, row_t, R, S, B, sc.G);
    launch_rows_gemm_dw(dwl, sc.M, tD, S, tD, grads->dec_w, grads->dec_b, sc.partial, false, sc.G, S, w->dec_w, tD, nullptr, R, S, tD, 0, nullptr, 0, sc.dM,
                        tD, s);
    launch_rows_gemm_dw(dwl, sc.HC, 2 * tD, tD, 2 * tD, grads->bw, nullptr, sc.partial, false, sc.dM, tD, w->bw, 2 * tD, nullptr, R, tD, 2 * tD, 0, nullptr, 0,
                        sc.dHC, 2 * tD, s);
    // ---- the attention (F), then dH (G) ----
    hipLaunchKernelGGL(narm_attn_bwd_query, rows_grid, dim3(256), 0, s, (const float*)sc.A_, (const float*)sc.Q, H, w->v, (const float*)sc.dHC, row_env, row_t,
                       offsets, R, sc.dA, sc.DV, sc.ones);
    hipLaunchKernelGGL(narm_attn_bwd_key, rows_grid, dim3(256), 0, s, (const float*)sc.A_, (const float*)sc.Q, H, w->v, (const float*)sc.dHC, row_env, row_t,
                       offsets, lens, R, sc.dQ, sc.dH);
    CIRS_CHECK_LAUNCH("narm tracker backward attention");
    launch_rows_gemm_dw(dwl, H, tD, tD, tD, grads->a1, nullptr, sc.partial, false, sc.dA, tD, w->a1, tD, nullptr, R, tD, tD, 0, nullptr, 1, sc.dH, tD, s);
    launch_rows_gemm_dw(dwl, H, tD, tD, tD, grads->a2, nullptr, sc.partial, false, sc.dQ, tD, w->a2, tD, nullptr, R, tD, tD, 0, nullptr, 1, sc.dH, tD, s);
    // ---- the encoder (H): the GRU tracker's chain with dv riding in its weight-gradient batch ----
    hipLaunchKernelGGL(gru_seq_bwd, dim3(B), dim3(64), 0, s, (const float*)sc.dH, sc.rows, w->w_hh, offsets, lens, sc.dGi, sc.dGh);
    DwBatch bt{};
    dw_batch_add(bt, dwl, sc.ones, 1, sc.DV, tD, R, 1, tD, grads->v, nullptr, 0, sc.partial);
    dw_batch_add(bt, dwl, sc.dGi, gG, sc.X, tD, R, gG, tD, grads->w_ih, grads->b_ih, 0, sc.partial);
    dw_batch_add(bt, dwl, sc.dGh, gG, sc.rows.hp, tD, R, gG, tD, grads->w_hh, grads->b_hh, 0, sc.partial);
    dw_batch_launch(bt, R, s);
    launch_rows_gemm(false, sc.dGi, gG, w->w_ih, tD, nullptr, R, gG, tD, 0, nullptr, 0, sc.dX, tD, s);
    CIRS_CHECK_LAUNCH("narm tracker backward encoder");
    return slots_backward(cfg, w, grads, sc.dX, users, act, rew, row_env, row_t, lens, R, dwl, sc, s);
}
