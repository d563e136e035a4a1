// table_step.h -- the back half of an optimiser step over embedding tables, shared by the Kuaishou trainers (deepfm_train.hip: the
// pairwise / IPS / PD DeepFM; dice_train.hip: the DICE model).  Each trainer keeps its own row kernel and per-row contribution tables
// (the tower both row kernels run is in deepfm_tower.h); what follows them exists once, here:
//   Bump                the workspace as a bump allocator: a trainer writes its carve once and runs it without a base pointer for the
//                       size query and on the real pointer for the launches.
//   train_scatter       stable radix sort of (key, row) + ordered segment sums (no float atomics) of a contribution table [R, W] into up
//                       to three destination tables, each taking a column range of the contribution row; a destination either takes the
//                       segment sum (the gradient buffer starts from zero) or, marked `add`, adds it to what an earlier pass left.
//   adam_l2_kernel      g += 2 * l2_c * p (the regulariser is dense: every row of every table decays), Adam, and the regulariser's
//                       value as per-workgroup partials; reg_final_kernel sums them in index order into one slot of the loss vector;
//                       table_adam_step launches the pair with the bias corrections of the step count.  The corrections, the element
//                       update and the block sums are optim.h's (adam_bias through tstep::adam_args, adam_update, block_sum).
// Every sum has a fixed order: two runs give identical bits.
#pragma once
#include <hipcub/hipcub.hpp>

#include "common.h"
#include "train_step.h"

namespace cirs {
// ---- the workspace: floats handed out in order, each buffer a multiple of 16 bytes; base == nullptr only counts ----
struct Bump {
    float* base;
    size_t used = 0;
    float* take(size_t cnt) {
        float* r = base ? base + used : nullptr;
        used += (cnt + 3) & ~(size_t)3;
        return r;
    }
};

// ---- sorted scatter: contributions [R, W] keyed by row id -> up to three destination tables -----------------------
static __global__ __launch_bounds__(256) void train_keys_kernel(const int32_t* __restrict__ keys, int R, int n_table, uint32_t* __restrict__ k_out,
                                                         int32_t* __restrict__ rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int32_t k = keys[r];
    k_out[r] = (k < 0 || k >= n_table) ? (uint32_t)n_table : (uint32_t)k;
    rows[r] = r;
}

struct ScatterDst { float* p[3]; int w[3]; int add[3]; };  // column ranges of the contribution row -> table [n_table, w] each; add: += instead of =

static __global__ __launch_bounds__(256) void train_segment_sum_kernel(const uint32_t* __restrict__ ks, const int32_t* __restrict__ rs,
                                                                const float* __restrict__ contrib, int R, int W, int n_table, ScatterDst dst) {
    const int l = threadIdx.x & 31;
    const int pth = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (pth >= R) return;
    const uint32_t key = ks[pth];
    if (key >= (uint32_t)n_table || (pth > 0 && ks[pth - 1] == key)) return;  // not a segment head
    // segment length once (the 32 lanes scan cooperatively), then every lane streams its columns with 16 loads in flight
    int len = 0;
    for (int base = pth; base < R; base += 32) {
        const bool same = base + l < R && ks[base + l] == key;
        const unsigned long long m = __ballot(same) >> ((threadIdx.x & 32) ? 32 : 0) & 0xFFFFFFFFull;
        const int run = m == 0xFFFFFFFFull ? 32 : __builtin_ctzll(~m);
        len += run;
        if (run < 32) break;
    }
    for (int d = l; d < W; d += 32) {
        float acc = 0.f;
        for (int q0 = 0; q0 < len; q0 += 16) {
            float t16[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t16[u] = (q0 + u < len) ? contrib[(size_t)rs[pth + q0 + u] * W + d] : 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u) acc += t16[u];      // rows ascend inside a key: fixed order
        }
        int c = d;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (dst.p[t] && c < dst.w[t]) {
                float* out = dst.p[t] + (size_t)key * dst.w[t] + c;
                *out = dst.add[t] ? *out + acc : acc;
                break;
            }
            c -= dst.w[t];
        }
    }
}

static size_t train_sort_bytes(long R) { return (size_t)R * 64 + (1u << 20); }

static int train_scatter(const int32_t* keys, const float* contrib, int R, int W, int n_table, const ScatterDst& dst, void* scratch,
                         size_t scratch_bytes, hipStream_t s) {
    uint32_t* k_in = (uint32_t*)scratch;
    uint32_t* k_out = k_in + R;
    int32_t* r_in = (int32_t*)(k_out + R);
    int32_t* r_out = r_in + R;
    char* temp = (char*)(((uintptr_t)(r_out + R) + 255) & ~(uintptr_t)255);
    const size_t avail = scratch_bytes - (size_t)(temp - (char*)scratch);
    int end_bit = 1;
    while ((1u << end_bit) <= (uint32_t)n_table && end_bit < 32) ++end_bit;
    size_t need = 0;
    CIRS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, k_in, k_out, r_in, r_out, R, 0, end_bit, s));
    CIRS_REQUIRE(need <= avail, "train scatter: sort scratch too small");
    hipLaunchKernelGGL(train_keys_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, keys, R, n_table, k_in, r_in);
    CIRS_HIP(hipcub::DeviceRadixSort::SortPairs(temp, need, k_in, k_out, r_in, r_out, R, 0, end_bit, s));
    hipLaunchKernelGGL(train_segment_sum_kernel, dim3(cdiv(R, 8)), dim3(256), 0, s, k_out, r_out, contrib, R, W, n_table, dst);
    CIRS_CHECK_LAUNCH("train_segment_sum_kernel");
    return CIRS_OK;
}

// ---- regulariser + Adam over the whole flat buffer ----------------------------------------------------------------
struct L2Segs { long end[6]; float c[6]; int n; };  // element i belongs to the first segment with i < end

constexpr int kRegBlocks = 1024;
static __global__ __launch_bounds__(256) void adam_l2_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                      long n, L2Segs segs, float beta1, float beta2, float eps, float step_size, float bc2s,
                                                      float* __restrict__ reg_partial) {
    __shared__ float sh[256];
    const int tid = threadIdx.x;
    float reg = 0.f;
    for (long i = blockIdx.x * 256L + tid; i < n; i += (long)kRegBlocks * 256) {
        float c = segs.c[segs.n - 1];
#pragma unroll
        for (int q = 5; q >= 0; --q)
            if (q < segs.n && i < segs.end[q]) c = segs.c[q];
        float pi = p[i], mi = m[i], vi = v[i];
        reg = __builtin_fmaf(c * pi, pi, reg);
        const float gi = __builtin_fmaf(2.0f * c, pi, g[i]);   // d/dp of c * p^2 joins the data gradient
        adam_update(pi, mi, vi, gi, step_size, bc2s, beta1, beta2, eps);
        g[i] = gi; m[i] = mi; v[i] = vi; p[i] = pi;
    }
    reg = block_sum<256>(reg, sh);
    if (tid == 0) reg_partial[blockIdx.x] = reg;
}

static __global__ __launch_bounds__(256) void reg_final_kernel(const float* __restrict__ part, float* __restrict__ loss_out, int slot) {
    __shared__ float sh[256];
    const int tid = threadIdx.x;
    float t = 0.f;
    for (int q = tid; q < kRegBlocks; q += 256) t += part[q];
    t = block_sum<256>(t, sh);
    if (tid == 0) loss_out[slot] = t;
}

// what both trainers carve behind their row kernel's outputs: the dW slab partials, the regulariser partials, the sort scratch of the
// largest key space
struct StepScratch { float *partial, *regp; void* sort; size_t sort_bytes; };
inline StepScratch step_scratch(Bump& w, size_t partial_floats, long max_keys) {
    StepScratch t;
    t.partial = w.take(partial_floats + 64);
    t.regp = w.take(kRegBlocks + 8);
    t.sort_bytes = train_sort_bytes(max_keys);
    t.sort = (void*)w.take(t.sort_bytes / 4 + 64);
    return t;
}

struct TableHyper { float l2_embedding, l2_linear, l2_all, lr, beta1, beta2, eps; };

// regulariser + Adam (torch.optim.Adam, bias corrections from the step count) over the `total` parameters; the regulariser's value goes
// to loss_out[reg_slot].  regp: kRegBlocks floats
static int table_adam_step(float* params, float* grads, float* adam_m, float* adam_v, long total, const L2Segs& segs, const TableHyper& h,
                           int64_t step_before, float* regp, float* loss_out, int reg_slot, hipStream_t s) {
    const tstep::AdamArgs a = tstep::adam_args(h.lr, h.beta1, h.beta2, h.eps, h.l2_linear, h.l2_all, step_before);
    hipLaunchKernelGGL(adam_l2_kernel, dim3(kRegBlocks), dim3(256), 0, s, params, grads, adam_m, adam_v, total, segs, a.beta1, a.beta2, a.eps,
                       a.step_size, a.bc2s, regp);
    hipLaunchKernelGGL(reg_final_kernel, dim3(1), dim3(256), 0, s, (const float*)regp, loss_out, reg_slot);
    CIRS_CHECK_LAUNCH("adam_l2_kernel");
    return CIRS_OK;
}

}  // namespace cirs
