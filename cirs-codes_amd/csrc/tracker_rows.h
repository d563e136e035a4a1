// tracker_rows.h -- what the backward passes of the Transformer tracker (tracker_bwd.hip) and of the seven slot trackers (through slot_tracker.h: gru_, lstm_,
// avg_, caser_, nextitnet_, stamp_, narm_tracker.hip) run on the buffer rows:
//   dw_batch_*            several weight-gradient problems over the same rows in one launch (slab partials, summed by dw_list_final)
//   gather_dstate         upstream gradient rows from dstate [T+1, B, S]
//   slot_bwd              backward of the input slots (user projection / gated action) down to the per-row embedding contributions
//   emb_scatter_*         ordered, atomic-free scatter of those contributions into the embedding-gradient tables
#pragma once
#include <hipcub/hipcub.hpp>
#include "small_gemm.h"
#include "internal.h"

namespace cirs {
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int tD = 32, tH = 128;   // dim_model, the Transformer's d_hid

// every weight-gradient problem of a layer in one launch: grid = (sum of the problems' 32 x 32 output tiles, row slabs), the slab
// partials go to each problem's own region (summed by dw_list_final at the end of the pass, like every other problem)
constexpr int kMaxDwBatch = 8;
struct DwBatchJob { const float* dY; int ldy; const float* X; int ldx; int O, K, tile_begin; float* partial; };
struct DwBatch { DwBatchJob j[kMaxDwBatch]; int n, total_tiles; };
static __global__ __launch_bounds__(64) void dw_batch_kernel(DwBatch jobs, int R, int rows_per_slab) {
    int ji = 0;
    for (; ji + 1 < jobs.n && (int)blockIdx.x >= jobs.j[ji + 1].tile_begin; ++ji) {}
    const DwBatchJob& jb = jobs.j[ji];
    dw_gemm_body((int)blockIdx.x - jb.tile_begin, blockIdx.y, jb.dY, jb.ldy, jb.X, jb.ldx, R, jb.O, jb.K, rows_per_slab, jb.partial);
}
static inline void dw_batch_add(DwBatch& b, DwList& list, const float* dY, int ldy, const float* X, int ldx, int R, int O, int K, float* dW,
                                float* db, int diag, float* partial) {
    const int slabs = dwg_slabs(R);
    DwListJob& lj = list.j[list.n++];
    lj.O = O; lj.K = K; lj.part_off = list.part_floats; lj.diag = diag; lj.dW = dW; lj.db = db;
    DwBatchJob& jb = b.j[b.n++];
    jb.dY = dY; jb.ldy = ldy; jb.X = X; jb.ldx = ldx; jb.O = O; jb.K = K; jb.tile_begin = b.total_tiles; jb.partial = partial + lj.part_off;
    b.total_tiles += cdiv(O, 32) * cdiv(K, 32);
    list.part_floats += slabs * O * (K + 1);
    list.total_out += O * (K + 1);
}
// (R_rows < R: problems over the first R_rows rows only -- the last-row pass -- in the slab count of the R-row problems of the same pass, which is the one
// dw_list_final walks; slabs beyond the rows write zero partials)
static inline void dw_batch_launch(const DwBatch& b, int R, hipStream_t s, int R_rows = -1) {
    if (!b.n) return;
    if (R_rows < 0) R_rows = R;
    const int slabs = dwg_slabs(R);
    int rows_per_slab = (R_rows + slabs - 1) / slabs;
    rows_per_slab = (rows_per_slab + 15) & ~15;
    hipLaunchKernelGGL(dw_batch_kernel, dim3(b.total_tiles, slabs), dim3(64), 0, s, b, R_rows, rows_per_slab);
}

// upstream gradient rows: G[r, s] = dstate[row_t, row_env, s]
static __global__ __launch_bounds__(256) void gather_dstate(const float* __restrict__ dstate, const int32_t* __restrict__ row_env,
                                                     const int32_t* __restrict__ row_t, int R, int S, int B, float* __restrict__ G) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)R * S) return;
    const int r = (int)(i / S), s = (int)(i % S);
    G[i] = dstate[((size_t)row_t[r] * B + row_env[r]) * S + s];
}

// input slots: rows with p == 0 are the user slot, p >= 1 the gated action slot (state_tracker.py:205-215,225-242).
// Produces, per row, the "pre" gradient vectors the two small weight-gradient GEMMs need and scatters into the
// embedding tables:   user rows : DU[r] = dX0 (for ffn_user), EU[r] = Emb_user[u]
//                     item rows : DPRE[r] = dX0 * a * g(1-g), GIN[r] = [rew, a]  (for fnn_gate)
// value of lane k (a compile-time or wave-uniform k) in every lane: v_readlane_b32, not a ds_bpermute round trip
__device__ __forceinline__ float lane_bcast(float x, int k) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), k));
}

static __global__ __launch_bounds__(256) void slot_bwd(cirs_tracker_weights w, const float* __restrict__ dH0, const int32_t* __restrict__ users,
                                                const int64_t* __restrict__ act, const double* __restrict__ rew,
                                                const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t, int R, int B,
                                                float* __restrict__ DU, float* __restrict__ EU, float* __restrict__ DPRE,
                                                float* __restrict__ GIN, float* __restrict__ CU, float* __restrict__ CI,
                                                int32_t* __restrict__ key_user, int32_t* __restrict__ key_item,
                                                float* __restrict__ contrib_c /* [B, 32] per-env user contribution (merged scatter) or null */,
                                                int rows_per_wave, float in_scale /* d x_in / d slot: sqrt(32) for the Transformer's x * sqrt(D), 1 for the GRU */) {
    const int lane = threadIdx.x & 63;
    // the gate matrix [32][33] once per workgroup, coalesced, into LDS: lane d then walks ITS row with stride-33 reads (no bank
    // conflicts); from memory that walk is one dword per lane and load, 64 cache lines per instruction, 33 instructions per row
    __shared__ float sG[tD * (tD + 1)];
    for (int q = threadIdx.x; q < tD * (tD + 1); q += 256) sG[q] = w.gate_w[q];
    __syncthreads();
    // (rows_per_wave > 1: the call batches of the exact-redraw pass, ~0.5 M rows -- the 4 KB gate image per four rows was most of the kernel's traffic)
    for (int it_r = 0; it_r < rows_per_wave; ++it_r) {
    const int r = (blockIdx.x * rows_per_wave + it_r) * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int b = row_env[r], p = row_t[r];
    const int d = lane & 31;
    const float dx = dH0[(size_t)r * tD + d] * in_scale;  // d/dx of x * in_scale
    if (p == 0) {
        const int u = users[b];
        const float eu = w.emb_user[(size_t)u * tD + d];
        if (lane < tD) {
            DU[(size_t)r * tD + d] = dx; EU[(size_t)r * tD + d] = eu;
            DPRE[(size_t)r * tD + d] = 0.f;
        }
        if (lane <= tD) GIN[(size_t)r * (tD + 1) + lane] = 0.f;
        // dEmb_user[u, k] += sum_o dx[o] * ffn_user_w[o, k] : lane k
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < tD; ++o) acc = __builtin_fmaf(lane_bcast(dx, o), w.ffn_user_w[(size_t)o * tD + d], acc);
        if (lane < tD) {
            CU[(size_t)r * tD + d] = acc; CI[(size_t)r * tD + d] = 0.f;
            if (contrib_c) contrib_c[(size_t)b * tD + d] = acc;
        }
        if (lane == 0) { key_user[r] = u; key_item[r] = -1; }
    } else {
        const size_t ti = (size_t)(p - 1) * B + b;
        const long it = act[ti];
        const float rw = (float)rew[ti];
        const float a = w.emb_item[(size_t)it * tD + d];
        // recompute the gate for feature d (lane o = d)
        const float* gw = sG + d * (tD + 1);
        float pre = w.gate_b[d];
        pre = __builtin_fmaf(gw[0], rw, pre);
#pragma unroll
        for (int k = 0; k < tD; ++k) pre = __builtin_fmaf(gw[1 + k], lane_bcast(a, k), pre);
        const float g = 1.0f / (1.0f + expf(-pre));
        const float dpre = dx * a * g * (1.0f - g);
        if (lane < tD) {
            DPRE[(size_t)r * tD + d] = dpre;
            DU[(size_t)r * tD + d] = 0.f; EU[(size_t)r * tD + d] = 0.f;
            GIN[(size_t)r * (tD + 1) + 1 + d] = a;
        }
        if (lane == 0) GIN[(size_t)r * (tD + 1)] = rw;
        // d a[k] = dx[k]*g[k] + sum_o dpre[o] * gate_w[o, 1+k]
        float acc = dx * g;
#pragma unroll
        for (int o = 0; o < tD; ++o) acc = __builtin_fmaf(lane_bcast(dpre, o), sG[o * (tD + 1) + 1 + d], acc);
        if (lane < tD) { CI[(size_t)r * tD + d] = acc; CU[(size_t)r * tD + d] = 0.f; }
        if (lane == 0) { key_item[r] = (int32_t)it; key_user[r] = -1; }
    }
    }
}

// Deterministic embedding-gradient scatter without float atomics and without an O(rows x table) scan: the (key, row)
// pairs are sorted by key with a stable radix sort (rows stay ascending inside a key), then one 32-lane group per
// segment head adds the contribution rows of its key in row order.  Cost O(rows), independent of the table size
// (a 10^6-row catalogue costs the same as 10^4), result independent of scheduling.
static __global__ __launch_bounds__(256) void scatter_keys_kernel(const int32_t* __restrict__ keys, int R, int n_table,
                                                           uint32_t* __restrict__ keys_u, int32_t* __restrict__ rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int32_t k = keys[r];
    keys_u[r] = (k < 0 || k >= n_table) ? (uint32_t)n_table : (uint32_t)k;  // rows without a contribution sort last
    rows[r] = r;
}

// Only the first row of an episode (the user slot) contributes to Emb_user: one (key, contribution) pair per env instead of one
// per buffer row -> the sort of the user-embedding scatter handles n_env pairs.  Slot = env id, so pairs of one user stay in env
// (= row) order.
static __global__ __launch_bounds__(256) void compact_user_rows(const int32_t* __restrict__ row_env, const int32_t* __restrict__ row_t,
                                                         const int32_t* __restrict__ users, const float* __restrict__ CU, int R,
                                                         int32_t* __restrict__ keys_c, float* __restrict__ contrib_c) {
    const int d = threadIdx.x & 31;
    const int r = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (r >= R || row_t[r] != 0) return;
    const int b = row_env[r];
    contrib_c[(size_t)b * tD + d] = CU[(size_t)r * tD + d];
    if (d == 0) keys_c[b] = users[b];
}

// Ordered segment sums over the (key, row) pairs sorted by key, in two levels so that a very popular key (thousands of rows
// once the policy concentrates on few items) is not one sequential chain:
//   sub-runs   a sub-run starts at every segment head and at every multiple of 64 in the sorted order and ends at the next
//              such position: <= 64 rows, summed in row order by one half-wave (lane = embedding dimension) -> part[start]
//   segments   the head of a segment adds its sub-run partials in position order (every 64th position) -> g_emb[key]
// Fixed order, no atomics; rows of keys outside the table are skipped.
constexpr int kSubRun = 64;
// One half-wave (lane = embedding dimension) per sub-run start.  The keys and rows of the sub-run's 64-position block are read once
// (two per lane), the run length comes from a ballot, the row numbers travel between lanes by shuffle: every contribution row of the
// sub-run can then be requested without waiting for a key comparison (2 dependent round trips + one per 16 rows instead of two per 8).
static __global__ __launch_bounds__(256) void emb_subrun_kernel(const uint32_t* __restrict__ ks, const int32_t* __restrict__ rs,
                                                         const float* __restrict__ contrib, int R, int n_table, float* __restrict__ part) {
    const int d = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const int p = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool in = p < R;
    const uint32_t key = in ? ks[p] : 0xffffffffu;
    const bool start = in && key < (uint32_t)n_table && ((p % kSubRun) == 0 || ks[p - 1] != key);   // block start or segment head
    const int end = min(R, (p / kSubRun + 1) * kSubRun);
    // positions p + d and p + 32 + d of the block (the ballot needs every lane of the wavefront: no early return above)
    const int q0 = p + d, q1 = p + 32 + d;
    const bool s0 = start && q0 < end && ks[q0] == key, s1 = start && q1 < end && ks[q1] == key;
    const int r0 = s0 ? rs[q0] : 0, r1 = s1 ? rs[q1] : 0;
    const unsigned long long m0 = __ballot(s0), m1 = __ballot(s1);
    if (!start) return;
    const uint32_t h0 = (uint32_t)(m0 >> (32 * half)), h1 = (uint32_t)(m1 >> (32 * half));
    // run length: leading positions with the same key (the sort makes them contiguous)
    const int n = h0 == 0xffffffffu ? 32 + (h1 == 0xffffffffu ? 32 : __builtin_ctz(~h1)) : __builtin_ctz(~h0);
    float acc = 0.f;
    for (int q = 0; q < n; q += 16) {   // 16 rows in flight, added in row order
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int qq = q + u;
            const int row = __shfl(qq < 32 ? r0 : r1, (qq & 31) + 32 * half, CIRS_WAVE);
            t[u] = qq < n ? contrib[(size_t)row * tD + d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += (q + u < n) ? t[u] : 0.f;
    }
    part[(size_t)p * tD + d] = acc;
}

static __global__ __launch_bounds__(256) void emb_segment_sum_kernel(const uint32_t* __restrict__ ks, const float* __restrict__ part, int R,
                                                              int n_table, float* __restrict__ g_emb, int n_first = 0x7fffffff,
                                                              float* __restrict__ g_second = nullptr) {   // keys >= n_first: rows of g_second
    const int d = threadIdx.x & 31;
    const int p = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (p >= R) return;
    const uint32_t key = ks[p];
    if (key >= (uint32_t)n_table || (p > 0 && ks[p - 1] == key)) return;  // not a segment head
    float acc = part[(size_t)p * tD + d];
    for (int q = (p / kSubRun + 1) * kSubRun; q < R; q += 8 * kSubRun) {   // the segment's later sub-runs, 8 loads in flight
        float t8[8];
        int n_ok = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int qq = q + u * kSubRun;
            const bool ok = (n_ok == u) && qq < R && ks[qq] == key;
            t8[u] = ok ? part[(size_t)qq * tD + d] : 0.f;
            n_ok += ok;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (u < n_ok) ? t8[u] : 0.f;
        if (n_ok < 8) break;
    }
    if (key < (uint32_t)n_first) g_emb[(size_t)key * tD + d] = acc;
    else g_second[(size_t)(key - (uint32_t)n_first) * tD + d] = acc;
}

static size_t emb_sort_bytes(long R) { return (size_t)R * (64 + 4 * tD) + (1u << 20); }   // keys/rows in+out, sub-run partials, sort temp

// keys [R] (< 0: no contribution), contrib [R, 32] -> g_emb [n_table, 32] (fully overwritten)
static int emb_scatter_sorted(const int32_t* keys, const float* contrib, int R, int n_table, float* g_emb, void* scratch,
                              size_t scratch_bytes, hipStream_t s) {
    static_assert(tD == 32, "emb_segment_sum_kernel maps one lane per embedding dimension");
    uint32_t* k_in = (uint32_t*)scratch;
    uint32_t* k_out = k_in + R;
    int32_t* r_in = (int32_t*)(k_out + R);
    int32_t* r_out = r_in + R;
    float* part = (float*)(((uintptr_t)(r_out + R) + 255) & ~(uintptr_t)255);   // [R, 32] sub-run partials
    char* temp = (char*)(((uintptr_t)(part + (size_t)R * tD) + 255) & ~(uintptr_t)255);
    const size_t avail = scratch_bytes - (size_t)(temp - (char*)scratch);
    int end_bit = 1;
    while ((1u << end_bit) <= (uint32_t)n_table && end_bit < 32) ++end_bit;
    size_t need = 0;
    CIRS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, k_in, k_out, r_in, r_out, R, 0, end_bit, s));
    CIRS_REQUIRE(need <= avail, "embedding scatter: sort scratch too small");
    CIRS_HIP(hipMemsetAsync(g_emb, 0, (size_t)n_table * tD * sizeof(float), s));
    hipLaunchKernelGGL(scatter_keys_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, keys, R, n_table, k_in, r_in);
    CIRS_HIP(hipcub::DeviceRadixSort::SortPairs(temp, need, k_in, k_out, r_in, r_out, R, 0, end_bit, s));
    hipLaunchKernelGGL(emb_subrun_kernel, dim3(cdiv(R, 8)), dim3(256), 0, s, k_out, r_out, contrib, R, n_table, part);
    hipLaunchKernelGGL(emb_segment_sum_kernel, dim3(cdiv(R, 8)), dim3(256), 0, s, k_out, (const float*)part, R, n_table, g_emb);
    CIRS_CHECK_LAUNCH("emb_segment_sum_kernel");
    return CIRS_OK;
}

// Both embedding tables of the tracker in ONE sort: R item pairs (key = item id) followed by one user pair per env (key = n_items +
// user id, present when the env has rows in this call); contrib = [R + B, 32] (item rows, then the per-env user rows).  Same ordered
// sub-run / segment sums, half the launches of two separate scatters.
static __global__ __launch_bounds__(256) void scatter_keys2_kernel(const int32_t* __restrict__ key_item, const int32_t* __restrict__ users,
                                                            const int32_t* __restrict__ lens, int R, int B, int n_items, int n_users,
                                                            uint32_t* __restrict__ keys_u, int32_t* __restrict__ rows,
                                                            float* __restrict__ zero_table /* nullable: the contiguous gradient tables, cleared here */, long zero_floats) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    // (the tables' clear rides in this launch -- emb_segment_sum_kernel, three launches on, writes the touched rows only; a memset is a launch of its own)
    if (zero_table)
        for (long i = (long)p * 4; i < zero_floats; i += (long)gridDim.x * blockDim.x * 4) *reinterpret_cast<f32x4*>(zero_table + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p >= R + B) return;
    const uint32_t sent = (uint32_t)n_items + (uint32_t)n_users;
    uint32_t k = sent;
    if (p < R) {
        const int32_t v = key_item[p];
        if (v >= 0 && v < n_items) k = (uint32_t)v;
    } else {
        const int b = p - R;
        const int32_t u = users[b];
        if (lens[b] > 0 && u >= 0 && u < n_users) k = (uint32_t)n_items + (uint32_t)u;
    }
    keys_u[p] = k;
    rows[p] = p;
}
static int emb_scatter_merged(const int32_t* key_item, const int32_t* users, const int32_t* lens, const float* contrib, int R, int B,
                              int n_items, int n_users, float* g_item, float* g_user, void* scratch, size_t scratch_bytes, hipStream_t s) {
    const int N = R + B, n_table = n_items + n_users;
    uint32_t* k_in = (uint32_t*)scratch;
    uint32_t* k_out = k_in + N;
    int32_t* r_in = (int32_t*)(k_out + N);
    int32_t* r_out = r_in + N;
    float* part = (float*)(((uintptr_t)(r_out + N) + 255) & ~(uintptr_t)255);
    char* temp = (char*)(((uintptr_t)(part + (size_t)N * tD) + 255) & ~(uintptr_t)255);
    const size_t avail = scratch_bytes - (size_t)(temp - (char*)scratch);
    int end_bit = 1;
    while ((1u << end_bit) <= (uint32_t)n_table && end_bit < 32) ++end_bit;
    size_t need = 0;
    CIRS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, k_in, k_out, r_in, r_out, N, 0, end_bit, s));
    CIRS_REQUIRE(need <= avail, "embedding scatter: sort scratch too small");
    float* zero_table = nullptr;       // contiguous tables (the flat gradient buffer): cleared inside scatter_keys2_kernel (tD = 32 floats per row: float4 units)
    if (g_user + (size_t)n_users * tD == g_item) zero_table = g_user;
    else if (g_item + (size_t)n_items * tD == g_user) zero_table = g_item;
    if (zero_table && ((uintptr_t)zero_table & 15)) zero_table = nullptr;
    if (!zero_table) {
        CIRS_HIP(hipMemsetAsync(g_item, 0, (size_t)n_items * tD * sizeof(float), s));
        CIRS_HIP(hipMemsetAsync(g_user, 0, (size_t)n_users * tD * sizeof(float), s));
    }
    hipLaunchKernelGGL(scatter_keys2_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, key_item, users, lens, R, B, n_items, n_users, k_in, r_in, zero_table,
                       (long)n_table * tD);
    CIRS_HIP(hipcub::DeviceRadixSort::SortPairs(temp, need, k_in, k_out, r_in, r_out, N, 0, end_bit, s));
    hipLaunchKernelGGL(emb_subrun_kernel, dim3(cdiv(N, 8)), dim3(256), 0, s, k_out, r_out, contrib, N, n_table, part);
    hipLaunchKernelGGL(emb_segment_sum_kernel, dim3(cdiv(N, 8)), dim3(256), 0, s, k_out, (const float*)part, N, n_table, g_item, n_items, g_user);
    CIRS_CHECK_LAUNCH("emb_segment_sum_kernel (merged)");
    return CIRS_OK;
}

}  // namespace cirs
