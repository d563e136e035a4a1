// rankmetrics.hip -- top-k lists of a score table and their ranking / diversity metrics against a relevance table (include/cirs_hip.h:
// cirs_rows_topk, cirs_rank_metrics).  No reference counterpart.  One wavefront per row, four rows per workgroup, no hand-off between
// workgroups; every loop is bounded by n_items or k.  Selection is topk_select_wave of policy_kernels.h (the loop of cirs_actor_topk): fp32
// scores for the lists, float64 gains for the ideal list.  Every float64 sum has one order (stated at its site); the build keeps
// -ffp-contract=off, so cirs_hip/rankmetrics_host.py restates them bit for bit.
#include "common.h"
#include "policy_kernels.h"

namespace cirs {

// bit i of bitmap row `vrow` (nullptr: nothing is masked)
__device__ __forceinline__ bool rank_masked(const uint32_t* __restrict__ vrow, int i) { return vrow && ((vrow[i >> 5] >> (i & 31)) & 1u); }

__global__ __launch_bounds__(256) void rows_topk_kernel(const float* __restrict__ scores, int n, int n_items, long ld, int k,
                                                        const int32_t* __restrict__ env_ids, const uint32_t* __restrict__ visited,
                                                        const uint8_t* __restrict__ skip, int64_t* __restrict__ ids_out, float* __restrict__ vals_out) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    if (skip && skip[j]) {
        for (int r = lane; r < k; r += CIRS_WAVE) {
            ids_out[(size_t)j * k + r] = -1;
            if (vals_out) vals_out[(size_t)j * k + r] = -INFINITY;
        }
        return;
    }
    const float* row = scores + (size_t)j * ld;
    const uint32_t* vrow = visited ? visited + (size_t)(env_ids ? env_ids[j] : j) * ((n_items + 31) / 32) : nullptr;
    topk_select_wave<float>(
        lane, n_items, k, [&](int i) { return rank_masked(vrow, i) ? -INFINITY : row[i]; },
        [&](int r, float v, int id) {
            if (lane != 0) return;
            const bool none = id == 0x7FFFFFFF;
            ids_out[(size_t)j * k + r] = none ? -1 : (int64_t)id;
            if (vals_out) vals_out[(size_t)j * k + r] = none ? -INFINITY : v;
        });
}

__global__ __launch_bounds__(256) void rank_metrics_kernel(cirs_rank_cfg cfg, const int64_t* __restrict__ ids, long ld_ids,
                                                           const int32_t* __restrict__ users, int n, const double* __restrict__ rel, long ld_rel,
                                                           const uint32_t* __restrict__ item_cats, const int32_t* __restrict__ env_ids,
                                                           const uint32_t* __restrict__ visited, const uint8_t* __restrict__ skip,
                                                           double* __restrict__ per_row, int32_t* __restrict__ row_err) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    double* out = per_row + (size_t)j * CIRS_RANK_NCOL;
    const int k = cfg.k, I = cfg.n_items;
    // the list: lane a < k holds position a; nothing is addressed before the ids and the user are known to be in range
    const int u = users[j];
    const bool skipped = skip && skip[j];
    const int64_t id64 = (lane < k && !skipped) ? ids[(size_t)j * ld_ids + lane] : -1;
    const bool bad_id = id64 < -1 || id64 >= I;
    int err = __ballot(bad_id) ? CIRS_RANK_ERR_ID : 0;
    if (!skipped && (u < 0 || u >= cfg.n_users)) err |= CIRS_RANK_ERR_USER;
    if (lane == 0) row_err[j] = err;
    if (skipped || err) {
        if (lane < CIRS_RANK_NCOL) out[lane] = 0.0;
        return;
    }
    const double* rrow = rel + (size_t)u * ld_rel;
    const uint32_t* vrow = visited ? visited + (size_t)(env_ids ? env_ids[j] : j) * ((I + 31) / 32) : nullptr;
    const int id = (int)id64;
    const bool listed = id >= 0;
    const double x = listed ? rrow[id] : 0.0;
    const double gain = x > 0.0 ? x : 0.0;
    const unsigned long long listed_m = __ballot(listed), hit_m = __ballot(listed && x >= cfg.rel_threshold);
    const int n_list = __popcll(listed_m), hits = __popcll(hit_m);
    // dcg: position order r = 0 .. k-1 (a fill's term is +0.0)
    const double term = gain * cfg.discount[lane < k ? lane : 0];
    double dcg = 0.0;
    for (int r = 0; r < k; ++r) dcg += __shfl(term, r, CIRS_WAVE);
    // one pass over the user's row: n_rel (counted in the first scan only) and the k largest gains in descending order; idcg in rank order
    int n_rel_lane = 0;
    bool first_scan = true;
    double idcg = 0.0;
    topk_select_wave<double>(
        lane, I, k,
        [&](int i) {
            if (rank_masked(vrow, i)) return (double)-INFINITY;
            const double y = rrow[i];
            if (first_scan && y >= cfg.rel_threshold) ++n_rel_lane;
            return y > 0.0 ? y : (double)-INFINITY;      // a zero gain adds nothing: not a candidate
        },
        [&](int r, double v, int idx) {
            first_scan = false;
            if (idx != 0x7FFFFFFF) idcg += v * cfg.discount[r];
        });
    const int n_rel = wave_sum_i32(n_rel_lane);
    // ild: lane a holds the category mask of list item a and adds the similarities of the pairs (a, b), b = a+1 .. k-1 ascending; the lane sums are then
    // added in ascending a
    const unsigned long long cm = listed ? cat_mask(item_cats[id]) : 0ull;
    double sim_a = 0.0;
    for (int b = 1; b < k; ++b) {
        const unsigned long long cb = __shfl(cm, b, CIRS_WAVE);
        if (lane < b && listed && ((listed_m >> b) & 1ull)) {
            const int uni = __popcll(cm | cb);
            sim_a += uni ? (double)__popcll(cm & cb) / (double)uni : 0.0;
        }
    }
    double sim = 0.0;
    for (int a = 0; a < k; ++a) sim += __shfl(sim_a, a, CIRS_WAVE);
    if (lane != 0) return;
    const double pairs = 0.5 * (double)n_list * (double)(n_list - 1);
    out[0] = (double)n_list;
    out[1] = (double)n_rel;
    out[2] = (double)hits;
    out[3] = (double)hits / (double)k;
    out[4] = n_rel > 0 ? (double)hits / (double)n_rel : 0.0;
    out[5] = hits > 0 ? 1.0 : 0.0;
    out[6] = hits > 0 ? 1.0 / (double)(__ffsll(hit_m)) : 0.0;
    out[7] = dcg;
    out[8] = idcg;
    out[9] = idcg > 0.0 ? dcg / idcg : 0.0;
    out[10] = n_list >= 2 ? 1.0 - sim / pairs : 0.0;
}

// one workgroup: thread t adds rows t, t + 256, ... in ascending order, then a halving tree over the 256 partials
__global__ __launch_bounds__(256) void rank_reduce_kernel(const double* __restrict__ per_row, const int32_t* __restrict__ row_err,
                                                          const uint8_t* __restrict__ skip, int n, double* __restrict__ sums) {
    __shared__ double part[6][256];
    __shared__ int cnt[256], errs[256];
    const int t = threadIdx.x;
    const int col[6] = {3, 4, 5, 6, 9, 10};
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int c = 0, e = 0;
    for (int j = t; j < n; j += 256) {
        e |= row_err[j];
        if (skip && skip[j]) continue;
        ++c;
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] += per_row[(size_t)j * CIRS_RANK_NCOL + col[q]];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) part[q][t] = acc[q];
    cnt[t] = c; errs[t] = e;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int q = 0; q < 6; ++q) part[q][t] += part[q][t + off];
            cnt[t] += cnt[t + off];
            errs[t] |= errs[t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        sums[0] = (double)cnt[0];
        sums[1] = (double)errs[0];
    }
    if (t < 6) sums[2 + t] = cnt[0] > 0 ? part[t][0] / (double)cnt[0] : 0.0;
}

}  // namespace cirs

extern "C" int cirs_rows_topk(const float* scores, int32_t n, int32_t n_items, int64_t ld, int32_t k, const int32_t* env_ids,
                              const uint32_t* visited, const uint8_t* skip, int64_t* ids_out, float* vals_out, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(k >= 1 && k <= CIRS_TOPK_MAX, "k must lie in 1..32");
    CIRS_REQUIRE(n_items >= 1, "n_items < 1");
    CIRS_REQUIRE(ld >= n_items, "ld < n_items");
    if (n <= 0) return CIRS_OK;
    CIRS_REQUIRE(scores && ids_out, "null scores/ids");
    hipLaunchKernelGGL(rows_topk_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, scores, n, n_items, (long)ld, k, env_ids, visited, skip,
                       ids_out, vals_out);
    CIRS_CHECK_LAUNCH("rows_topk_kernel");
    return CIRS_OK;
}

extern "C" int64_t cirs_rank_metrics_workspace_bytes(int32_t n) { return n > 0 ? (int64_t)n * 4 : 0; }

extern "C" int cirs_rank_metrics(const cirs_rank_cfg* cfg, const int64_t* ids, int64_t ld_ids, const int32_t* users, int32_t n, const double* rel,
                                 int64_t ld_rel, const uint32_t* item_cats, const int32_t* env_ids, const uint32_t* visited, const uint8_t* skip,
                                 double* per_row, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cirs;
    CIRS_REQUIRE(cfg, "null cfg");
    CIRS_REQUIRE(cfg->k >= 1 && cfg->k <= CIRS_TOPK_MAX, "k must lie in 1..32");
    CIRS_REQUIRE(cfg->n_users >= 1 && cfg->n_items >= 1, "n_users / n_items < 1");
    CIRS_REQUIRE(ld_ids >= cfg->k, "ld_ids < k");
    CIRS_REQUIRE(ld_rel >= cfg->n_items, "ld_rel < n_items");
    if (n <= 0) return CIRS_OK;
    CIRS_REQUIRE(ids && users && rel && item_cats && per_row && sums && workspace, "null ids/users/rel/item_cats/per_row/sums/workspace");
    CIRS_REQUIRE(workspace_bytes >= cirs_rank_metrics_workspace_bytes(n), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int32_t* row_err = (int32_t*)workspace;
    hipLaunchKernelGGL(rank_metrics_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, *cfg, ids, (long)ld_ids, users, n, rel, (long)ld_rel, item_cats, env_ids,
                       visited, skip, per_row, row_err);
    CIRS_CHECK_LAUNCH("rank_metrics_kernel");
    hipLaunchKernelGGL(rank_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)per_row, (const int32_t*)row_err, skip, n, sums);
    CIRS_CHECK_LAUNCH("rank_reduce_kernel");
    return CIRS_OK;
}
