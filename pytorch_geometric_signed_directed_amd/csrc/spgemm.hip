// Sparse Gram product C = B^T diag(s) B (Gustavson, one output row at a time) and the row-wise intersection merge of two
// CSRs: the second-order proximity operators of DGCN (utils/directed/features_in_out.py) and DiGCN
// (utils/directed/get_adjs_DiGCN.py:get_second_directed_adj).  include/pygsd_hip.h documents the pipeline.
//
// Output row i of C gathers one product per pair (t, e): t an entry (k, B[k, i]) of row i of B^T, e an entry (j, B[k, j])
// of row k of B.  The products of a row are numbered p = 0, 1, ... in that (t, e) order, and every path sums the products
// of one output column in ascending p, sequentially, in float64 -- so the LDS tiers and the global (hub) path give
// bit-identical rows, whatever the binning or the launch geometry.  No floating-point atomics.
//   LDS tiers: the row's products are expanded into LDS as 64-bit keys (j << 32 | p) beside their float64 values, the
//              keys are bitonic-sorted, and one wavefront sums the runs of equal j and compacts the non-zero sums.
//   hub path : the products of a batch of long rows are expanded to global memory under the key (hub << 32 | j), stably
//              radix-sorted (rocPRIM; equal keys keep ascending p), and reduced run by run.
// Both write the compacted row into a temporary laid out like the products (row i at prod_ptr[i]); pygsd_gram_emit packs
// the rows into the final int32 CSR once the exact nnz is known.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.hpp"

namespace pygsd {
namespace {

constexpr int kBlock = 256;

// the value of one product, computed the same way on every path: (B[k, i] * s[k]) * B[k, j] in float64
__device__ __forceinline__ double row_factor(float t_val, const double* scale, int k)
{
    return static_cast<double>(t_val) * (scale ? scale[k] : 1.0);
}

// count[i] = number of products of output row i = sum over k in row i of B^T of rowlen_B(k)
__global__ void gram_count_kernel(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_col,
                                  const int32_t* __restrict__ b_rowptr, int32_t n_out, int64_t* __restrict__ count)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_out;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        int64_t c = 0;
        for (int32_t t = t_rowptr[i]; t < t_rowptr[i + 1]; ++t) {
            const int32_t k = t_col[t];
            c += b_rowptr[k + 1] - b_rowptr[k];
        }
        count[i] = c;
    }
}

// One output row per block, held in LDS: CAP products at most (rows above it must not be listed; a row that is gets
// row_nnz = -1 and no LDS write).  Persistent over the listed rows.
template <int THREADS, int CAP>
__global__ __launch_bounds__(THREADS) void gram_rows_lds(
    const int32_t* __restrict__ b_rowptr, const int32_t* __restrict__ b_col, const float* __restrict__ b_val,
    const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_col, const float* __restrict__ t_val,
    const double* __restrict__ scale, const int32_t* __restrict__ rows, int32_t n_rows,
    const int64_t* __restrict__ prod_ptr, int32_t* __restrict__ tmp_col, float* __restrict__ tmp_val,
    int64_t* __restrict__ row_nnz)
{
    __shared__ uint64_t keys[CAP];
    __shared__ double vals[CAP];
    for (int32_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int32_t i = rows[r];
        const int64_t base = prod_ptr[i];
        const int64_t np64 = prod_ptr[i + 1] - base;
        if (np64 > CAP) {
            if (threadIdx.x == 0) row_nnz[i] = -1;
            continue;
        }
        const int np = static_cast<int>(np64);
        // expand in (t, e) order
        int run = 0;
        for (int32_t t = t_rowptr[i]; t < t_rowptr[i + 1]; ++t) {
            const int32_t k = t_col[t];
            const double a = row_factor(t_val[t], scale, k);
            const int32_t lo = b_rowptr[k], len = b_rowptr[k + 1] - lo;
            for (int e = threadIdx.x; e < len; e += THREADS) {
                keys[run + e] = (static_cast<uint64_t>(static_cast<uint32_t>(b_col[lo + e])) << 32) |
                                static_cast<uint32_t>(run + e);
                vals[run + e] = a * static_cast<double>(b_val[lo + e]);
            }
            run += len;
        }
        int p2 = 1;
        while (p2 < np) p2 <<= 1;
        for (int q = np + threadIdx.x; q < p2; q += THREADS) keys[q] = ~uint64_t(0);
        __syncthreads();
        // bitonic sort of keys[0, p2): keys are distinct (p is part of them), so the order is total
        for (int size = 2; size <= p2; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int q = threadIdx.x; q < (p2 >> 1); q += THREADS) {
                    const int lo = 2 * q - (q & (stride - 1));
                    const int hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const uint64_t x = keys[lo], y = keys[hi];
                    if ((x > y) == up) {
                        keys[lo] = y;
                        keys[hi] = x;
                    }
                }
                __syncthreads();
            }
        }
        // one wavefront: runs of equal j summed in ascending p, non-zero sums compacted in column order
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            int cnt = 0;
            for (int c = 0; c < np; c += 64) {
                const int q = c + lane;
                bool emit = false;
                double sum = 0.0;
                uint32_t j = 0;
                if (q < np) {
                    j = static_cast<uint32_t>(keys[q] >> 32);
                    if (q == 0 || static_cast<uint32_t>(keys[q - 1] >> 32) != j) {
                        for (int u = q; u < np && static_cast<uint32_t>(keys[u] >> 32) == j; ++u)
                            sum += vals[static_cast<uint32_t>(keys[u])];
                        emit = sum != 0.0;
                    }
                }
                const uint64_t m = __ballot(emit);
                if (emit) {
                    const int pos = cnt + __popcll(m & ((uint64_t(1) << lane) - 1));
                    tmp_col[base + pos] = static_cast<int32_t>(j);
                    tmp_val[base + pos] = static_cast<float>(sum);
                }
                cnt += __popcll(m);
            }
            if (lane == 0) row_nnz[i] = cnt;
        }
        __syncthreads();
    }
}

// ---- hub path ---------------------------------------------------------------------------------------------------------
// products of hub h start at hub_off[h] (batch-relative, hub_off[n_hub] = batch products), key = h << 32 | j
__global__ void hub_expand(const int32_t* __restrict__ b_rowptr, const int32_t* __restrict__ b_col,
                           const float* __restrict__ b_val, const int32_t* __restrict__ t_rowptr,
                           const int32_t* __restrict__ t_col, const float* __restrict__ t_val,
                           const double* __restrict__ scale, const int32_t* __restrict__ hub_rows,
                           const int64_t* __restrict__ hub_off, int32_t n_hub, uint64_t* __restrict__ keys,
                           uint32_t* __restrict__ ids, double* __restrict__ vals)
{
    for (int32_t h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const int32_t i = hub_rows[h];
        int64_t run = hub_off[h];
        for (int32_t t = t_rowptr[i]; t < t_rowptr[i + 1]; ++t) {
            const int32_t k = t_col[t];
            const double a = row_factor(t_val[t], scale, k);
            const int32_t lo = b_rowptr[k], len = b_rowptr[k + 1] - lo;
            for (int e = threadIdx.x; e < len; e += blockDim.x) {
                const int64_t q = run + e;
                keys[q] = (static_cast<uint64_t>(h) << 32) | static_cast<uint32_t>(b_col[lo + e]);
                ids[q] = static_cast<uint32_t>(q);
                vals[q] = a * static_cast<double>(b_val[lo + e]);
            }
            run += len;
        }
    }
}

__global__ void hub_gather(const double* __restrict__ vals, const uint32_t* __restrict__ perm, int64_t n,
                           double* __restrict__ sorted)
{
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < n;
         q += static_cast<int64_t>(gridDim.x) * blockDim.x)
        sorted[q] = vals[perm[q]];
}

// at each run head: the run's float64 sum (ascending p: the sort is stable) and whether it is emitted
__global__ void hub_heads(const uint64_t* __restrict__ keys, const double* __restrict__ sorted, int64_t n,
                          double* __restrict__ sums, int32_t* __restrict__ flags)
{
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < n;
         q += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const uint64_t key = keys[q];
        int32_t f = 0;
        if (q == 0 || keys[q - 1] != key) {
            double sum = 0.0;
            for (int64_t u = q; u < n && keys[u] == key; ++u) sum += sorted[u];
            sums[q] = sum;
            f = sum != 0.0 ? 1 : 0;
        }
        flags[q] = f;
    }
}

__global__ void hub_emit(const uint64_t* __restrict__ keys, const double* __restrict__ sums,
                         const int32_t* __restrict__ flags, const int32_t* __restrict__ incl, int64_t n,
                         const int32_t* __restrict__ hub_rows, const int64_t* __restrict__ hub_off,
                         const int64_t* __restrict__ prod_ptr, int32_t* __restrict__ tmp_col, float* __restrict__ tmp_val)
{
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < n;
         q += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        if (!flags[q]) continue;
        const int32_t h = static_cast<int32_t>(keys[q] >> 32);
        const int64_t start = hub_off[h];
        const int32_t before = start > 0 ? incl[start - 1] : 0;
        const int64_t out = prod_ptr[hub_rows[h]] + (incl[q] - 1 - before);
        tmp_col[out] = static_cast<int32_t>(static_cast<uint32_t>(keys[q]));
        tmp_val[out] = static_cast<float>(sums[q]);
    }
}

__global__ void hub_counts(const int32_t* __restrict__ incl, const int32_t* __restrict__ hub_rows,
                           const int64_t* __restrict__ hub_off, int32_t n_hub, int64_t* __restrict__ row_nnz)
{
    for (int32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n_hub; h += gridDim.x * blockDim.x) {
        const int64_t lo = hub_off[h], hi = hub_off[h + 1];
        const int32_t before = lo > 0 ? incl[lo - 1] : 0;
        row_nnz[hub_rows[h]] = hi > lo ? incl[hi - 1] - before : 0;
    }
}

// ---- packing and the intersection merge -------------------------------------------------------------------------------
// one wavefront per row: rowptr[i] = c_ptr[i]; the compacted row moves from the temporary to the final CSR
__global__ void gram_pack(const int64_t* __restrict__ prod_ptr, const int32_t* __restrict__ tmp_col,
                          const float* __restrict__ tmp_val, const int64_t* __restrict__ c_ptr, int32_t n_out,
                          int32_t* __restrict__ rowptr, int32_t* __restrict__ col, float* __restrict__ val)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (blockDim.x >> 6);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); i <= n_out; i += waves) {
        if (lane == 0) rowptr[i] = static_cast<int32_t>(c_ptr[i]);
        if (i == n_out) break;
        const int64_t src = prod_ptr[i], dst = c_ptr[i], len = c_ptr[i + 1] - dst;
        for (int64_t e = lane; e < len; e += 64) {
            col[dst + e] = tmp_col[src + e];
            val[dst + e] = tmp_val[src + e];
        }
    }
}

// lower bound of j in col[lo, hi); the midpoint never forms lo + hi, which wraps int32 once offsets pass 2^30
__device__ __forceinline__ int32_t find_col(const int32_t* __restrict__ col, int32_t lo, int32_t hi, int32_t j)
{
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < j) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wavefront per row of A: binary search of each entry in the same row of B.  emit == 0: count[i] = entries in both
// with a non-zero (a + b); emit != 0: write them (ascending column, as A's row) at c_ptr[i] with value (a + b) / 2.
__global__ void intersect_kernel(const int32_t* __restrict__ a_rowptr, const int32_t* __restrict__ a_col,
                                 const float* __restrict__ a_val, const int32_t* __restrict__ b_rowptr,
                                 const int32_t* __restrict__ b_col, const float* __restrict__ b_val, int32_t n_rows,
                                 int emit, int64_t* __restrict__ count, const int64_t* __restrict__ c_ptr,
                                 int32_t* __restrict__ rowptr, int32_t* __restrict__ out_col, float* __restrict__ out_val)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (blockDim.x >> 6);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); i <= n_rows; i += waves) {
        if (emit && lane == 0) rowptr[i] = static_cast<int32_t>(c_ptr[i]);
        if (i == n_rows) break;
        const int32_t a0 = a_rowptr[i], a1 = a_rowptr[i + 1], b0 = b_rowptr[i], b1 = b_rowptr[i + 1];
        int64_t cnt = 0;
        const int64_t dst = emit ? c_ptr[i] : 0;
        for (int64_t base = a0; base < a1; base += 64) {          // int64: base + 64 may pass INT32_MAX
            const int64_t e = base + lane;
            bool hit = false;
            double v = 0.0;
            int32_t j = 0;
            if (e < a1) {
                j = a_col[e];
                const int32_t f = find_col(b_col, b0, b1, j);
                if (f < b1 && b_col[f] == j) {
                    v = static_cast<double>(a_val[e]) + static_cast<double>(b_val[f]);
                    hit = v != 0.0;
                }
            }
            const uint64_t m = __ballot(hit);
            if (emit && hit) {
                const int64_t pos = dst + cnt + __popcll(m & ((uint64_t(1) << lane) - 1));
                out_col[pos] = j;
                out_val[pos] = static_cast<float>(v * 0.5);
            }
            cnt += __popcll(m);
        }
        if (!emit && lane == 0) count[i] = cnt;
    }
}

template <int THREADS, int CAP>
int launch_tier(const int32_t* b_rowptr, const int32_t* b_col, const float* b_val, const int32_t* t_rowptr,
                const int32_t* t_col, const float* t_val, const double* scale, const int32_t* rows, int32_t n_rows,
                const int64_t* prod_ptr, int32_t* tmp_col, float* tmp_val, int64_t* row_nnz, int per_cu,
                hipStream_t s)
{
    const int32_t grid = n_rows < 256 * per_cu ? n_rows : 256 * per_cu;
    hipLaunchKernelGGL((gram_rows_lds<THREADS, CAP>), dim3(grid), dim3(THREADS), 0, s, b_rowptr, b_col, b_val, t_rowptr,
                       t_col, t_val, scale, rows, n_rows, prod_ptr, tmp_col, tmp_val, row_nnz);
    return check_launch("gram_rows_lds");
}

struct HubWs {
    size_t keys_in, keys_out, ids, perm, vals, sorted, sums, flags, incl, temp, temp_bytes, total;
};

int hub_ws_layout(int64_t n, HubWs* w)
{
    size_t sort_temp = 0, scan_temp = 0;
    uint64_t* k = nullptr;
    uint32_t* v = nullptr;
    int32_t* f = nullptr;
    PYGSD_HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_temp, k, k, v, v, static_cast<size_t>(n), 0u, 64u,
                                            hipStream_t(nullptr)));
    PYGSD_HIP_TRY(rocprim::inclusive_scan(nullptr, scan_temp, f, f, static_cast<size_t>(n), rocprim::plus<int32_t>(),
                                          hipStream_t(nullptr)));
    const size_t n8 = round_up(static_cast<size_t>(n) * 8, 256), n4 = round_up(static_cast<size_t>(n) * 4, 256);
    size_t off = 0;
    w->keys_in = off; off += n8;
    w->keys_out = off; off += n8;
    w->vals = off; off += n8;
    w->sorted = off; off += n8;
    w->sums = off; off += n8;
    w->ids = off; off += n4;
    w->perm = off; off += n4;
    w->flags = off; off += n4;
    w->incl = off; off += n4;
    w->temp = off;
    w->temp_bytes = sort_temp > scan_temp ? sort_temp : scan_temp;
    off += round_up(w->temp_bytes, 256);
    w->total = off + 256;
    return 0;
}

int scan_temp_bytes(int32_t n, size_t* bytes)
{
    int64_t* p = nullptr;
    PYGSD_HIP_TRY(rocprim::inclusive_scan(nullptr, *bytes, p, p, static_cast<size_t>(n > 0 ? n : 1),
                                          rocprim::plus<int64_t>(), hipStream_t(nullptr)));
    return 0;
}

}  // namespace
}  // namespace pygsd

using namespace pygsd;

extern "C" int pygsd_scan_i64_workspace(int32_t n, size_t* bytes)
{
    PYGSD_REQUIRE(bytes && n >= 0, "pygsd_scan_i64_workspace: bad arguments");
    size_t t = 0;
    if (int rc = scan_temp_bytes(n, &t)) return rc;
    *bytes = t + 256;
    return 0;
}

extern "C" int pygsd_scan_i64(const int64_t* in, int32_t n, int64_t* out, void* workspace, size_t workspace_bytes,
                              void* stream)
{
    PYGSD_REQUIRE(n >= 0 && out, "pygsd_scan_i64: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    PYGSD_HIP_TRY(hipMemsetAsync(out, 0, sizeof(int64_t), s));
    if (n == 0) return 0;
    PYGSD_REQUIRE(in && workspace, "pygsd_scan_i64: null pointer");
    size_t t = 0;
    if (int rc = scan_temp_bytes(n, &t)) return rc;
    PYGSD_REQUIRE(workspace_bytes >= t + 256, "pygsd_scan_i64: workspace too small (%zu < %zu)", workspace_bytes, t + 256);
    PYGSD_HIP_TRY(rocprim::inclusive_scan(align256(workspace), t, in, out + 1, static_cast<size_t>(n),
                                          rocprim::plus<int64_t>(), s));
    return 0;
}

extern "C" int pygsd_gram_count(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* b_rowptr, int32_t n_out,
                                int64_t* count, void* stream)
{
    PYGSD_REQUIRE(n_out >= 0, "pygsd_gram_count: negative row count");
    if (n_out == 0) return 0;
    PYGSD_REQUIRE(t_rowptr && t_col && b_rowptr && count, "pygsd_gram_count: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    hipLaunchKernelGGL(gram_count_kernel, dim3(grid_for(n_out)), dim3(kBlock), 0, s, t_rowptr, t_col, b_rowptr, n_out,
                       count);
    return check_launch("gram_count_kernel");
}

extern "C" int pygsd_gram_tier_cap(int32_t tier)
{
    return tier == 0 ? PYGSD_GRAM_CAP0 : tier == 1 ? PYGSD_GRAM_CAP1 : tier == 2 ? PYGSD_GRAM_CAP2 : 0;
}

extern "C" int pygsd_gram_rows(const int32_t* b_rowptr, const int32_t* b_col, const float* b_val,
                               const int32_t* t_rowptr, const int32_t* t_col, const float* t_val, const double* scale,
                               const int32_t* rows, int32_t n_rows, int32_t tier, const int64_t* prod_ptr,
                               int32_t* tmp_col, float* tmp_val, int64_t* row_nnz, void* stream)
{
    PYGSD_REQUIRE(n_rows >= 0 && tier >= 0 && tier <= 2, "pygsd_gram_rows: n_rows=%d tier=%d", n_rows, tier);
    if (n_rows == 0) return 0;
    PYGSD_REQUIRE(b_rowptr && b_col && b_val && t_rowptr && t_col && t_val && rows && prod_ptr && tmp_col && tmp_val &&
                  row_nnz, "pygsd_gram_rows: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    if (tier == 0)
        return launch_tier<64, PYGSD_GRAM_CAP0>(b_rowptr, b_col, b_val, t_rowptr, t_col, t_val, scale, rows, n_rows,
                                                prod_ptr, tmp_col, tmp_val, row_nnz, 16, s);
    if (tier == 1)
        return launch_tier<256, PYGSD_GRAM_CAP1>(b_rowptr, b_col, b_val, t_rowptr, t_col, t_val, scale, rows, n_rows,
                                                 prod_ptr, tmp_col, tmp_val, row_nnz, 4, s);
    return launch_tier<512, PYGSD_GRAM_CAP2>(b_rowptr, b_col, b_val, t_rowptr, t_col, t_val, scale, rows, n_rows,
                                             prod_ptr, tmp_col, tmp_val, row_nnz, 2, s);
}

extern "C" int pygsd_gram_hub_workspace(int64_t n_products, size_t* bytes)
{
    PYGSD_REQUIRE(bytes, "pygsd_gram_hub_workspace: null output");
    PYGSD_REQUIRE(n_products >= 0 && n_products < (int64_t(1) << 31),
                  "pygsd_gram_hub_workspace: %lld products in one hub batch; the limit is 2^31 - 1",
                  static_cast<long long>(n_products));
    HubWs w;
    if (int rc = hub_ws_layout(n_products > 0 ? n_products : 1, &w)) return rc;
    *bytes = w.total;
    return 0;
}

extern "C" int pygsd_gram_hub(const int32_t* b_rowptr, const int32_t* b_col, const float* b_val,
                              const int32_t* t_rowptr, const int32_t* t_col, const float* t_val, const double* scale,
                              const int32_t* hub_rows, const int64_t* hub_off, int32_t n_hub, int64_t n_products,
                              const int64_t* prod_ptr, int32_t* tmp_col, float* tmp_val, int64_t* row_nnz,
                              void* workspace, size_t workspace_bytes, void* stream)
{
    PYGSD_REQUIRE(n_hub >= 0 && n_products >= 0 && n_products < (int64_t(1) << 31),
                  "pygsd_gram_hub: %lld products in one hub batch; the limit is 2^31 - 1",
                  static_cast<long long>(n_products));
    if (n_hub == 0) return 0;
    PYGSD_REQUIRE(b_rowptr && b_col && b_val && t_rowptr && t_col && t_val && hub_rows && hub_off && prod_ptr &&
                  tmp_col && tmp_val && row_nnz && workspace, "pygsd_gram_hub: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    if (n_products == 0) {
        hipLaunchKernelGGL(hub_counts, dim3(grid_for(n_hub)), dim3(kBlock), 0, s, nullptr, hub_rows, hub_off, n_hub,
                           row_nnz);
        return check_launch("hub_counts");
    }
    HubWs w;
    if (int rc = hub_ws_layout(n_products, &w)) return rc;
    PYGSD_REQUIRE(workspace_bytes >= w.total, "pygsd_gram_hub: workspace too small (%zu < %zu)", workspace_bytes, w.total);
    char* base = align256(workspace);
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(base + w.keys_in);
    uint64_t* keys_out = reinterpret_cast<uint64_t*>(base + w.keys_out);
    uint32_t* ids = reinterpret_cast<uint32_t*>(base + w.ids);
    uint32_t* perm = reinterpret_cast<uint32_t*>(base + w.perm);
    double* vals = reinterpret_cast<double*>(base + w.vals);
    double* sorted = reinterpret_cast<double*>(base + w.sorted);
    double* sums = reinterpret_cast<double*>(base + w.sums);
    int32_t* flags = reinterpret_cast<int32_t*>(base + w.flags);
    int32_t* incl = reinterpret_cast<int32_t*>(base + w.incl);
    const int64_t n = n_products;
    hipLaunchKernelGGL(hub_expand, dim3(n_hub < 1024 ? n_hub : 1024), dim3(kBlock), 0, s, b_rowptr, b_col, b_val,
                       t_rowptr, t_col, t_val, scale, hub_rows, hub_off, n_hub, keys_in, ids, vals);
    if (int rc = check_launch("hub_expand")) return rc;
    size_t temp_bytes = w.temp_bytes;
    const unsigned bits = 32u + static_cast<unsigned>(bits_for(static_cast<uint64_t>(n_hub - 1)));
    PYGSD_HIP_TRY(rocprim::radix_sort_pairs(base + w.temp, temp_bytes, keys_in, keys_out, ids, perm,
                                            static_cast<size_t>(n), 0u, bits, s));
    hipLaunchKernelGGL(hub_gather, dim3(grid_for(n)), dim3(kBlock), 0, s, vals, perm, n, sorted);
    if (int rc = check_launch("hub_gather")) return rc;
    hipLaunchKernelGGL(hub_heads, dim3(grid_for(n)), dim3(kBlock), 0, s, keys_out, sorted, n, sums, flags);
    if (int rc = check_launch("hub_heads")) return rc;
    temp_bytes = w.temp_bytes;
    PYGSD_HIP_TRY(rocprim::inclusive_scan(base + w.temp, temp_bytes, flags, incl, static_cast<size_t>(n),
                                          rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(hub_emit, dim3(grid_for(n)), dim3(kBlock), 0, s, keys_out, sums, flags, incl, n, hub_rows, hub_off,
                       prod_ptr, tmp_col, tmp_val);
    if (int rc = check_launch("hub_emit")) return rc;
    hipLaunchKernelGGL(hub_counts, dim3(grid_for(n_hub)), dim3(kBlock), 0, s, incl, hub_rows, hub_off, n_hub, row_nnz);
    return check_launch("hub_counts");
}

extern "C" int pygsd_gram_emit(const int64_t* prod_ptr, const int32_t* tmp_col, const float* tmp_val,
                               const int64_t* c_ptr, int32_t n_out, int64_t nnz, int32_t* rowptr, int32_t* col,
                               float* val, void* stream)
{
    PYGSD_REQUIRE(nnz >= 0 && nnz <= INT32_MAX,
                  "pygsd_gram_emit: the product has %lld entries; an int32 CSR holds at most 2^31 - 1 = %d",
                  static_cast<long long>(nnz), INT32_MAX);
    PYGSD_REQUIRE(n_out >= 0 && rowptr && c_ptr, "pygsd_gram_emit: bad arguments");
    PYGSD_REQUIRE(nnz == 0 || (prod_ptr && tmp_col && tmp_val && col && val), "pygsd_gram_emit: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    hipLaunchKernelGGL(gram_pack, dim3(grid_for(static_cast<int64_t>(n_out) + 1, 4)), dim3(kBlock), 0, s, prod_ptr,
                       tmp_col, tmp_val, c_ptr, n_out, rowptr, col, val);
    return check_launch("gram_pack");
}

extern "C" int pygsd_csr_intersect_count(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val,
                                         const int32_t* b_rowptr, const int32_t* b_col, const float* b_val,
                                         int32_t n_rows, int64_t* count, void* stream)
{
    PYGSD_REQUIRE(n_rows >= 0, "pygsd_csr_intersect_count: negative row count");
    if (n_rows == 0) return 0;
    PYGSD_REQUIRE(a_rowptr && b_rowptr && count, "pygsd_csr_intersect_count: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    hipLaunchKernelGGL(intersect_kernel, dim3(grid_for(static_cast<int64_t>(n_rows) + 1, 4)), dim3(kBlock), 0, s,
                       a_rowptr, a_col, a_val, b_rowptr, b_col, b_val, n_rows, 0, count, nullptr, nullptr, nullptr,
                       nullptr);
    return check_launch("intersect_kernel");
}

extern "C" int pygsd_csr_intersect_emit(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val,
                                        const int32_t* b_rowptr, const int32_t* b_col, const float* b_val,
                                        int32_t n_rows, const int64_t* c_ptr, int64_t nnz, int32_t* rowptr,
                                        int32_t* out_col, float* out_val, void* stream)
{
    PYGSD_REQUIRE(nnz >= 0 && nnz <= INT32_MAX,
                  "pygsd_csr_intersect_emit: %lld entries; an int32 CSR holds at most 2^31 - 1 = %d",
                  static_cast<long long>(nnz), INT32_MAX);
    PYGSD_REQUIRE(n_rows >= 0 && rowptr && c_ptr, "pygsd_csr_intersect_emit: bad arguments");
    PYGSD_REQUIRE(nnz == 0 || (a_rowptr && a_col && a_val && b_rowptr && b_col && b_val && out_col && out_val),
                  "pygsd_csr_intersect_emit: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    hipLaunchKernelGGL(intersect_kernel, dim3(grid_for(static_cast<int64_t>(n_rows) + 1, 4)), dim3(kBlock), 0, s,
                       a_rowptr, a_col, a_val, b_rowptr, b_col, b_val, n_rows, 1, nullptr, c_ptr, rowptr, out_col,
                       out_val);
    return check_launch("intersect_kernel");
}
