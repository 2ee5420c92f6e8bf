// Typed triangle-motif counts of the signed models SDGNN and SiGAT (nn/models.py: build_edge_lists).
// include/pygsd_hip.h documents the pipeline.
//
// Neighbourhoods: every key (u, v) of U = P u N (sorted unique u * n + v with two flag bits: in P, in N) emits
// (u, v) with its "out" bits and (v, u) with its "in" bits.  One radix sort (pygsd_sort_keys_u64) brings the two
// entries of a pair next to each other -- a pair (a, b) comes from at most the key (a, b) and the key (b, a), so runs are
// at most two long and a self-loop is exactly such a run -- head marking + pygsd_scan_i64 compact them into an int32 CSR
// with ascending columns and one 4-bit mask per entry (bit 0: w in out_P, 1: out_N, 2: in_P, 3: in_N).
//
// Counts: for a key (u, v) the shorter of the two typed lists is searched in the longer one (binary search whose lower
// end only moves forward, as the short list ascends).  A common w with masks a (of u) and b (of v) adds
// a_i & b_j to one of 16 integer counters.  Two tiers: one lane per key, and one wavefront per key (lanes split the
// short list, the counters are reduced across the wavefront).  No atomics: one lane or one wavefront owns a key, so
// both tiers give the same bits.
#include "common.hpp"

namespace pygsd {
namespace {

constexpr int kThreads = 256;

// ---- neighbourhoods -------------------------------------------------------------------------------------------------------------

__global__ void nb_emit_kernel(const int64_t* __restrict__ keys, int64_t k, int64_t n, uint64_t* __restrict__ out)
{
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < k; i += int64_t(gridDim.x) * blockDim.x) {
        const int64_t key = keys[i];
        const int64_t u = key / n, v = key - u * n;
        out[i] = static_cast<uint64_t>(key);
        out[k + i] = static_cast<uint64_t>(v * n + u);
    }
}

__global__ void nb_head_kernel(const uint64_t* __restrict__ sorted, int64_t m, int64_t* __restrict__ head)
{
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x)
        head[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

// mask bits of emitted entry q (< k: the out entry of key q, else the in entry of key q - k); flags bit 0 = P, bit 1 = N
__device__ __forceinline__ uint8_t entry_bits(const uint8_t* flags, int32_t q, int64_t k)
{
    return q < k ? flags[q] : static_cast<uint8_t>(flags[q - k] << 2);
}

__global__ void nb_compact_kernel(const uint64_t* __restrict__ sorted, const int32_t* __restrict__ perm,
                                  const uint8_t* __restrict__ flags, int64_t k, int64_t n, int64_t m,
                                  const int64_t* __restrict__ pos, int32_t* __restrict__ col, uint8_t* __restrict__ mask)
{
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
        const uint64_t key = sorted[i];
        if (i > 0 && sorted[i - 1] == key) continue;                  // the second entry of a run: folded in by its head
        uint8_t bits = entry_bits(flags, perm[i], k);
        if (i + 1 < m && sorted[i + 1] == key) bits |= entry_bits(flags, perm[i + 1], k);
        const int64_t p = pos[i];
        col[p] = static_cast<int32_t>(key % static_cast<uint64_t>(n));
        mask[p] = bits;
    }
}

// rowptr[r] = compact index of the first sorted entry with key >= r * n (r = n: the total)
__global__ void nb_rowptr_kernel(const uint64_t* __restrict__ sorted, int64_t m, int64_t n,
                                 const int64_t* __restrict__ pos, int32_t* __restrict__ rowptr)
{
    for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r <= n; r += int64_t(gridDim.x) * blockDim.x) {
        const uint64_t want = static_cast<uint64_t>(r) * static_cast<uint64_t>(n);
        int64_t lo = 0, hi = m;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (sorted[mid] < want) lo = mid + 1; else hi = mid;
        }
        rowptr[r] = static_cast<int32_t>(pos[lo]);
    }
}

// ---- counts -----------------------------------------------------------------------------------------------------------------------

// first index in [lo, hi) with col[idx] >= w
__device__ __forceinline__ int32_t lower_bound(const int32_t* __restrict__ col, int32_t lo, int32_t hi, int32_t w)
{
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a common neighbour with mask a in u's list and b in v's list; counter 4 g + 2 x + y, g: d1 out(u)&in(v),
// d2 out(u)&out(v), d3 in(u)&out(v), d4 in(u)&in(v); x, y: 0 = P, 1 = N
__device__ __forceinline__ void add_pair(int32_t (&c)[16], uint32_t a, uint32_t b)
{
    const uint32_t side_u[4] = {a & 3u, a & 3u, a >> 2, a >> 2};
    const uint32_t side_v[4] = {b >> 2, b & 3u, b & 3u, b >> 2};
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) c[4 * g + 2 * x + y] += static_cast<int32_t>((side_u[g] >> x) & (side_v[g] >> y) & 1u);
}

struct Lists {
    int32_t s0, s1, l0, l1;   // short list [s0, s1), long list [l0, l1)
    bool short_is_u;
};

__device__ __forceinline__ Lists lists_of(const int64_t* keys, int64_t n, const int32_t* rowptr, int32_t idx)
{
    const int64_t key = keys[idx];
    const int32_t u = static_cast<int32_t>(key / n), v = static_cast<int32_t>(key - (key / n) * n);
    const int32_t u0 = rowptr[u], u1 = rowptr[u + 1], v0 = rowptr[v], v1 = rowptr[v + 1];
    Lists L;
    L.short_is_u = (u1 - u0) <= (v1 - v0);
    L.s0 = L.short_is_u ? u0 : v0;
    L.s1 = L.short_is_u ? u1 : v1;
    L.l0 = L.short_is_u ? v0 : u0;
    L.l1 = L.short_is_u ? v1 : u1;
    return L;
}

// walk short-list entries j = first, first + step, ... (ascending): binary-search each in the long list
__device__ __forceinline__ void intersect(const int32_t* __restrict__ col, const uint8_t* __restrict__ mask, const Lists& L,
                                          int32_t first, int32_t step, int32_t (&c)[16])
{
    int32_t lo = L.l0;
    for (int32_t j = first; j < L.s1; j += step) {
        const int32_t w = col[j];
        lo = lower_bound(col, lo, L.l1, w);
        if (lo == L.l1) break;
        if (col[lo] == w) {
            const uint32_t ms = mask[j], ml = mask[lo];
            add_pair(c, L.short_is_u ? ms : ml, L.short_is_u ? ml : ms);
        }
    }
}

__device__ __forceinline__ void store16(int32_t* __restrict__ out, const int32_t (&c)[16])
{
    int4* o = reinterpret_cast<int4*>(out);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = make_int4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
}

// tier 0: one lane per key
__global__ void __launch_bounds__(kThreads) motif_lane_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col,
                                                                const uint8_t* __restrict__ mask,
                                                                const int32_t* __restrict__ ids, int64_t n_ids,
                                                                int32_t* __restrict__ counts)
{
    for (int64_t e = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; e < n_ids; e += int64_t(gridDim.x) * blockDim.x) {
        const int32_t idx = ids ? ids[e] : static_cast<int32_t>(e);
        const Lists L = lists_of(keys, n, rowptr, idx);
        int32_t c[16] = {};
        intersect(col, mask, L, L.s0, 1, c);
        store16(counts + int64_t(idx) * 16, c);
    }
}

// tier 1: one wavefront per key; lane k of the reduced wavefront writes counter k
__global__ void __launch_bounds__(kThreads) motif_wave_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col,
                                                                const uint8_t* __restrict__ mask,
                                                                const int32_t* __restrict__ ids, int64_t n_ids,
                                                                int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = int64_t(gridDim.x) * (kThreads / 64);
    for (int64_t e = blockIdx.x * int64_t(kThreads / 64) + (threadIdx.x >> 6); e < n_ids; e += waves) {
        const int32_t idx = ids ? ids[e] : static_cast<int32_t>(e);
        const Lists L = lists_of(keys, n, rowptr, idx);
        int32_t c[16] = {};
        intersect(col, mask, L, L.s0 + lane, 64, c);
        int32_t mine = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int32_t s = c[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            mine = lane == k ? s : mine;
        }
        if (lane < 16) counts[int64_t(idx) * 16 + lane] = mine;
    }
}

struct NbWorkspace {
    uint64_t* keys_in;
    uint64_t* keys_out;
    int32_t* perm;
    int64_t* head;
    int64_t* pos;
    void* sort_ws;
    void* scan_ws;
    size_t sort_bytes, scan_bytes, total;
};

int nb_workspace(int64_t k, void* base, NbWorkspace* w)
{
    const int64_t m = 2 * k;
    PYGSD_REQUIRE(m <= INT32_MAX, "typed motif neighbourhoods: %lld entries; an int32 CSR holds at most 2^31 - 1 = %d",
                  static_cast<long long>(m), INT32_MAX);
    w->total = 0;
    if (m == 0) return 0;                         // no keys: nothing is sorted (and no device is asked)
    if (int rc = pygsd_sort_keys_u64_workspace(m, &w->sort_bytes)) return rc;
    if (int rc = pygsd_scan_i64_workspace(static_cast<int32_t>(m), &w->scan_bytes)) return rc;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = round_up(off + bytes, 256);
        return at;
    };
    const size_t o_in = take(m * 8), o_out = take(m * 8), o_perm = take(m * 4), o_head = take(m * 8),
                 o_pos = take((m + 1) * 8), o_sort = take(w->sort_bytes), o_scan = take(w->scan_bytes);
    w->total = off + 256;                         // room to align the base
    if (base) {
        char* b = align256(base);
        w->keys_in = reinterpret_cast<uint64_t*>(b + o_in);
        w->keys_out = reinterpret_cast<uint64_t*>(b + o_out);
        w->perm = reinterpret_cast<int32_t*>(b + o_perm);
        w->head = reinterpret_cast<int64_t*>(b + o_head);
        w->pos = reinterpret_cast<int64_t*>(b + o_pos);
        w->sort_ws = b + o_sort;
        w->scan_ws = b + o_scan;
    }
    return 0;
}

}  // namespace
}  // namespace pygsd

using namespace pygsd;

extern "C" int pygsd_motif_workspace(int64_t n_keys, size_t* bytes)
{
    PYGSD_REQUIRE(bytes, "pygsd_motif_workspace: null pointer");
    PYGSD_REQUIRE(n_keys >= 0, "pygsd_motif_workspace: negative key count");
    NbWorkspace w;
    if (int rc = nb_workspace(n_keys, nullptr, &w)) return rc;
    *bytes = w.total;
    return 0;
}

extern "C" int pygsd_motif_neighbourhoods(const int64_t* keys, const uint8_t* flags, int64_t n_keys, int32_t n,
                                          int32_t* rowptr, int32_t* col, uint8_t* mask, void* workspace,
                                          size_t workspace_bytes, void* stream)
{
    PYGSD_REQUIRE(n_keys >= 0 && n >= 0, "pygsd_motif_neighbourhoods: negative key or node count");
    PYGSD_REQUIRE(2 * n_keys <= INT32_MAX,
                  "pygsd_motif_neighbourhoods: %lld typed entries; an int32 CSR holds at most 2^31 - 1 = %d",
                  static_cast<long long>(2 * n_keys), INT32_MAX);
    PYGSD_REQUIRE(rowptr, "pygsd_motif_neighbourhoods: null pointer");
    PYGSD_REQUIRE(n_keys == 0 || (n > 0 && keys && flags && col && mask && workspace),
                  "pygsd_motif_neighbourhoods: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_keys == 0) {
        PYGSD_HIP_TRY(hipMemsetAsync(rowptr, 0, (static_cast<size_t>(n) + 1) * sizeof(int32_t), s));
        return 0;
    }
    NbWorkspace w;
    if (int rc = nb_workspace(n_keys, workspace, &w)) return rc;
    PYGSD_REQUIRE(workspace_bytes >= w.total, "pygsd_motif_neighbourhoods: workspace of %zu bytes, %zu needed",
                  workspace_bytes, w.total);
    const int64_t m = 2 * n_keys;
    hipLaunchKernelGGL(nb_emit_kernel, dim3(grid_for(n_keys)), dim3(kThreads), 0, s, keys, n_keys, int64_t(n), w.keys_in);
    if (int rc = check_launch("nb_emit_kernel")) return rc;
    const uint64_t nn = static_cast<uint64_t>(n) * static_cast<uint64_t>(n);
    if (int rc = pygsd_sort_keys_u64(w.keys_in, w.keys_out, w.perm, m, bits_for(nn - 1), w.sort_ws, w.sort_bytes, s))
        return rc;
    hipLaunchKernelGGL(nb_head_kernel, dim3(grid_for(m)), dim3(kThreads), 0, s, w.keys_out, m, w.head);
    if (int rc = check_launch("nb_head_kernel")) return rc;
    if (int rc = pygsd_scan_i64(w.head, static_cast<int32_t>(m), w.pos, w.scan_ws, w.scan_bytes, s)) return rc;
    hipLaunchKernelGGL(nb_compact_kernel, dim3(grid_for(m)), dim3(kThreads), 0, s, w.keys_out, w.perm, flags, n_keys,
                       int64_t(n), m, w.pos, col, mask);
    if (int rc = check_launch("nb_compact_kernel")) return rc;
    hipLaunchKernelGGL(nb_rowptr_kernel, dim3(grid_for(int64_t(n) + 1)), dim3(kThreads), 0, s, w.keys_out, m, int64_t(n),
                       w.pos, rowptr);
    return check_launch("nb_rowptr_kernel");
}

extern "C" int pygsd_motif_count(const int64_t* keys, int64_t n_keys, int32_t n, const int32_t* rowptr, const int32_t* col,
                                 const uint8_t* mask, const int32_t* ids, int64_t n_ids, int32_t tier, int32_t* counts,
                                 void* stream)
{
    PYGSD_REQUIRE(n_keys >= 0 && n >= 0 && n_ids >= 0, "pygsd_motif_count: negative count");
    PYGSD_REQUIRE(n_keys <= INT32_MAX && n_ids <= n_keys, "pygsd_motif_count: %lld keys, %lld ids",
                  static_cast<long long>(n_keys), static_cast<long long>(n_ids));
    PYGSD_REQUIRE(tier == 0 || tier == 1, "pygsd_motif_count: tier %d (0: lane per key, 1: wavefront per key)", tier);
    if (n_ids == 0) return 0;
    PYGSD_REQUIRE(n > 0 && keys && rowptr && col && mask && counts && (ids || n_ids == n_keys),
                  "pygsd_motif_count: null pointer");
    PYGSD_REQUIRE(aligned16(counts), "pygsd_motif_count: counts must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    if (tier == 0) {
        hipLaunchKernelGGL(motif_lane_kernel, dim3(grid_for(n_ids)), dim3(kThreads), 0, s, keys, int64_t(n), rowptr, col,
                           mask, ids, n_ids, counts);
        return check_launch("motif_lane_kernel");
    }
    hipLaunchKernelGGL(motif_wave_kernel, dim3(grid_for(n_ids, kThreads / 64)), dim3(kThreads), 0, s, keys, int64_t(n),
                       rowptr, col, mask, ids, n_ids, counts);
    return check_launch("motif_wave_kernel");
}
