// Perron vectors and symmetrised PageRank operators: the first-order operators of DiGCN
// (utils/directed/get_adjs_DiGCN.py:get_appr_directed_adj) and DiGCL (cal_fast_appr).  include/pygsd_hip.h documents
// the pipeline.
//
// Power iteration: every step is two plain launches over the transposed transition matrix (int32 CSR, rows split over
// groups of `lanes` lanes of a wavefront, float64 accumulation, no atomics).
//   pr_step_kernel  : y = M x (+ teleport), and per-block partials of sum(y) and sum(z * x).
//   pr_update_kernel: every block reduces those partials in the same fixed order (so every block holds bit-identical
//                     scalars), writes the new x and per-block partials of the change of x.
// The stopping rule is evaluated by the next step's pr_step_kernel, again redundantly and identically in every block:
// once it holds, block 0 sets status[0] and every later launch returns at once.  status[1] counts the completed
// steps.  The host enqueues steps in batches and reads `status` once per batch.
//
// Symmetrisation: one wavefront per row merges row i of P and row i of P^T (ascending columns, duplicates adjacent)
// along the merge path; the first merged slot of each column sums both runs in slot order and forms
// 1/2 (sqrt(pi_i) P_ij pi_j^-1/2 + pi_i^-1/2 P_ji sqrt(pi_j)).  Count pass, pygsd_scan_i64, emit pass, as the
// intersection merge of spgemm.hip.
#include <cmath>

#include "common.hpp"

namespace pygsd {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kParts = PYGSD_PAGERANK_PARTIALS;
// work[] layout (doubles): step partials of sum(y) | of sum(z * x) | update partials of the change | t | |t' - t|
constexpr int kSumY = 0, kSumZX = kParts, kDiff = 2 * kParts, kT = 3 * kParts, kDt = 3 * kParts + 1;

inline unsigned blocks_for(int64_t items, int64_t per_block)
{
    int64_t g = (items + per_block - 1) / per_block;
    if (g > kParts) g = kParts;
    if (g < 1) g = 1;
    return static_cast<unsigned>(g);
}

// Sum over the block in a fixed order (wave butterfly, then the wave sums in wave order); every thread gets it.
__device__ double block_sum(double v, double* lds)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                              // the previous call's readers are done with lds
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) s += lds[w];
    return s;
}

__device__ double sum_partials(const double* p, int n, double* lds)
{
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) v += p[i];
    return block_sum(v, lds);
}

struct StepArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const double* val64;   // mode 0: (1 - alpha) P^T per slot
    const float* val32;    // mode 1: W per slot
    const double* z;       // mode 1: z per node
    int32_t n, lanes, mode, max_steps;
    int32_t g_step, g_update;
    double alpha, c, tol;
    double* x;
    double* y;
    double* work;
    int64_t* status;
};

__global__ __launch_bounds__(kThreads) void pr_step_kernel(StepArgs a)
{
    __shared__ double lds[kWaves];
    __shared__ int64_t st[2];
    if (threadIdx.x == 0) {                       // one read per block: block 0 may set status[0] meanwhile
        st[0] = a.status[0];
        st[1] = a.status[1];
    }
    __syncthreads();
    if (st[0]) return;
    const int64_t steps = st[1];
    if (steps > 0) {
        bool done = steps >= a.max_steps;
        if (!done) {
            const double d = sum_partials(a.work + kDiff, a.g_update, lds);
            done = a.mode == 0 ? d + a.work[kDt] < a.tol : sqrt(d) <= a.tol;
        }
        if (done) {
            if (blockIdx.x == 0 && threadIdx.x == 0) a.status[0] = 1;
            return;
        }
    }
    const int L = a.lanes;
    const int lane = threadIdx.x & 63, sub = lane & (L - 1);
    const int per_wave = 64 / L;
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWaves;
    const double teleport = a.mode == 0 ? a.work[kT] / a.n : 0.0;
    double acc_y = 0.0, acc_zx = 0.0;
    for (int64_t base = (static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * per_wave; base < a.n;
         base += n_waves * per_wave) {
        const int64_t j = base + lane / L;
        double s = 0.0;
        if (j < a.n) {
            const int64_t e1 = a.rowptr[j + 1];
            for (int64_t e = a.rowptr[j] + sub; e < e1; e += L) {
                const double w = a.mode == 0 ? a.val64[e] : static_cast<double>(a.val32[e]);
                s += w * a.x[a.col[e]];
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (sub == 0 && j < a.n) {
            const double v = s + teleport;
            a.y[j] = v;
            acc_y += v;
            acc_zx += (a.z ? a.z[j] : 1.0) * a.x[j];
        }
    }
    const double py = block_sum(acc_y, lds);
    const double pzx = block_sum(acc_zx, lds);
    if (threadIdx.x == 0) {
        a.work[kSumY + blockIdx.x] = py;
        a.work[kSumZX + blockIdx.x] = pzx;
    }
}

// mode 0 (augmented): s = sum(y) + alpha sum(x); x' = y / s, t' = alpha sum(x) / s; partials of |x' - x|.
// mode 1 (fast):      x' = y + c (z^T x); partials of (x' - x)^2.
__global__ __launch_bounds__(kThreads) void pr_update_kernel(StepArgs a)
{
    __shared__ double lds[kWaves];
    if (a.status[0]) return;
    const double sy = a.mode == 0 ? sum_partials(a.work + kSumY, a.g_step, lds) : 0.0;
    const double szx = sum_partials(a.work + kSumZX, a.g_step, lds);
    const double nt = a.alpha * szx, s = sy + nt, shift = a.c * szx;
    double acc = 0.0;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < a.n;
         j += static_cast<int64_t>(gridDim.x) * kThreads) {
        const double xo = a.x[j];
        const double xn = a.mode == 0 ? a.y[j] / s : a.y[j] + shift;
        const double d = xn - xo;
        acc += a.mode == 0 ? fabs(d) : d * d;
        a.x[j] = xn;
    }
    const double p = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        a.work[kDiff + blockIdx.x] = p;
        if (blockIdx.x == 0) {
            if (a.mode == 0) {
                const double tn = nt / s;
                a.work[kDt] = fabs(tn - a.work[kT]);
                a.work[kT] = tn;
            }
            a.status[1] += 1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void pr_sum_kernel(const double* __restrict__ x, int32_t n, double* __restrict__ part)
{
    __shared__ double lds[kWaves];
    double acc = 0.0;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * kThreads)
        acc += x[j];
    const double p = block_sum(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

__global__ __launch_bounds__(kThreads) void pr_divide_kernel(const double* __restrict__ x, int32_t n,
                                                             const double* __restrict__ part, int32_t n_part,
                                                             double* __restrict__ pi)
{
    __shared__ double lds[kWaves];
    const double s = sum_partials(part, n_part, lds);
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * kThreads)
        pi[j] = x[j] / s;
}

// one thread per row, slots in order
__global__ void pr_row_sum_kernel(const int32_t* __restrict__ rowptr, const double* __restrict__ val, int32_t n,
                                  double* __restrict__ out)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        double s = 0.0;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s += val[e];
        out[i] = s;
    }
}

// Fast mode, per row i of A (ascending columns): duplicate runs are summed in float32 (as scipy sums duplicates), the
// row sum r_i of the merged entries is formed in float64 and rounded once; inv_i = 1 / r_i (float32, 0 where r_i = 0),
// z_i = z_nz where r_i != 0 else z_zero.
__global__ void pr_fast_rows_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                    const float* __restrict__ w, int32_t n, double z_nz, double z_zero,
                                    float* __restrict__ inv, double* __restrict__ z)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
        double r = 0.0;
        float run = 0.0f;
        for (int64_t e = e0; e < e1; ++e) {
            run = (e > e0 && col[e] == col[e - 1]) ? run + w[e] : 0.0f + w[e];
            if (e + 1 == e1 || col[e + 1] != col[e]) r += static_cast<double>(run);
        }
        const float r32 = static_cast<float>(r);
        inv[i] = r32 != 0.0f ? 1.0f / r32 : 0.0f;
        z[i] = r32 != 0.0f ? z_nz : z_zero;
    }
}

// Fast mode, per row j of A^T: W_ji = fl32(fl32(A_ij * fl32(1 - alpha)) * inv_i) at the first slot of each run of
// equal i (A_ij the run's float32 sum), 0 at the others.
__global__ void pr_fast_weights_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                       const float* __restrict__ w, int32_t n, float damp,
                                       const float* __restrict__ inv, float* __restrict__ out)
{
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n;
         j += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t e1 = rowptr[j + 1];
        for (int64_t e = rowptr[j]; e < e1;) {
            const int32_t i = col[e];
            float a = 0.0f + w[e];
            int64_t f = e + 1;
            for (; f < e1 && col[f] == i; ++f) {
                a += w[f];
                out[f] = 0.0f;
            }
            out[e] = (a * damp) * inv[i];
            e = f;
        }
    }
}

// one side of the merge
struct Side {
    const int32_t* col;
    const double* val64;   // mode 0: P per slot
    const float* val32;    // mode 1: A per slot
};

// Sum of the run of column j starting at slot e (float64 in mode 0; in mode 1 the float32 run sum scaled by the owner's
// inverse row sum in float32, as P = D^-1 A is formed on the host); 0 for an empty run.
__device__ double run_value(const Side& s, int64_t e, int64_t end, int32_t j, const float* inv, bool transposed,
                            int32_t i)
{
    if (e >= end || s.col[e] != j) return 0.0;
    if (s.val64) {
        double v = 0.0;
        for (; e < end && s.col[e] == j; ++e) v += s.val64[e];
        return v;
    }
    float v = 0.0f;
    for (; e < end && s.col[e] == j; ++e) v += s.val32[e];
    return static_cast<double>(inv[transposed ? j : i] * v);
}

struct UnionArgs {
    const int32_t* p_rowptr;
    const int32_t* t_rowptr;
    Side p, t;
    const float* inv;
    const double* sq;
    const double* isq;
    int32_t n, fast;
    int64_t* count;
    const int64_t* c_ptr;
    int32_t* rowptr;
    int32_t* out_col;
    double* out_val;
};

// One wavefront per row i: merged slot k (of |P_i| + |P^T_i|, P's slots first on equal columns) is located by a binary
// search along the merge path; the first merged slot of each column computes the entry.  Offsets are int64 throughout:
// a row's two lengths can sum past INT32_MAX.  emit == 0: count[i] = entries whose sum is not 0 (NaN counts);
// emit != 0: write them at c_ptr[i] in ascending column order.
__global__ __launch_bounds__(kThreads) void pr_union_kernel(UnionArgs u, int emit)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * kWaves;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); i <= u.n; i += waves) {
        if (emit && lane == 0) u.rowptr[i] = static_cast<int32_t>(u.c_ptr[i]);
        if (i == u.n) break;
        const int64_t a0 = u.p_rowptr[i], la = u.p_rowptr[i + 1] - a0;
        const int64_t b0 = u.t_rowptr[i], lb = u.t_rowptr[i + 1] - b0;
        const int32_t* A = u.p.col + a0;
        const int32_t* B = u.t.col + b0;
        const int64_t dst = emit ? u.c_ptr[i] : 0;
        int64_t cnt = 0;
        for (int64_t base = 0; base < la + lb; base += 64) {
            const int64_t k = base + lane;
            bool hit = false;
            double v = 0.0;
            int32_t j = 0;
            if (k < la + lb) {
                int64_t lo = k > lb ? k - lb : 0, hi = k < la ? k : la;
                while (lo < hi) {                     // a = number of P slots among the first k merged slots
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (A[mid] <= B[k - mid - 1]) lo = mid + 1; else hi = mid;
                }
                const int64_t a = lo, b = k - lo;
                j = (a < la && (b >= lb || A[a] <= B[b])) ? A[a] : B[b];
                const int32_t prev = k == 0 ? -1 : max(a > 0 ? A[a - 1] : -1, b > 0 ? B[b - 1] : -1);
                if (prev != j) {                      // first merged slot of column j: both runs start at (a, b)
                    const double pij = run_value(u.p, a0 + a, a0 + la, j, u.inv, false, static_cast<int32_t>(i));
                    const double pji = run_value(u.t, b0 + b, b0 + lb, j, u.inv, true, static_cast<int32_t>(i));
                    // a zero entry of P or P^T contributes nothing (scipy drops zero products before scaling)
                    const double x = pij != 0.0 ? (u.sq[i] * pij) * u.isq[j] : 0.0;
                    const double y = pji == 0.0 ? 0.0
                                     : u.fast ? (u.isq[i] * pji) * u.sq[j] : (u.sq[j] * pji) * u.isq[i];
                    const double sum = x + y;
                    hit = sum != 0.0;
                    v = sum * 0.5;
                    if (u.fast && v != v) v = 0.0;
                }
            }
            const uint64_t m = __ballot(hit);
            if (emit && hit) {
                const int64_t pos = dst + cnt + __popcll(m & ((uint64_t(1) << lane) - 1));
                u.out_col[pos] = j;
                u.out_val[pos] = v;
            }
            cnt += __popcll(m);
        }
        if (!emit && lane == 0) u.count[i] = cnt;
    }
}

// D^-1/2 L D^-1/2 with D = row sums, one thread per row.  mode 0: float64 sums and scaling, rounded once to float32.
// mode 1: the values rounded to float32 first, float32 sums in slot order and float32 scaling.
__global__ void pr_degree_kernel(const int32_t* __restrict__ rowptr, const double* __restrict__ val, int32_t n,
                                 int fast, double* __restrict__ dis)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t e1 = rowptr[i + 1];
        double d;
        if (fast) {
            float s = 0.0f;
            for (int64_t e = rowptr[i]; e < e1; ++e) s += static_cast<float>(val[e]);
            float r = 1.0f / sqrtf(s);
            d = isinf(r) ? 0.0 : static_cast<double>(r);
        } else {
            double s = 0.0;
            for (int64_t e = rowptr[i]; e < e1; ++e) s += val[e];
            d = pow(s, -0.5);
            if (isinf(d)) d = 0.0;
        }
        dis[i] = d;
    }
}

__global__ void pr_apply_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                const double* __restrict__ val, int32_t n, int fast, const double* __restrict__ dis,
                                float* __restrict__ out)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t e1 = rowptr[i + 1];
        for (int64_t e = rowptr[i]; e < e1; ++e) {
            if (fast)
                out[e] = (static_cast<float>(dis[i]) * static_cast<float>(val[e])) * static_cast<float>(dis[col[e]]);
            else
                out[e] = static_cast<float>((dis[i] * val[e]) * dis[col[e]]);
        }
    }
}

}  // namespace
}  // namespace pygsd

using namespace pygsd;

extern "C" int pygsd_pagerank_row_sum_f64(const int32_t* rowptr, const double* val, int32_t n, double* out,
                                          void* stream)
{
    PYGSD_REQUIRE(n >= 0, "pygsd_pagerank_row_sum_f64: negative row count");
    if (n == 0) return 0;
    PYGSD_REQUIRE(rowptr && val && out, "pygsd_pagerank_row_sum_f64: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    hipLaunchKernelGGL(pr_row_sum_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, rowptr, val, n, out);
    return check_launch("pr_row_sum_kernel");
}

extern "C" int pygsd_pagerank_fast_prepare(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val,
                                           const int32_t* t_rowptr, const int32_t* t_col, const float* t_val,
                                           int32_t n, double alpha, float* inv, double* z, float* w_out, void* stream)
{
    PYGSD_REQUIRE(n > 0, "pygsd_pagerank_fast_prepare: n = %d", n);
    PYGSD_REQUIRE(a_rowptr && a_col && a_val && t_rowptr && t_col && t_val && inv && z && w_out,
                  "pygsd_pagerank_fast_prepare: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    const double z_nz = alpha * (1 + alpha), z_zero = (1 - alpha) / (1 + alpha) + alpha * (1 + alpha);
    hipLaunchKernelGGL(pr_fast_rows_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, a_rowptr, a_col, a_val, n, z_nz,
                       z_zero, inv, z);
    if (int rc = check_launch("pr_fast_rows_kernel")) return rc;
    hipLaunchKernelGGL(pr_fast_weights_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, t_rowptr, t_col, t_val, n,
                       static_cast<float>(1 - alpha), inv, w_out);
    return check_launch("pr_fast_weights_kernel");
}

extern "C" int pygsd_pagerank_step(int32_t mode, const int32_t* rowptr, const int32_t* col, const double* val64,
                                   const float* val32, const double* z, int32_t n, int32_t lanes, double alpha,
                                   double c, double tol, int32_t max_steps, int32_t n_steps, double* x, double* y,
                                   double* work, int64_t work_len, int64_t* status, void* stream)
{
    PYGSD_REQUIRE(mode == 0 || mode == 1, "pygsd_pagerank_step: mode %d", mode);
    PYGSD_REQUIRE(n > 0 && n_steps >= 0 && max_steps >= 0, "pygsd_pagerank_step: n=%d n_steps=%d max_steps=%d", n,
                  n_steps, max_steps);
    PYGSD_REQUIRE(lanes >= 1 && lanes <= 64 && (lanes & (lanes - 1)) == 0, "pygsd_pagerank_step: lanes=%d", lanes);
    PYGSD_REQUIRE(work_len >= PYGSD_PAGERANK_WORK, "pygsd_pagerank_step: work holds %lld doubles, %d needed",
                  static_cast<long long>(work_len), PYGSD_PAGERANK_WORK);
    PYGSD_REQUIRE(rowptr && col && x && y && work && status && (mode == 0 ? val64 != nullptr : (val32 && z)),
                  "pygsd_pagerank_step: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    StepArgs a{rowptr, col, mode == 0 ? val64 : nullptr, mode == 1 ? val32 : nullptr, mode == 1 ? z : nullptr,
               n, lanes, mode, max_steps, 0, 0, alpha, c, tol, x, y, work, status};
    a.g_step = static_cast<int32_t>(blocks_for(n, static_cast<int64_t>(kWaves) * (64 / lanes)));
    a.g_update = static_cast<int32_t>(blocks_for(n, kThreads));
    for (int32_t k = 0; k < n_steps; ++k) {
        hipLaunchKernelGGL(pr_step_kernel, dim3(a.g_step), dim3(kThreads), 0, s, a);
        if (int rc = check_launch("pr_step_kernel")) return rc;
        hipLaunchKernelGGL(pr_update_kernel, dim3(a.g_update), dim3(kThreads), 0, s, a);
        if (int rc = check_launch("pr_update_kernel")) return rc;
    }
    return 0;
}

extern "C" int pygsd_pagerank_normalise(const double* x, int32_t n, double* work, int64_t work_len, double* pi,
                                        void* stream)
{
    PYGSD_REQUIRE(n > 0 && work_len >= PYGSD_PAGERANK_WORK, "pygsd_pagerank_normalise: n=%d work_len=%lld", n,
                  static_cast<long long>(work_len));
    PYGSD_REQUIRE(x && work && pi, "pygsd_pagerank_normalise: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    const unsigned g = blocks_for(n, kThreads);
    hipLaunchKernelGGL(pr_sum_kernel, dim3(g), dim3(kThreads), 0, s, x, n, work);
    if (int rc = check_launch("pr_sum_kernel")) return rc;
    hipLaunchKernelGGL(pr_divide_kernel, dim3(g), dim3(kThreads), 0, s, x, n, work, static_cast<int32_t>(g), pi);
    return check_launch("pr_divide_kernel");
}

static int union_launch(const int32_t* p_rowptr, const int32_t* p_col, const double* p_val64, const float* p_val32,
                        const int32_t* t_rowptr, const int32_t* t_col, const double* t_val64, const float* t_val32,
                        const float* inv, const double* sq, const double* isq, int32_t n, int32_t fast, int emit,
                        int64_t* count, const int64_t* c_ptr, int32_t* rowptr, int32_t* out_col, double* out_val,
                        void* stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    UnionArgs u{p_rowptr, t_rowptr, {p_col, fast ? nullptr : p_val64, fast ? p_val32 : nullptr},
                {t_col, fast ? nullptr : t_val64, fast ? t_val32 : nullptr}, inv, sq, isq, n, fast, count, c_ptr,
                rowptr, out_col, out_val};
    hipLaunchKernelGGL(pr_union_kernel, dim3(grid_for(static_cast<int64_t>(n) + 1, kWaves)), dim3(kThreads), 0, s, u,
                       emit);
    return check_launch("pr_union_kernel");
}

#define PYGSD_UNION_INPUTS_OK                                                                                        \
    (p_rowptr && p_col && t_rowptr && t_col && sq && isq &&                                                         \
     (fast ? (p_val32 && t_val32 && inv) : (p_val64 && t_val64)))

extern "C" int pygsd_pagerank_union_count(const int32_t* p_rowptr, const int32_t* p_col, const double* p_val64,
                                          const float* p_val32, const int32_t* t_rowptr, const int32_t* t_col,
                                          const double* t_val64, const float* t_val32, const float* inv,
                                          const double* sq, const double* isq, int32_t n, int32_t fast,
                                          int64_t* count, void* stream)
{
    PYGSD_REQUIRE(n >= 0, "pygsd_pagerank_union_count: negative row count");
    if (n == 0) return 0;
    PYGSD_REQUIRE(PYGSD_UNION_INPUTS_OK && count, "pygsd_pagerank_union_count: null pointer");
    return union_launch(p_rowptr, p_col, p_val64, p_val32, t_rowptr, t_col, t_val64, t_val32, inv, sq, isq, n, fast, 0,
                        count, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int pygsd_pagerank_union_emit(const int32_t* p_rowptr, const int32_t* p_col, const double* p_val64,
                                         const float* p_val32, const int32_t* t_rowptr, const int32_t* t_col,
                                         const double* t_val64, const float* t_val32, const float* inv,
                                         const double* sq, const double* isq, int32_t n, int32_t fast,
                                         const int64_t* c_ptr, int64_t nnz, int32_t* rowptr, int32_t* out_col,
                                         double* out_val, void* stream)
{
    PYGSD_REQUIRE(nnz >= 0 && nnz <= INT32_MAX,
                  "pygsd_pagerank_union_emit: %lld entries; an int32 CSR holds at most 2^31 - 1 = %d",
                  static_cast<long long>(nnz), INT32_MAX);
    PYGSD_REQUIRE(n >= 0 && rowptr && c_ptr, "pygsd_pagerank_union_emit: bad arguments");
    PYGSD_REQUIRE(n == 0 || (PYGSD_UNION_INPUTS_OK && (nnz == 0 || (out_col && out_val))),
                  "pygsd_pagerank_union_emit: null pointer");
    return union_launch(p_rowptr, p_col, p_val64, p_val32, t_rowptr, t_col, t_val64, t_val32, inv, sq, isq, n, fast, 1,
                        nullptr, c_ptr, rowptr, out_col, out_val, stream);
}

extern "C" int pygsd_pagerank_scale(const int32_t* rowptr, const int32_t* col, const double* val, int32_t n,
                                    int32_t fast, double* dis, float* out, void* stream)
{
    PYGSD_REQUIRE(n >= 0, "pygsd_pagerank_scale: negative row count");
    if (n == 0) return 0;
    PYGSD_REQUIRE(rowptr && col && val && dis && out, "pygsd_pagerank_scale: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof(PYGSD_K_BUILD, s);
    hipLaunchKernelGGL(pr_degree_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, rowptr, val, n, fast, dis);
    if (int rc = check_launch("pr_degree_kernel")) return rc;
    hipLaunchKernelGGL(pr_apply_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, rowptr, col, val, n, fast, dis, out);
    return check_launch("pr_apply_kernel");
}
