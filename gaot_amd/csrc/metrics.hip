// Evaluation on the device: the reference's test metric (utils/metrics.py: per-sample, per-variable-chunk relative L1 error, median over
// samples, mean over chunks) and the validation loss with a device-resident running mean (static_trainer.py:204-292,
// sequential_trainer.py:243-320, 417-450).  Three entry points, all deterministic: no floating-point atomics, no tickets -- every
// result is a pure function of its inputs, and no workspace word is read before this call wrote it.
#include "common.h"

using namespace gaot;
#define ST(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int REL_L1_MAX_V = 32;          // variables per node (the per-workgroup fold below keeps 1024 + V entries in LDS)
constexpr int REL_L1_MAX_C = 256;         // chunks: one thread each in the finishing launch
constexpr int REL_L1_MAX_WG = 2048;       // workgroups of the streaming launch (8 per CU: enough loads in flight for the HBM rate)

// ---------------------------------------------------------------- gaot_rel_l1_errors
// A sample's T rows of S = N * V contiguous floats are read as 16-byte vectors; "slot" = the vector a thread owns within a pass.  A
// sample is shared by G = Gj * Gt workgroups: Gj side by side along the row, Gt taking every Gt-th row.  The P active slots of a pass
// (the largest multiple of V that fits Gj * 256 threads; at most V - 1 threads idle) advance by P vectors = 4 P floats, a multiple
// of V, and every row starts at variable 0: the variable of a thread's k-th vector element is (4 slot + k) mod V for the whole launch,
// so the per-variable sums are eight double accumulators in registers with static indices, whatever V is.
struct rel_l1_grid { int Gj, Gt, G; long P; };

static rel_l1_grid rel_l1_plan(int64_t B, int64_t T, int64_t S, int V) {
    const int64_t S4 = (S + 3) / 4;
    int64_t wg = (B * T * S4 + 2047) / 2048;                 // ~2048 vectors (32 KB of each tensor) per workgroup
    wg = wg > REL_L1_MAX_WG ? REL_L1_MAX_WG : wg;
    int64_t G = wg / B; G = G < 1 ? 1 : G;
    int64_t Gj = (S4 + 1023) / 1024; Gj = Gj > G ? G : (Gj < 1 ? 1 : Gj);
    int64_t Gt = G / Gj; Gt = Gt > T ? T : (Gt < 1 ? 1 : Gt);
    rel_l1_grid r;
    r.Gj = (int)Gj; r.Gt = (int)Gt; r.G = (int)(Gj * Gt);
    r.P = (Gj * 256 / V) * V;
    return r;
}

struct rel_l1_args {
    const float* g; const float* p;
    long sbg, stg, sbp, stp;          // element strides of b and t
    long T, S;
    int V, Gj, Gt;
    long P;
    const float* a; const float* b;   // optional affine (both or neither)
    const float* mean; const float* sd;
    double* part;                     // [B][G][2][V]
};

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* row, long j) {
    if (VEC) return reinterpret_cast<const f32x4*>(row)[j];
    const float* q = row + 4 * j;
    return f32x4{q[0], q[1], q[2], q[3]};
}

// the reference's arithmetic, every operation rounded on its own in fp32 (no contraction): x * a + b (trainer_utils.py:145), then
// (x - mean) / std with a true division (metrics.py:38-39), |g - p| and |g| (metrics.py:42, 51); only the sums are wider
__device__ __forceinline__ void rel_l1_term(float g, float p, bool affine, float a, float b, float mean, float sd, double& num, double& den) {
#pragma clang fp contract(off)
    if (affine) {
        g = g * a; g = g + b;
        p = p * a; p = p + b;
    }
    const float gn = (g - mean) / sd, pn = (p - mean) / sd;
    num += (double)fabsf(gn - pn);
    den += (double)fabsf(gn);
}

template <bool VEC>
__global__ __launch_bounds__(256) void rel_l1_partial_kernel(const rel_l1_args A) {
    __shared__ double fold[2][1024 + REL_L1_MAX_V];
    const int V = A.V, tid = threadIdx.x;
    const int G = A.Gj * A.Gt;
    const long bi = blockIdx.x / G;
    const int gw = (int)(blockIdx.x - bi * G), gj = gw % A.Gj, gt = gw / A.Gj;
    const long slot = (long)gj * 256 + tid;
    const bool active = slot < A.P;
    const bool affine = A.a != nullptr;
    float ca[4], cb[4], cm[4], cs[4];
    {
        int v = (int)((4 * slot) % V);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ca[k] = affine ? A.a[v] : 1.f; cb[k] = affine ? A.b[v] : 0.f;
            cm[k] = A.mean[v]; cs[k] = A.sd[v];
            v = v + 1 == V ? 0 : v + 1;
        }
    }
    double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
    const long S4f = A.S / 4;
    const int rem = (int)(A.S - 4 * S4f);
    const float* gb = A.g + bi * A.sbg;
    const float* pb = A.p + bi * A.sbp;
    if (active) {
        for (long t = gt; t < A.T; t += A.Gt) {
            const float* gr = gb + t * A.stg;
            const float* pr = pb + t * A.stp;
            long j = slot;
            for (; j + 3 * A.P < S4f; j += 4 * A.P) {          // four vectors of each tensor in flight
                const f32x4 g0 = load4<VEC>(gr, j), g1 = load4<VEC>(gr, j + A.P), g2 = load4<VEC>(gr, j + 2 * A.P), g3 = load4<VEC>(gr, j + 3 * A.P);
                const f32x4 p0 = load4<VEC>(pr, j), p1 = load4<VEC>(pr, j + A.P), p2 = load4<VEC>(pr, j + 2 * A.P), p3 = load4<VEC>(pr, j + 3 * A.P);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    rel_l1_term(g0[k], p0[k], affine, ca[k], cb[k], cm[k], cs[k], num[k], den[k]);
                    rel_l1_term(g1[k], p1[k], affine, ca[k], cb[k], cm[k], cs[k], num[k], den[k]);
                    rel_l1_term(g2[k], p2[k], affine, ca[k], cb[k], cm[k], cs[k], num[k], den[k]);
                    rel_l1_term(g3[k], p3[k], affine, ca[k], cb[k], cm[k], cs[k], num[k], den[k]);
                }
            }
            for (; j < S4f; j += A.P) {
                const f32x4 g0 = load4<VEC>(gr, j), p0 = load4<VEC>(pr, j);
#pragma unroll
                for (int k = 0; k < 4; ++k) rel_l1_term(g0[k], p0[k], affine, ca[k], cb[k], cm[k], cs[k], num[k], den[k]);
            }
            if (rem != 0 && j == S4f) {          // the row's last, partial vector: scalar loads of the elements that exist
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < rem) rel_l1_term(gr[4 * j + k], pr[4 * j + k], affine, ca[k], cb[k], cm[k], cs[k], num[k], den[k]);
            }
        }
    }
    // per-variable sums of the workgroup: entry e = 4 tid + k belongs to variable (c + e) mod V, c = 1024 gj mod V.  Halve the number of
    // V-wide groups until one is left, always adding entry e + d into entry e with d a multiple of V: a fixed tree, the same bits every run.
    const int n0 = (1024 + V - 1) / V * V;
#pragma unroll
    for (int k = 0; k < 4; ++k) { fold[0][4 * tid + k] = num[k]; fold[1][4 * tid + k] = den[k]; }
    if (tid < n0 - 1024) { fold[0][1024 + tid] = 0.0; fold[1][1024 + tid] = 0.0; }
    __syncthreads();
    for (int cur = n0; cur > V;) {
        const int d = ((cur / V + 1) / 2) * V;
        for (int e = tid; e + d < cur; e += 256) { fold[0][e] += fold[0][e + d]; fold[1][e] += fold[1][e + d]; }
        cur = d;
        __syncthreads();
    }
    if (tid < V) {
        const int v = (int)(((long)gj * 1024 + tid) % V);
        double* out = A.part + (bi * G + gw) * 2 * V;
        out[v] = fold[0][tid];
        out[V + v] = fold[1][tid];
    }
}

// one workgroup per sample: the G partials of every variable in a fixed order (lane-strided, then the butterfly), the variables of a
// chunk in index order, and err = num / (den + 1e-10) in fp32 (metrics.py:56)
__global__ __launch_bounds__(256) void rel_l1_finish_kernel(const double* __restrict__ part, int G, int V, const int* __restrict__ chunk_of_var, int C,
                                                            float* __restrict__ err, long ld_err) {
    __shared__ double tot[2][REL_L1_MAX_V];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double* pb = part + (long)blockIdx.x * G * 2 * V;
    for (int v = w; v < V; v += 4) {
        double n = 0.0, d = 0.0;
        for (int g = lane; g < G; g += 64) { n += pb[(long)g * 2 * V + v]; d += pb[(long)g * 2 * V + V + v]; }
        n = wave_sum_d(n); d = wave_sum_d(d);
        if (lane == 0) { tot[0][v] = n; tot[1][v] = d; }
    }
    __syncthreads();
    if (tid < C) {
#pragma clang fp contract(off)
        double n = 0.0, d = 0.0;
        for (int v = 0; v < V; ++v)
            if (chunk_of_var[v] == tid) { n += tot[0][v]; d += tot[1][v]; }
        const float nf = (float)n, df = (float)d;
        err[(long)blockIdx.x * ld_err + tid] = nf / (df + 1e-10f);
    }
}

// ---------------------------------------------------------------- gaot_median_mean
// torch.median(dim=0) is the element of rank (n - 1) / 2 in sorted order.  Rank by counting: the rank of entry i is the number of entries
// that sort before it, equal values ordered by index, NaN after everything -- exactly one entry has each rank, so exactly one thread
// writes the column's median, a copy of an input element.  O(n^2) comparisons per column, the column staged through LDS 256 at a time:
// any n, no sort buffer.
__device__ __forceinline__ bool sorts_before(float xj, long j, float xi, long i) {
    const bool nj = xj != xj, ni = xi != xi;
    if (nj) return ni && j < i;
    if (ni) return true;
    return xj < xi || (xj == xi && j < i);
}
__global__ __launch_bounds__(256) void median_select_kernel(const float* __restrict__ x, long n, long ld, float* __restrict__ med) {
    __shared__ float tile[256];
    const int c = blockIdx.y, tid = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + tid;
    const float xi = i < n ? x[i * ld + c] : 0.f;
    long rank = 0;
    for (long j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        tile[tid] = j0 + tid < n ? x[(j0 + tid) * ld + c] : 0.f;
        __syncthreads();
        const int m = (int)(n - j0 < 256 ? n - j0 : 256);
        for (int k = 0; k < m; ++k) rank += sorts_before(tile[k], j0 + k, xi, i) ? 1 : 0;
    }
    if (i < n && rank == (n - 1) / 2) med[c] = xi;
}
// a NaN anywhere in a column makes its median NaN (torch.median propagates it); then the mean of the medians, summed in index order
__global__ __launch_bounds__(256) void median_mean_kernel(const float* __restrict__ x, long n, long ld, int C, float* __restrict__ med,
                                                          float* __restrict__ metric) {
    const int tid = threadIdx.x;
    for (int c = 0; c < C; ++c) {
        int bad = 0;
        for (long i = tid; i < n; i += 256) { const float v = x[i * ld + c]; bad |= v != v; }
        bad = __syncthreads_or(bad);
        if (bad && tid == 0) med[c] = __builtin_nanf("");
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += (double)med[c];
        metric[0] = (float)(s / (double)C);
    }
}

// ---------------------------------------------------------------- gaot_mse_loss_eval
// gaot_mse_loss_fwd's two launches with the same partial sums in the same order (the same bits); the finishing launch also adds the
// batch loss into running = {sum (double), batches (double)}
__global__ __launch_bounds__(256) void mse_eval_partial_kernel(const float* __restrict__ p, const float* __restrict__ y, long n, float* __restrict__ part) {
    __shared__ float red[4];
    float s = 0.f;
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 a = reinterpret_cast<const f32x4*>(p)[i], b = reinterpret_cast<const f32x4*>(y)[i];
        const f32x4 d = a - b;
        s += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) { const float d = p[n4 * 4 + threadIdx.x] - y[n4 * 4 + threadIdx.x]; s += d * d; }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(64) void mse_eval_final_kernel(const float* __restrict__ part, int nparts, float inv_n, float* __restrict__ loss,
                                                            double* __restrict__ running) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 64) s += part[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const float l = s * inv_n;
        loss[0] = l;
        running[0] += (double)l;
        running[1] += 1.0;
    }
}
static int mse_eval_blocks(int64_t n) { long b = (n / 4 + 1023) / 1024; return (int)(b < 1 ? 1 : (b > 256 ? 256 : b)); }

}  // namespace

extern "C" int64_t gaot_rel_l1_errors_workspace(int64_t B, int64_t T, int64_t N, int32_t V) {
    if (B <= 0 || T <= 0 || N <= 0 || V <= 0 || V > REL_L1_MAX_V) return 0;
    const rel_l1_grid r = rel_l1_plan(B, T, N * V, V);
    return 2 * (B * r.G * 2 * V);          // doubles, counted in floats
}

extern "C" int gaot_rel_l1_errors(const float* gtr, int64_t gtr_stride_b, int64_t gtr_stride_t, const float* prd, int64_t prd_stride_b,
                                  int64_t prd_stride_t, int64_t B, int64_t T, int64_t N, int32_t V, const float* affine_a,
                                  const float* affine_b, const float* mean, const float* std_, const int32_t* chunk_of_var, int32_t C,
                                  float* workspace, float* err_out, int64_t ld_err, gaot_stream_t stream) {
    GAOT_REQUIRE(gtr && prd && mean && std_ && chunk_of_var && workspace && err_out, "rel_l1_errors: null pointer");
    GAOT_REQUIRE(B > 0 && T > 0 && N > 0 && B <= (int64_t)1 << 20 && T <= (int64_t)1 << 31 && N <= (int64_t)1 << 40, "rel_l1_errors: bad shape B=%lld T=%lld N=%lld",
                 (long long)B, (long long)T, (long long)N);
    GAOT_REQUIRE(V >= 1 && V <= REL_L1_MAX_V, "rel_l1_errors: V=%d variables, at most %d are supported", V, REL_L1_MAX_V);
    GAOT_REQUIRE(C >= 1 && C <= REL_L1_MAX_C && ld_err >= C, "rel_l1_errors: C=%d chunks (1..%d) with row stride %lld", C, REL_L1_MAX_C, (long long)ld_err);
    GAOT_REQUIRE((affine_a == nullptr) == (affine_b == nullptr), "rel_l1_errors: the affine needs both a and b, or neither");
    const int64_t S = N * V;
    GAOT_REQUIRE((T == 1 || (gtr_stride_t >= S && prd_stride_t >= S)) && (B == 1 || (gtr_stride_b >= S && prd_stride_b >= S)),
                 "rel_l1_errors: the [N, V] block is contiguous, so the strides of b and t are at least N * V = %lld elements", (long long)S);
    GAOT_REQUIRE((reinterpret_cast<uintptr_t>(gtr) & 3u) == 0 && (reinterpret_cast<uintptr_t>(prd) & 3u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(err_out) & 3u) == 0, "rel_l1_errors: float pointers are 4-byte aligned, the workspace 8-byte");
    const rel_l1_grid r = rel_l1_plan(B, T, S, V);
    rel_l1_args A;
    A.g = gtr; A.p = prd;
    A.sbg = B == 1 ? 0 : gtr_stride_b; A.stg = T == 1 ? 0 : gtr_stride_t;
    A.sbp = B == 1 ? 0 : prd_stride_b; A.stp = T == 1 ? 0 : prd_stride_t;
    A.T = T; A.S = S; A.V = V; A.Gj = r.Gj; A.Gt = r.Gt; A.P = r.P;
    A.a = affine_a; A.b = affine_b; A.mean = mean; A.sd = std_;
    A.part = reinterpret_cast<double*>(workspace);
    // 16-byte loads where every row of both tensors starts on a 16-byte boundary, scalar loads elsewhere
    const bool vec = aligned16(gtr) && aligned16(prd) && A.sbg % 4 == 0 && A.stg % 4 == 0 && A.sbp % 4 == 0 && A.stp % 4 == 0;
    const dim3 grid((unsigned)(B * r.G));
    if (vec) hipLaunchKernelGGL(rel_l1_partial_kernel<true>, grid, dim3(256), 0, ST(stream), A);
    else hipLaunchKernelGGL(rel_l1_partial_kernel<false>, grid, dim3(256), 0, ST(stream), A);
    hipLaunchKernelGGL(rel_l1_finish_kernel, dim3((unsigned)B), dim3(256), 0, ST(stream), A.part, r.G, (int)V, chunk_of_var, (int)C, err_out, (long)ld_err);
    GAOT_CHECK_LAUNCH("gaot_rel_l1_errors");
    return GAOT_OK;
}

extern "C" int gaot_median_mean(const float* errs, int64_t n, int32_t C, int64_t ld, float* median_out, float* metric_out, gaot_stream_t stream) {
    GAOT_REQUIRE(errs && median_out && metric_out, "median_mean: null pointer");
    GAOT_REQUIRE(n >= 1 && n <= (int64_t)1 << 31 && C >= 1 && C <= 65535 && ld >= C, "median_mean: n=%lld rows (1..2^31) of C=%d columns (1..65535), row stride %lld",
                 (long long)n, C, (long long)ld);
    hipLaunchKernelGGL(median_select_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)C), dim3(256), 0, ST(stream), errs, (long)n, (long)ld, median_out);
    hipLaunchKernelGGL(median_mean_kernel, dim3(1), dim3(256), 0, ST(stream), errs, (long)n, (long)ld, (int)C, median_out, metric_out);
    GAOT_CHECK_LAUNCH("gaot_median_mean");
    return GAOT_OK;
}

extern "C" int gaot_mse_loss_eval(const float* pred, const float* target, int64_t n, float* partial, float* loss, double* running, gaot_stream_t stream) {
    GAOT_REQUIRE(pred && target && partial && loss && running && n > 0 && aligned16(pred) && aligned16(target) && (reinterpret_cast<uintptr_t>(running) & 7u) == 0,
                 "mse_loss_eval: bad arguments (16-byte aligned inputs, partial[256], running = two doubles)");
    const int nb = mse_eval_blocks(n);
    hipLaunchKernelGGL(mse_eval_partial_kernel, dim3(nb), dim3(256), 0, ST(stream), pred, target, (long)n, partial);
    hipLaunchKernelGGL(mse_eval_final_kernel, dim3(1), dim3(64), 0, ST(stream), partial, nb, 1.0f / (float)n, loss, running);
    GAOT_CHECK_LAUNCH("gaot_mse_loss_eval");
    return GAOT_OK;
}
