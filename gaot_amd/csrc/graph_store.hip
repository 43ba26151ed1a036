// Dataset-level graph building for variable-coordinate (vx) runs: what the reference's GraphBuilder.build_graphs_for_split
// (datasets/graph_builder.py:28-87) does sample by sample in Python -- rescale(x, (-1, 1)) (utils/scaling.py:10-35), then 2 x len(scales)
// radius searches against the shared latent grid -- for ALL S samples of a split in a fixed number of launches.
//
//   gaot_rescale_batch      x[S, N, d] -> ((x - min) / range) * 2 + (-1) per sample and dimension, range 0 -> 1; every operation rounded on
//                           its own (__fsub_rn / __fdiv_rn / __fmul_rn / __fadd_rn: no reciprocal, no contraction) = the torch expression bit
//                           for bit.  One workgroup per sample (grid-strided over S).
//   gaot_graph_store_count  one cell list over the LATENT points (shared by every sample; the grid spans [-1 - cell, 1 + cell]^d, so no
//                           bounding box is read back: rescaled points lie in [-1, 1]^d, latent points further out clamp into border cells
//                           and simply fail the distance test), then one thread per (sample, physical point) walks the 3^d cells around
//                           its point: its hit count is the DECODER row's length, and every hit adds 1 to the ENCODER row of the token it
//                           hit (integer atomics that only count).  Batched scans turn both into per-sample row splits (each sample's start
//                           at 0) and per-sample totals and maxima -- the one thing the host reads back.
//   gaot_graph_store_fill   the same walk again writes both directions' rows into arenas at 64-bit offsets; all rows are then sorted
//                           ascending (rows hold distinct indices: the sorted row is unique, whatever order the atomics handed out slots
//                           in), and one thread per edge links the two directions: the distance test (radius.hip `within`, copied
//                           unchanged) is exactly symmetric, so the decoder list IS the transpose of the encoder list, and each
//                           direction's transposed CSR (t_splits, t_edge) reads off the other's -- t_splits is the other's row splits,
//                           t_edge the position of the mate edge, found by bisection in the mate's sorted row; ascending inside a source
//                           because the mates of a row lie in rows of ascending number.
//
// Row-length thresholds of the row sort (segsort.h, on the int64 arenas): rows of <= 32 entries are insertion-sorted by one thread; rows of
// 33 .. 4096 entries by one workgroup ranking in LDS; rows of more than 4096 entries by one workgroup ranking against global memory through
// `sort_scratch`.  The walk itself is one thread per physical point for any row length (latent cells are small: a token grid).
//
// Launches: rescale 1, count 7, fill 7 (walk, absolute starts, 2 x 2 of the segment sorts, link) -- none depends on S (grid dimensions do).
// Nothing here allocates, synchronises or keeps state.
//
// Not measured outside the 2-D shape of tools/graph_store_bench.py: the cell scan is ONE 1 024-thread workgroup over up to 2^22 cells
// (serial chunks of up to 4 096 cells per thread), and in 3-D with a small radius the cell floor (at most 161 cells per axis) puts many
// tokens into each cell, which the one-thread-per-point walk then tests one by one.  Correct, but its cost there is unknown.
#include "common.h"
#include "segsort.h"

using namespace gaot;
#define ST(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int GS_MAX_Y = 32768;          // samples per grid.y; more are strided over

struct LatentGrid {
    float o;              // origin of every axis
    float inv_cell;
    int n;                // cells per axis
    int dim;
    int ncell;
};

// cell slightly larger than r (as neighbor_search.py's caller-side grid here: the +-1 cell reach then holds with margin against the
// rounding of (v - o) / cell), at least 2 / 2048, grown until the grid has at most 2^22 cells
LatentGrid latent_grid(int dim, float radius) {
    double cell = (double)radius * 1.001;
    if (cell < 2.0 / 2048.0) cell = 2.0 / 2048.0;
    LatentGrid g;
    g.dim = dim;
    for (;;) {
        const double n = floor((2.0 + 2.0 * cell) / cell) + 1.0;
        const double total = dim == 3 ? n * n * n : n * n;
        if (total <= (double)(1 << 22)) { g.n = (int)n; g.ncell = (int)total; break; }
        cell *= 1.5;
    }
    g.o = (float)(-1.0 - cell);
    g.inv_cell = (float)(1.0 / cell);
    return g;
}

__device__ __forceinline__ int axis_cell(float v, const LatentGrid& g) { return (int)floorf((v - g.o) * g.inv_cell); }
__device__ __forceinline__ int clamp_cell(int c, int n) { return c < 0 ? 0 : (c >= n ? n - 1 : c); }
__device__ __forceinline__ int latent_cell(const LatentGrid& g, const float* __restrict__ p) {
    const int cx = clamp_cell(axis_cell(p[0], g), g.n);
    const int cy = clamp_cell(axis_cell(p[1], g), g.n);
    const int cz = g.dim == 3 ? clamp_cell(axis_cell(p[2], g), g.n) : 0;
    return (cz * g.n + cy) * g.n + cx;
}

// radius.hip `within`, unchanged: separate roundings of the squares and of their sum, no FMA.  q - d and d - q are exact negations of each
// other, so within(q, d) == within(d, q) for every pair, ties at dist == r included.
__device__ __forceinline__ bool within(const float* __restrict__ q, const float* __restrict__ d, int dim, float r) {
    float s = 0.f;
    for (int k = 0; k < dim; ++k) {
        const float df = __fsub_rn(q[k], d[k]);
        s = __fadd_rn(s, __fmul_rn(df, df));
    }
    return __fsqrt_rn(s) <= r;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rescale
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void rescale_batch_kernel(const float* __restrict__ x, int S, int N, int dim, float* __restrict__ out) {
    __shared__ float red[2][3][16];
    __shared__ float lohi[2][3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int s = blockIdx.x; s < S; s += gridDim.x) {
        const float* __restrict__ xs = x + (long)s * N * dim;
        float* __restrict__ os = out + (long)s * N * dim;
        float mn[3], mx[3];
        for (int k = 0; k < 3; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
        for (int i = t; i < N; i += 1024)
            for (int k = 0; k < dim; ++k) {
                const float v = xs[(long)i * dim + k];
                mn[k] = fminf(mn[k], v);
                mx[k] = fmaxf(mx[k], v);
            }
        for (int k = 0; k < dim; ++k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
                mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
            }
            if (lane == 0) { red[0][k][wave] = mn[k]; red[1][k][wave] = mx[k]; }
        }
        __syncthreads();
        if (t < dim) {
            float a = red[0][t][0], b = red[1][t][0];
            for (int w = 1; w < 16; ++w) { a = fminf(a, red[0][t][w]); b = fmaxf(b, red[1][t][w]); }
            float range = __fsub_rn(b, a);
            if (range == 0.f) range = 1.f;
            lohi[0][t] = a;
            lohi[1][t] = range;
        }
        __syncthreads();
        const int total = N * dim;
        for (int e = t; e < total; e += 1024) {
            const int k = e % dim;
            const float nrm = __fdiv_rn(__fsub_rn(xs[e], lohi[0][k]), lohi[1][k]);
            os[e] = __fadd_rn(__fmul_rn(nrm, 2.0f), -1.0f);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// latent cell list
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void gs_zero_kernel(int* __restrict__ p, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = 0;
}
__global__ void gs_cell_count_kernel(const float* __restrict__ lat, int Q, LatentGrid g, int* __restrict__ cell_id, int* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    const int c = latent_cell(g, lat + (long)i * g.dim);
    cell_id[i] = c;
    atomicAdd(&cnt[c], 1);
}
__global__ __launch_bounds__(1024) void gs_cell_scan_kernel(const int* __restrict__ cnt, int n, int* __restrict__ start) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int chunk = (n + 1023) / 1024;
    const int b = min(n, t * chunk), e = min(n, b + chunk);
    int s = 0;
    for (int i = b; i < e; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = (t == 0) ? 0 : part[t - 1];
    for (int i = b; i < e; ++i) { start[i] = run; run += cnt[i]; }
    if (t == 1023) start[n] = part[1023];
}
// (the order of a cell's tokens depends on the atomics; every row they end up in is sorted afterwards)
__global__ void gs_cell_fill_kernel(const int* __restrict__ cell_id, int Q, const int* __restrict__ start, int* __restrict__ cnt, int* __restrict__ pts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    const int c = cell_id[i];
    pts[start[c] + atomicSub(&cnt[c], 1) - 1] = i;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the walk: one thread per (sample, physical point).  FILL = false: count; FILL = true: write both directions' rows (unsorted)
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void gs_walk_kernel(const float* __restrict__ xs, int S, int N, const float* __restrict__ lat, int Q, LatentGrid g,
                                                      float r, const int* __restrict__ start, const int* __restrict__ pts, int* __restrict__ enc_deg,
                                                      int* __restrict__ dec_deg, const int64_t* __restrict__ off, const int* __restrict__ enc_sp,
                                                      const int* __restrict__ dec_sp, int64_t* __restrict__ enc_index, int64_t* __restrict__ dec_index) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    for (int s = blockIdx.y; s < S; s += gridDim.y) {
        const float* p = xs + ((long)s * N + n) * g.dim;
        int lo[3], hi[3];
        bool empty = false;
        for (int k = 0; k < 3; ++k) {
            if (k >= g.dim) { lo[k] = hi[k] = 0; continue; }
            const int c = axis_cell(p[k], g);
            lo[k] = max(c - 1, 0);
            hi[k] = min(c + 1, g.n - 1);
            if (lo[k] > hi[k]) empty = true;
        }
        int* edeg = enc_deg + (long)s * Q;
        int64_t ebase = 0, dbase = 0;
        const int* esp = nullptr;
        if (FILL) {
            ebase = off[s];
            esp = enc_sp + (long)s * (Q + 1);
            dbase = ebase + dec_sp[(long)s * (N + 1) + n];
        }
        int count = 0;
        if (!empty)
            for (int cz = lo[2]; cz <= hi[2]; ++cz)
                for (int cy = lo[1]; cy <= hi[1]; ++cy)
                    for (int cx = lo[0]; cx <= hi[0]; ++cx) {
                        const int c = (cz * g.n + cy) * g.n + cx;
                        for (int t = start[c]; t < start[c + 1]; ++t) {
                            const int q = pts[t];
                            if (!within(lat + (long)q * g.dim, p, g.dim, r)) continue;
                            if (FILL) {
                                dec_index[dbase + count] = q;
                                const int slot = atomicSub(&edeg[q], 1) - 1;          // the row's slots, handed out in arrival order: sorted below
                                enc_index[ebase + esp[q] + slot] = n;
                            } else {
                                atomicAdd(&edeg[q], 1);
                            }
                            ++count;
                        }
                    }
        if (!FILL) dec_deg[(long)s * N + n] = count;
    }
}

// per-sample exclusive scan of deg[S, L] -> sp64 / sp32 [S, L + 1] (each sample's at 0); stats[s * 3 + 0] = the sample's total (when
// `total_too`), stats[s * 3 + col] = its longest row
__global__ __launch_bounds__(1024) void gs_scan_rows_kernel(const int* __restrict__ deg, int S, int L, int64_t* __restrict__ sp64, int* __restrict__ sp32,
                                                            int64_t* __restrict__ stats, int col, int total_too) {
    __shared__ long part[1024];
    __shared__ int top[1024];
    const int t = threadIdx.x;
    const int chunk = (L + 1023) / 1024;
    const int b = min(L, t * chunk), e = min(L, b + chunk);
    for (int s = blockIdx.x; s < S; s += gridDim.x) {
        const int* __restrict__ cnt = deg + (long)s * L;
        long sum = 0;
        int mx = 0;
        for (int i = b; i < e; ++i) { sum += cnt[i]; mx = max(mx, cnt[i]); }
        part[t] = sum;
        top[t] = mx;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long v = (t >= o) ? part[t - o] : 0;
            const int w = (t >= o) ? top[t - o] : 0;
            __syncthreads();
            part[t] += v;
            top[t] = max(top[t], w);
            __syncthreads();
        }
        long run = (t == 0) ? 0 : part[t - 1];
        int64_t* __restrict__ o64 = sp64 + (long)s * (L + 1);
        int* __restrict__ o32 = sp32 + (long)s * (L + 1);
        for (int i = b; i < e; ++i) { o64[i] = run; o32[i] = (int)run; run += cnt[i]; }
        if (t == 1023) {
            o64[L] = part[1023];
            o32[L] = (int)part[1023];
            if (total_too) stats[(long)s * 3] = part[1023];
            stats[(long)s * 3 + col] = top[1023];
        }
        __syncthreads();
    }
}

// absolute row starts of both arenas for the segment sort: abs[s * (L + 1) + i] = off[s] + sp[s][i] (the closing entry of a sample is the
// next sample's start: an empty segment), abs[S * (L + 1)] = off[S]
__global__ void gs_abs_starts_kernel(const int64_t* __restrict__ off, int S, const int* __restrict__ enc_sp, int Q, const int* __restrict__ dec_sp, int N,
                                     int64_t* __restrict__ enc_abs, int64_t* __restrict__ dec_abs) {
    const long ne = (long)S * (Q + 1), nd = (long)S * (N + 1);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i <= ne + nd + 1; i += (long)gridDim.x * blockDim.x) {
        if (i < ne) enc_abs[i] = off[i / (Q + 1)] + enc_sp[i];
        else if (i == ne) enc_abs[ne] = off[S];
        else if (i - ne - 1 < nd) dec_abs[i - ne - 1] = off[(i - ne - 1) / (N + 1)] + dec_sp[i - ne - 1];
        else dec_abs[nd] = off[S];
    }
}

// one thread per ENCODER edge (sample s, local id e): its row q by bisection in the sample's splits, its source n from the sorted list, its
// mate (the decoder edge n -> q) by bisection in decoder row n.  Writes the int32 plan arrays of both directions, exactly as
// gaot_csr_prepare / gaot_csr_transpose leave them.
__global__ __launch_bounds__(256) void gs_link_kernel(int S, int N, int Q, const int64_t* __restrict__ off, const int* __restrict__ enc_sp,
                                                      const int* __restrict__ dec_sp, const int64_t* __restrict__ enc_index,
                                                      const int64_t* __restrict__ dec_index, int* __restrict__ enc_i32, int* __restrict__ dec_i32,
                                                      int* __restrict__ enc_eq, int* __restrict__ dec_eq, int* __restrict__ enc_te, int* __restrict__ dec_te) {
    for (int s = blockIdx.y; s < S; s += gridDim.y) {
        const int64_t base = off[s];
        const int E = (int)(off[s + 1] - base);
        const int* __restrict__ esp = enc_sp + (long)s * (Q + 1);
        const int* __restrict__ dsp = dec_sp + (long)s * (N + 1);
        for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
            int lo = 0, hi = Q;                       // esp[lo] <= e < esp[hi]
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (esp[mid] <= e) lo = mid; else hi = mid; }
            const int q = lo;
            const int n = (int)enc_index[base + e];
            const int a = dsp[n], b = dsp[n + 1];
            int l = a, h = b;                         // first position of row n holding a token >= q: the mate
            while (l < h) { const int mid = (l + h) >> 1; if (dec_index[base + mid] < q) l = mid + 1; else h = mid; }
            const int d = l < b ? l : b - 1;
            enc_i32[base + e] = n;
            enc_eq[base + e] = q;
            dec_te[base + e] = d;
            dec_i32[base + d] = q;
            dec_eq[base + d] = n;
            enc_te[base + d] = e;
        }
    }
}

// scratch layout (int32 words unless noted): cell_id[Q] cell_cnt[ncell + 1] cell_start[ncell + 1] cell_pts[Q] enc_deg[S Q] dec_deg[S N],
// then (8-byte aligned) int64 enc_abs[S (Q + 1) + 1] dec_abs[S (N + 1) + 1]
struct Scratch {
    int *cell_id, *cell_cnt, *cell_start, *cell_pts, *enc_deg, *dec_deg;
    int64_t *enc_abs, *dec_abs;
    int64_t bytes;
};
Scratch carve(void* p, int S, int N, int Q, const LatentGrid& g) {
    Scratch s;
    int* w = static_cast<int*>(p);
    long at = 0;
    s.cell_id = w + at; at += Q;
    s.cell_cnt = w + at; at += g.ncell + 1;
    s.cell_start = w + at; at += g.ncell + 1;
    s.cell_pts = w + at; at += Q;
    s.enc_deg = w + at; at += (long)S * Q;
    s.dec_deg = w + at; at += (long)S * N;
    at = (at + 1) & ~1L;
    s.enc_abs = reinterpret_cast<int64_t*>(w + at); at += 2 * ((long)S * (Q + 1) + 1);
    s.dec_abs = reinterpret_cast<int64_t*>(w + at); at += 2 * ((long)S * (N + 1) + 1);
    s.bytes = at * 4;
    return s;
}

int check_shape(const char* who, int32_t S, int32_t N, int32_t Q, int32_t dim, float radius) {
    GAOT_REQUIRE(S > 0 && N > 0 && Q > 0 && (dim == 2 || dim == 3), "%s: need S, N, Q > 0 and dim 2 or 3", who);
    GAOT_REQUIRE(radius >= 0.f && radius == radius && radius < 1e30f, "%s: radius must be finite and >= 0", who);
    const int64_t rows = N > Q ? N : Q;
    GAOT_REQUIRE((int64_t)S * (rows + 1) < ((int64_t)1 << 31) - 1, "%s: S * (max(N, Q) + 1) must stay below 2^31", who);
    return GAOT_OK;
}

}  // namespace

extern "C" int gaot_rescale_batch(const float* x, int32_t S, int32_t N, int32_t dim, float* out, gaot_stream_t stream) {
    GAOT_REQUIRE(x && out && S > 0 && N > 0 && dim >= 1 && dim <= 3, "rescale_batch: null pointer, empty shape or dim outside 1..3");
    GAOT_REQUIRE((int64_t)N * dim < (int64_t)1 << 31, "rescale_batch: one sample must stay below 2^31 elements");
    hipLaunchKernelGGL(rescale_batch_kernel, dim3(S < 4096 ? S : 4096), dim3(1024), 0, ST(stream), x, S, N, dim, out);
    GAOT_CHECK_LAUNCH("gaot_rescale_batch");
    return GAOT_OK;
}

extern "C" int64_t gaot_graph_store_scratch(int32_t S, int32_t N, int32_t Q, int32_t dim, float radius) {
    if (check_shape("graph_store_scratch", S, N, Q, dim, radius) != GAOT_OK) return -1;
    return carve(nullptr, S, N, Q, latent_grid(dim, radius)).bytes;
}

extern "C" int gaot_graph_store_count(const float* xs, int32_t S, int32_t N, const float* latent, int32_t Q, int32_t dim, float radius,
                                      int64_t* enc_splits, int64_t* dec_splits, int32_t* enc_splits32, int32_t* dec_splits32, int64_t* stats,
                                      void* scratch, gaot_stream_t stream) {
    if (int rc = check_shape("graph_store_count", S, N, Q, dim, radius)) return rc;
    GAOT_REQUIRE(xs && latent && enc_splits && dec_splits && enc_splits32 && dec_splits32 && stats && scratch, "graph_store_count: null pointer");
    GAOT_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "graph_store_count: scratch must be 8-byte aligned");
    const LatentGrid g = latent_grid(dim, radius);
    const Scratch w = carve(scratch, S, N, Q, g);
    hipStream_t st = ST(stream);
    // the two counters, cell_cnt and enc_deg, start at zero whatever the scratch held: one launch clears cell_cnt .. the end of enc_deg
    // (the words in between, cell_start and cell_pts, are written below anyway)
    const long nz = (w.enc_deg + (long)S * Q) - w.cell_cnt;
    hipLaunchKernelGGL(gs_zero_kernel, dim3(cap_blocks(nz, 256, 4096)), dim3(256), 0, st, w.cell_cnt, nz);
    hipLaunchKernelGGL(gs_cell_count_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, latent, Q, g, w.cell_id, w.cell_cnt);
    hipLaunchKernelGGL(gs_cell_scan_kernel, dim3(1), dim3(1024), 0, st, w.cell_cnt, g.ncell, w.cell_start);
    hipLaunchKernelGGL(gs_cell_fill_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, w.cell_id, Q, w.cell_start, w.cell_cnt, w.cell_pts);
    hipLaunchKernelGGL(gs_walk_kernel<false>, dim3(cdiv(N, 256), S < GS_MAX_Y ? S : GS_MAX_Y), dim3(256), 0, st, xs, S, N, latent, Q, g, radius,
                       w.cell_start, w.cell_pts, w.enc_deg, w.dec_deg, (const int64_t*)nullptr, (const int*)nullptr, (const int*)nullptr,
                       (int64_t*)nullptr, (int64_t*)nullptr);
    const int sb = S < 4096 ? S : 4096;
    hipLaunchKernelGGL(gs_scan_rows_kernel, dim3(sb), dim3(1024), 0, st, w.enc_deg, S, Q, enc_splits, enc_splits32, stats, 1, 1);
    hipLaunchKernelGGL(gs_scan_rows_kernel, dim3(sb), dim3(1024), 0, st, w.dec_deg, S, N, dec_splits, dec_splits32, stats, 2, 0);
    GAOT_CHECK_LAUNCH("gaot_graph_store_count");
    return GAOT_OK;
}

extern "C" int gaot_graph_store_fill(const float* xs, int32_t S, int32_t N, const float* latent, int32_t Q, int32_t dim, float radius,
                                     const int64_t* offsets, int64_t total, int32_t max_edges, int32_t max_row, const int32_t* enc_splits32,
                                     const int32_t* dec_splits32, int64_t* enc_index, int64_t* dec_index, int32_t* enc_index32,
                                     int32_t* dec_index32, int32_t* enc_edge_query, int32_t* dec_edge_query, int32_t* enc_t_edge,
                                     int32_t* dec_t_edge, void* scratch, int64_t* sort_scratch, gaot_stream_t stream) {
    if (int rc = check_shape("graph_store_fill", S, N, Q, dim, radius)) return rc;
    GAOT_REQUIRE(xs && latent && offsets && enc_splits32 && dec_splits32 && scratch, "graph_store_fill: null pointer");
    GAOT_REQUIRE(total >= 0 && max_edges >= 0 && max_edges <= total, "graph_store_fill: total / max_edges (the largest sample's count) out of range");
    GAOT_REQUIRE(total == 0 || (enc_index && dec_index && enc_index32 && dec_index32 && enc_edge_query && dec_edge_query && enc_t_edge && dec_t_edge),
                 "graph_store_fill: null arena with edges to write");
    GAOT_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "graph_store_fill: scratch must be 8-byte aligned");
    GAOT_REQUIRE(max_row >= 0 && (sort_scratch || max_row <= SEGSORT_LDS_BYTES / 8), "graph_store_fill: rows of more than %d entries need sort_scratch (total int64)",
                 SEGSORT_LDS_BYTES / 8);
    if (total == 0) return GAOT_OK;
    const LatentGrid g = latent_grid(dim, radius);
    const Scratch w = carve(scratch, S, N, Q, g);
    hipStream_t st = ST(stream);
    const int gy = S < GS_MAX_Y ? S : GS_MAX_Y;
    hipLaunchKernelGGL(gs_walk_kernel<true>, dim3(cdiv(N, 256), gy), dim3(256), 0, st, xs, S, N, latent, Q, g, radius, w.cell_start, w.cell_pts,
                       w.enc_deg, (int*)nullptr, offsets, enc_splits32, dec_splits32, enc_index, dec_index);
    const long nabs = (long)S * (Q + 1) + (long)S * (N + 1) + 2;
    hipLaunchKernelGGL(gs_abs_starts_kernel, dim3(cap_blocks(nabs, 256, 4096)), dim3(256), 0, st, offsets, S, enc_splits32, Q, dec_splits32, N,
                       w.enc_abs, w.dec_abs);
    sort_segments<int64_t, int64_t>(w.enc_abs, S * (Q + 1), enc_index, sort_scratch, st);
    sort_segments<int64_t, int64_t>(w.dec_abs, S * (N + 1), dec_index, sort_scratch, st);
    hipLaunchKernelGGL(gs_link_kernel, dim3(cap_blocks(max_edges, 256, 2048), gy), dim3(256), 0, st, S, N, Q, offsets, enc_splits32, dec_splits32,
                       enc_index, dec_index, enc_index32, dec_index32, enc_edge_query, dec_edge_query, enc_t_edge, dec_t_edge);
    GAOT_CHECK_LAUNCH("gaot_graph_store_fill");
    return GAOT_OK;
}
