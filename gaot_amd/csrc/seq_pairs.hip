// Sequential (time-dependent) training batches composed on the device from resident trajectories: the reference's DynamicPairDataset
// item (datasets/data_utils.py:162-235) and TestDataset item (:355-402) for a DEVICE list of B indices, one launch each.  Nothing about
// the batch but its shape is a launch argument, so a captured step replays with new indices (sequential.PairStore, trainer.bind_pairs).
//
//   pairs:  idx[b] -> sample = idx / P, pair = idx % P (data_utils.py:169-170), t_in / t_out from the pair tables
//           x[b,n,:] = [(u_in - u_mean) / u_std, (c_in - c_mean) / c_std, start_norm[pair], (diff_norm[pair])]     (n_time = 1: no diff column,
//                                                                                                                    cond[b] = start_norm[pair])
//           y[b,n,:] = mode 0 (u_out - u_mean) / u_std | 1 ((u_out - u_in) - a_mean) / a_std | 2 (((u_out - u_in) / diff[pair]) - a_mean) / a_std
//   test:   x0[b,n,:] = [(u - u_mean) / u_std, (c - c_mean) / c_std, 0, 0] at tidx[0];  yseq[b,k] = u[idx[b], tidx[k + 1]] as stored
//
// Every operation is rounded on its own, in the reference's order (__fsub_rn / __fdiv_rn: no contraction, no reciprocal multiply): the
// results equal the reference's fp32 tensor expressions bit for bit.  Slab offsets are 64-bit (S T N U passes 2^31 bytes at a few
// hundred samples); the position inside one [N, W] block is 32-bit.  Indices outside their range are clamped and *status_flag |= 1 (the
// sample / pair index) or |= 2 (a time index from a table): no read leaves the trajectories.
//
// Thread map: grid.y = the batch item, grid.x strides over the item's output elements in storage order -- consecutive lanes write
// consecutive floats of x (rows are U + Cc + n_time wide, odd in general: no 16-byte alignment to build on) and of y, and read the
// contiguous [N, U] slabs at consecutive (y) or nearly consecutive (x: U of every W lanes) addresses.
#include "common.h"

using namespace gaot;
#define ST(s) reinterpret_cast<hipStream_t>(s)

namespace {

struct seq_src {
    const float* u; const float* c;
    int S, T, N, U, Cc;
    const float* u_mean; const float* u_std; const float* c_mean; const float* c_std;
};

struct seq_pairs_args {
    seq_src d;
    const int32_t* t_in; const int32_t* t_out; const float* start_norm; const float* diff_norm; const float* diff;
    int P;
    const float* a_mean; const float* a_std;
    int mode, n_time;
    const int32_t* idx;
    float* x; float* y; float* cond; int32_t* flag;
};

struct seq_test_args {
    seq_src d;
    const int32_t* idx; const int32_t* tidx;
    int K;
    float* x0; float* yseq; int32_t* flag;
};

__device__ __forceinline__ int clamp_index(long v, long n, int& bad) {
    if (v < 0) { bad = 1; return 0; }
    if (v >= n) { bad = 1; return (int)(n - 1); }
    return (int)v;
}

// the [N, W] input block of one item: normalised u and c of slab (s, t), then the time columns t0 (and t1 when n_time = 2)
__device__ __forceinline__ void input_rows(const seq_src& d, int s, int t, float t0, float t1, int n_time, float* __restrict__ xb) {
    const int U = d.U, Cc = d.Cc, W = U + Cc + n_time;
    const long slab = (long)s * d.T + t;
    const float* __restrict__ ui = d.u + slab * ((long)d.N * U);
    const float* __restrict__ ci = Cc > 0 ? d.c + slab * ((long)d.N * Cc) : nullptr;
    const unsigned total = (unsigned)d.N * (unsigned)W;
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const unsigned n = e / (unsigned)W;
        const int col = (int)(e - n * (unsigned)W);
        float v;
        if (col < U) {
            v = __fdiv_rn(__fsub_rn(ui[n * (unsigned)U + col], d.u_mean[col]), d.u_std[col]);
        } else if (col < U + Cc) {
            const int k = col - U;
            v = ci[n * (unsigned)Cc + k];
            if (d.c_mean != nullptr) v = __fdiv_rn(__fsub_rn(v, d.c_mean[k]), d.c_std[k]);
        } else {
            v = col == U + Cc ? t0 : t1;
        }
        xb[e] = v;
    }
}

__global__ __launch_bounds__(256) void seq_pairs_compose_kernel(const seq_pairs_args a) {
    const seq_src& d = a.d;
    const int b = blockIdx.y;
    int bad = 0, bad_t = 0;
    const int id = clamp_index(a.idx[b], (long)d.S * a.P, bad);
    const int s = id / a.P, p = id - s * a.P;
    const int ti = clamp_index(a.t_in[p], d.T, bad_t), to = clamp_index(a.t_out[p], d.T, bad_t);
    const int flags = bad | (bad_t << 1);
    if (flags && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.flag, flags);
    const float sn = a.start_norm[p];
    const int W = d.U + d.Cc + a.n_time;
    input_rows(d, s, ti, sn, a.diff_norm[p], a.n_time, a.x + (long)b * d.N * W);
    if (a.cond != nullptr && blockIdx.x == 0 && threadIdx.x == 0) a.cond[b] = sn;

    const int U = d.U;
    const long NU = (long)d.N * U;
    const float* __restrict__ ui = d.u + ((long)s * d.T + ti) * NU;
    const float* __restrict__ uo = d.u + ((long)s * d.T + to) * NU;
    float* __restrict__ yb = a.y + (long)b * NU;
    const float df = a.diff[p];
    const unsigned total = (unsigned)NU;
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int col = (int)(e % (unsigned)U);
        float v;
        if (a.mode == 0) {
            v = __fdiv_rn(__fsub_rn(uo[e], d.u_mean[col]), d.u_std[col]);
        } else {
            float r = __fsub_rn(uo[e], ui[e]);
            if (a.mode == 2) r = __fdiv_rn(r, df);
            v = __fdiv_rn(__fsub_rn(r, a.a_mean[col]), a.a_std[col]);
        }
        yb[e] = v;
    }
}

__global__ __launch_bounds__(256) void seq_test_compose_kernel(const seq_test_args a) {
    const seq_src& d = a.d;
    const int b = blockIdx.y;
    int bad = 0, bad_t = 0;
    const int s = clamp_index(a.idx[b], d.S, bad);
    const int t0 = clamp_index(a.tidx[0], d.T, bad_t);
    const long NU = (long)d.N * d.U;
    input_rows(d, s, t0, 0.f, 0.f, 2, a.x0 + (long)b * d.N * (d.U + d.Cc + 2));
    const unsigned total = (unsigned)NU;
    for (int k = 0; k < a.K; ++k) {
        const int t = clamp_index(a.tidx[k + 1], d.T, bad_t);
        const float* __restrict__ src = d.u + ((long)s * d.T + t) * NU;
        float* __restrict__ dst = a.yseq + ((long)b * a.K + k) * NU;
        for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) dst[e] = src[e];
    }
    const int flags = bad | (bad_t << 1);
    if (flags && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.flag, flags);
}

int seq_src_check(const char* who, const seq_src& d, int32_t B, int32_t extra_cols) {
    GAOT_REQUIRE(d.u && d.S > 0 && d.T > 0 && d.N > 0 && d.U > 0 && d.Cc >= 0 && (d.Cc == 0 || d.c), "%s: null trajectories or empty shape", who);
    GAOT_REQUIRE(d.u_mean && d.u_std && ((d.c_mean == nullptr) == (d.c_std == nullptr)) && (d.Cc > 0 || d.c_mean == nullptr),
                 "%s: u statistics missing, or c statistics given by halves / without c", who);
    GAOT_REQUIRE(B > 0 && B <= 65535, "%s: batch of %d items (1..65535)", who, B);
    GAOT_REQUIRE((int64_t)d.N * (d.U + d.Cc + extra_cols) < (int64_t)1 << 31, "%s: one item's [N, width] block must stay below 2^31 elements", who);
    return GAOT_OK;
}

}  // namespace

extern "C" int gaot_seq_pairs_compose(const float* u, const float* c, int32_t S, int32_t T, int32_t N, int32_t U, int32_t Cc, const int32_t* t_in,
                                      const int32_t* t_out, const float* start_norm, const float* diff_norm, const float* diff, int32_t P,
                                      const float* u_mean, const float* u_std, const float* c_mean, const float* c_std, const float* a_mean,
                                      const float* a_std, int32_t mode, int32_t n_time, const int32_t* idx, int32_t B, float* x, float* y, float* cond,
                                      int32_t* status_flag, gaot_stream_t stream) {
    seq_pairs_args a;
    a.d = seq_src{u, c, S, T, N, U, Cc, u_mean, u_std, c_mean, c_std};
    GAOT_REQUIRE(n_time == 1 || n_time == 2, "seq_pairs_compose: n_time must be 1 or 2");
    if (int rc = seq_src_check("seq_pairs_compose", a.d, B, n_time)) return rc;
    GAOT_REQUIRE(t_in && t_out && start_norm && diff_norm && diff && P > 0 && (int64_t)S * P < (int64_t)1 << 31,
                 "seq_pairs_compose: null pair table, or S * P does not fit 31 bits");
    GAOT_REQUIRE(mode >= 0 && mode <= 2 && (mode == 0 || (a_mean && a_std)), "seq_pairs_compose: mode 0 output, 1 residual, 2 time_der (1, 2 need a_mean / a_std)");
    GAOT_REQUIRE(idx && x && y && status_flag && (n_time == 2 || cond), "seq_pairs_compose: null index list / output / status flag (n_time = 1 needs cond)");
    a.t_in = t_in; a.t_out = t_out; a.start_norm = start_norm; a.diff_norm = diff_norm; a.diff = diff; a.P = P;
    a.a_mean = a_mean; a.a_std = a_std; a.mode = mode; a.n_time = n_time; a.idx = idx;
    a.x = x; a.y = y; a.cond = n_time == 1 ? cond : nullptr; a.flag = status_flag;
    const int gx = cap_blocks((long)N * (U + Cc + n_time), 256, 1024);
    hipLaunchKernelGGL(seq_pairs_compose_kernel, dim3(gx, B), dim3(256), 0, ST(stream), a);
    GAOT_CHECK_LAUNCH("gaot_seq_pairs_compose");
    return GAOT_OK;
}

extern "C" int gaot_seq_test_compose(const float* u, const float* c, int32_t S, int32_t T, int32_t N, int32_t U, int32_t Cc, const float* u_mean,
                                     const float* u_std, const float* c_mean, const float* c_std, const int32_t* idx, int32_t B, const int32_t* tidx,
                                     int32_t K, float* x0, float* yseq, int32_t* status_flag, gaot_stream_t stream) {
    seq_test_args a;
    a.d = seq_src{u, c, S, T, N, U, Cc, u_mean, u_std, c_mean, c_std};
    if (int rc = seq_src_check("seq_test_compose", a.d, B, 2)) return rc;
    GAOT_REQUIRE(idx && tidx && K >= 0 && x0 && (K == 0 || yseq) && status_flag, "seq_test_compose: null index list / time list / output / status flag");
    a.idx = idx; a.tidx = tidx; a.K = K; a.x0 = x0; a.yseq = yseq; a.flag = status_flag;
    const int gx = cap_blocks((long)N * (U + Cc + 2), 256, 1024);
    hipLaunchKernelGGL(seq_test_compose_kernel, dim3(gx, B), dim3(256), 0, ST(stream), a);
    GAOT_CHECK_LAUNCH("gaot_seq_test_compose");
    return GAOT_OK;
}
