// Static (time-independent) training batches gathered on the device from a resident dataset: the reference's static trainer takes
// c[i], u[i] and -- vx -- the rescaled coordinates of sample i from its datasets per item, collates and uploads them every step
// (datasets/data_utils.py, static_trainer.py:160-202).  Here the three arrays stay on the device and ONE launch copies the blocks of a
// DEVICE list of B sample indices into the step's static buffers.  Nothing about the batch but its shape is a launch argument, so a
// captured step replays with new indices (static.SampleStore, trainer.bind_samples).
//
//   x[b] = c[idx[b]]   [N, Cc]        y[b] = u[idx[b]]   [N, U]        xcoord[b] = xs[idx[b]]   [N, D]   (xs = NULL: fx, no such copy)
//
// c and u are stored normalised, as the reference's data processor leaves them: a pure copy, equal bit for bit.  Slab offsets are
// 64-bit; the position inside one [N, width] block is 32-bit.  An index outside [0, S) is clamped and *status_flag |= 1: no read leaves
// the dataset.
//
// Thread map: grid.z = the array, grid.y = the batch item, grid.x strides over the block in storage order -- consecutive lanes move
// consecutive 16-byte pieces where the block is a whole number of them and both base pointers are 16-byte aligned (then every slab is),
// consecutive floats otherwise.
#include "common.h"

using namespace gaot;
#define ST(s) reinterpret_cast<hipStream_t>(s)

namespace {

struct sample_gather_args {
    const float* src[3]; float* dst[3];
    unsigned n[3];          // floats per block
    int vec[3];             // 16-byte copies apply
    int S;
    const int32_t* idx; int32_t* flag;
};

__global__ __launch_bounds__(256) void sample_gather_kernel(const sample_gather_args a) {
    const int w = blockIdx.z, b = blockIdx.y;
    const unsigned n = a.n[w];
    if (n == 0) return;
    const int v = a.idx[b];
    const int s = v < 0 ? 0 : (v >= a.S ? a.S - 1 : v);
    if (s != v && w == 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.flag, 1);
    const float* __restrict__ src = a.src[w] + (long)s * n;
    float* __restrict__ dst = a.dst[w] + (long)b * n;
    const unsigned first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (a.vec[w]) {
        const f32x4* __restrict__ s4 = reinterpret_cast<const f32x4*>(src);
        f32x4* __restrict__ d4 = reinterpret_cast<f32x4*>(dst);
        for (unsigned e = first; e < n / 4; e += step) d4[e] = s4[e];
    } else {
        for (unsigned e = first; e < n; e += step) dst[e] = src[e];
    }
}

}  // namespace

extern "C" int gaot_sample_gather(const float* c, const float* u, const float* xs, int32_t S, int32_t N, int32_t Cc, int32_t U, int32_t D,
                                  const int32_t* idx, int32_t B, float* x, float* y, float* xcoord, int32_t* status_flag, gaot_stream_t stream) {
    GAOT_REQUIRE(c && u && S > 0 && N > 0 && Cc > 0 && U > 0, "sample_gather: null dataset or empty shape");
    GAOT_REQUIRE((xs == nullptr) == (xcoord == nullptr) && (xs == nullptr || D > 0), "sample_gather: coordinates need a source, a destination and a width");
    GAOT_REQUIRE(B > 0 && B <= 65535, "sample_gather: batch of %d items (1..65535)", B);
    GAOT_REQUIRE(idx && x && y && status_flag, "sample_gather: null index list / output / status flag");
    const int64_t widest = std::max<int64_t>(std::max(Cc, U), xs ? D : 0);
    GAOT_REQUIRE((int64_t)N * widest < (int64_t)1 << 31, "sample_gather: one item's [N, width] block must stay below 2^31 elements");
    sample_gather_args a;
    const float* srcs[3] = {c, u, xs};
    float* dsts[3] = {x, y, xcoord};
    const int widths[3] = {Cc, U, xs ? D : 0};
    unsigned most = 1;
    for (int w = 0; w < 3; ++w) {
        a.src[w] = srcs[w]; a.dst[w] = dsts[w];
        a.n[w] = (unsigned)N * (unsigned)widths[w];
        a.vec[w] = a.n[w] % 4 == 0 && aligned16(srcs[w]) && aligned16(dsts[w]);
        most = std::max(most, a.vec[w] ? a.n[w] / 4 : a.n[w]);
    }
    a.S = S; a.idx = idx; a.flag = status_flag;
    hipLaunchKernelGGL(sample_gather_kernel, dim3(cap_blocks(most, 256, 1024), B, xs ? 3 : 2), dim3(256), 0, ST(stream), a);
    GAOT_CHECK_LAUNCH("gaot_sample_gather");
    return GAOT_OK;
}
