// Small HBM-bound kernels for the operator variants off the default configuration: rotary position
// embedding, dot-product edge scores, PointNet max pooling, per-edge broadcast, multiscale mixing, and the batched-kernel
// ('nonlinear') integral transform.  One pass over the big operand each, lanes along the contiguous (channel) dimension,
// 16-byte accesses where the shapes allow, no atomics (deterministic), no allocation, no synchronisation.
#include "common.h"

namespace gaot {

// ---------------------------------------------------------------------------------------------
// RoPE (attn.py:106-108 -> rotary_embedding_torch.RotaryEmbedding(dim=head_dim).rotate_queries_or_keys):
// position = sequence index, pairs (2i, 2i+1) of every head rotated by pos * theta^(-2i/D).  In place on the first
// `n_heads` heads of each row of the fused projection output [B*S, ld]; cs = [S, D/2] (cos, sin) interleaved.
// inverse = 1 applies the transposed rotation (the backward of an orthogonal map).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rope_kernel(float* __restrict__ x, long rows, int S, long ld, int n_heads, int D,
                                                   const float2* __restrict__ cs, int inverse) {
    const int half = D / 2;
    const long per_row = (long)n_heads * half;
    const long total = rows * per_row;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const long row = gid / per_row;
        const int rem = (int)(gid % per_row);
        const int h = rem / half, i = rem % half;
        const int s = (int)(row % S);
        const float2 c = cs[(long)s * half + i];
        const float sn = inverse ? -c.y : c.y;
        float2* p = reinterpret_cast<float2*>(x + row * ld + (long)h * D) + i;
        const float2 v = *p;
        // t * cos + rotate_half(t) * sin with rotate_half(x0, x1) = (-x1, x0); products rounded before the sum like the reference
        float2 o;
        o.x = __fadd_rn(__fmul_rn(v.x, c.x), __fmul_rn(-v.y, sn));
        o.y = __fadd_rn(__fmul_rn(v.y, c.x), __fmul_rn(v.x, sn));
        *p = o;
    }
}

// ---------------------------------------------------------------------------------------------
// dot-product edge score (agno.py:215-217): score[e] = scale * <qn[eq[e], :], kn[idx[e], :]>, C channels (64 in the reference).
// 16 lanes per edge when C == 64 (one float4 each), DPP-free butterfly over the lane group.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edge_dot_kernel(const float* __restrict__ qn, const float* __restrict__ kn, int C,
                                                       const int* __restrict__ idx, const int* __restrict__ eq, int E, float scale,
                                                       float* __restrict__ score, int lanes) {
    const int per_block = 256 / lanes;
    const int e = blockIdx.x * per_block + threadIdx.x / lanes;
    const int l = threadIdx.x % lanes;
    float acc = 0.f;
    if (e < E) {
        const float* a = qn + (long)eq[e] * C;
        const float* b = kn + (long)idx[e] * C;
        for (int c = l; c < C; c += lanes) acc += a[c] * b[c];
    }
    for (int off = lanes >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (e < E && l == 0) score[e] = acc * scale;
}

// ---------------------------------------------------------------------------------------------
// segment max pooling over edge rows (PointNet geoembed, gemb.py:217): out[q, c] = max_{e in seg(q)} h[e, c]; empty -> 0.
// backward: the gradient of (q, c) is shared EVENLY by the edges that attain the maximum (the semantics of the stand-in the
// golden vectors were made with, torch scatter_reduce(amax); ties are common: ReLU outputs that are all zero).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segment_max_fwd_kernel(const float* __restrict__ h, int C, const int* __restrict__ sp, int Q,
                                                              float* __restrict__ out) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)Q * C) return;
    const int q = (int)(gid / C), c = (int)(gid % C);
    const int b = sp[q], e = sp[q + 1];
    float m = 0.f;
    if (e > b) {
        m = h[(long)b * C + c];
        for (int t = b + 1; t < e; ++t) m = fmaxf(m, h[(long)t * C + c]);
    }
    out[gid] = m;
}
__global__ __launch_bounds__(256) void segment_max_bwd_kernel(const float* __restrict__ h, const float* __restrict__ out,
                                                              const float* __restrict__ dout, int C, const int* __restrict__ sp, int Q,
                                                              float* __restrict__ dh) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)Q * C) return;
    const int q = (int)(gid / C), c = (int)(gid % C);
    const int b = sp[q], e = sp[q + 1];
    if (e == b) return;
    const float m = out[gid];
    int ties = 0;
    for (int t = b; t < e; ++t) ties += (h[(long)t * C + c] == m) ? 1 : 0;
    const float g = dout[gid] / (float)ties;
    for (int t = b; t < e; ++t) dh[(long)t * C + c] = (h[(long)t * C + c] == m) ? g : 0.f;
}

// ---------------------------------------------------------------------------------------------
// per-edge broadcast (backward of the plain segment sum): dx[b, e, :] = rowscale[eq[e]] * dout[b, eq[e], :]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segment_broadcast_kernel(const float* __restrict__ dout, int B, int E, int C, int Q,
                                                                const int* __restrict__ eq, const float* __restrict__ rowscale,
                                                                float* __restrict__ dx) {
    const long total = (long)B * E * C;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % C);
        const long be = gid / C;
        const int e = (int)(be % E);
        const long b = be / E;
        const int q = eq[e];
        const float s = rowscale ? rowscale[q] : 1.0f;
        dx[gid] = s * dout[(b * Q + q) * C + c];
    }
}

// ---------------------------------------------------------------------------------------------
// multiscale mixing (magno.py:291-303): out[b, q, :] = sum_i w[q, i] * t_i[b, q, :]  (w == nullptr: plain mean over scales)
// backward: dt_i = w[q, i] * dout;  dw[q, i] = sum_b sum_c dout[b, q, c] * t_i[b, q, c]   (one wave per query row)
// ---------------------------------------------------------------------------------------------
struct ScalePtrs { const float* t[8]; float* d[8]; };

__global__ __launch_bounds__(256) void scale_mix_fwd_kernel(ScalePtrs p, int n, const float* __restrict__ w, int B, int Q, int C,
                                                            float* __restrict__ out) {
    const long total = (long)B * Q * C;
    const float inv = 1.0f / (float)n;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int q = (int)((gid / C) % Q);
        float acc = 0.f;
        if (w) { for (int i = 0; i < n; ++i) acc += w[(long)q * n + i] * p.t[i][gid]; }
        else { for (int i = 0; i < n; ++i) acc += p.t[i][gid]; acc *= inv; }       // torch.stack(...).mean(0)
        out[gid] = acc;
    }
}
__global__ __launch_bounds__(256) void scale_mix_bwd_kernel(ScalePtrs p, int n, const float* __restrict__ w, int B, int Q, int C,
                                                            const float* __restrict__ dout, float* __restrict__ dw) {
    // one wave per query row q: lanes stride over (b, c)
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= Q) return;
    const float inv = 1.0f / (float)n;
    float acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int b = 0; b < B; ++b)
        for (int c = lane; c < C; c += 64) {
            const long off = ((long)b * Q + q) * C + c;
            const float g = dout[off];
            for (int i = 0; i < n; ++i) {
                if (dw) acc[i] += g * p.t[i][off];
                if (p.d[i]) p.d[i][off] = (w ? w[(long)q * n + i] : inv) * g;
            }
        }
    if (dw)
        for (int i = 0; i < n; ++i) {
            const float s = wave_sum(acc[i]);
            if (lane == 0) dw[(long)q * n + i] = s;
        }
}

// ---------------------------------------------------------------------------------------------
// 'nonlinear' transforms (agno.py:230-271): the kernel MLP sees f(y_j), so kernel values are per SAMPLE, k[b, e, :].
//   edge_cat      : rows of the kernel MLP  x[b, e, :] = [feat[e, :W0], f[b, idx[e], :C]]
//   bk_reduce     : out[b, q, :] = sum_{e in seg(q)} a_e * k[b, e, :] * (MUL ? f[b, idx[e], :] : 1)
//   bk_edge_grad  : dk[b, e, :] = a_e * dout[b, eq[e], :] * (MUL ? f[b, idx[e], :] : 1)
//   bk_src_grad   : df[b, j, :] = sum_{e : idx[e] = j} ( MUL ? a_e * k[b, e, :] * dout[b, eq[e], :] : 0 ) + dx[b, e, W0:]   (transposed CSR)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edge_cat_kernel(const float* __restrict__ feat, int W0, const float* __restrict__ f, int B,
                                                       int n_src, int C, const int* __restrict__ idx, int E, float* __restrict__ x) {
    const int W = W0 + C;
    const long total = (long)B * E * W;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % W);
        const long be = gid / W;
        const int e = (int)(be % E);
        const long b = be / E;
        x[gid] = c < W0 ? feat[(long)e * W0 + c] : f[(b * n_src + idx[e]) * C + (c - W0)];
    }
}
template <bool MUL>
__global__ __launch_bounds__(256) void bk_reduce_kernel(const float* __restrict__ k, const float* __restrict__ f, int B, int n_src,
                                                        int C, int E, const int* __restrict__ sp, const int* __restrict__ idx, int Q,
                                                        const float* __restrict__ a, float* __restrict__ out) {
    const long total = (long)B * Q * C;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % C);
        const long bq = gid / C;
        const int q = (int)(bq % Q);
        const long b = bq / Q;
        float acc = 0.f;
        for (int t = sp[q]; t < sp[q + 1]; ++t) {
            float v = k[(b * E + t) * C + c];
            if (MUL) v *= f[(b * n_src + idx[t]) * C + c];
            acc += (a ? a[t] : 1.0f) * v;
        }
        out[gid] = acc;
    }
}
template <bool MUL>
__global__ __launch_bounds__(256) void bk_edge_grad_kernel(const float* __restrict__ dout, const float* __restrict__ f, int B, int n_src,
                                                           int C, int E, int Q, const int* __restrict__ idx, const int* __restrict__ eq,
                                                           const float* __restrict__ a, float* __restrict__ dk) {
    const long total = (long)B * E * C;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % C);
        const long be = gid / C;
        const int e = (int)(be % E);
        const long b = be / E;
        float v = (a ? a[e] : 1.0f) * dout[(b * Q + eq[e]) * C + c];
        if (MUL) v *= f[(b * n_src + idx[e]) * C + c];
        dk[gid] = v;
    }
}
template <bool MUL>
__global__ __launch_bounds__(256) void bk_src_grad_kernel(const float* __restrict__ dout, const float* __restrict__ k,
                                                          const float* __restrict__ dx, int W0, int B, int n_src, int C, int E, int Q,
                                                          const int* __restrict__ tsp, const int* __restrict__ tedge,
                                                          const int* __restrict__ eq, const float* __restrict__ a,
                                                          float* __restrict__ df) {
    const int W = W0 + C;
    const long total = (long)B * n_src * C;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % C);
        const long bj = gid / C;
        const int j = (int)(bj % n_src);
        const long b = bj / n_src;
        float acc = 0.f;
        for (int t = tsp[j]; t < tsp[j + 1]; ++t) {
            const int e = tedge[t];
            if (MUL) acc += (a ? a[e] : 1.0f) * k[(b * E + e) * C + c] * dout[(b * Q + eq[e]) * C + c];
            if (dx) acc += dx[(b * E + e) * W + W0 + c];
        }
        df[gid] = acc;
    }
}
// da[e] = sum_b sum_c dout[b, eq[e], c] * k[b, e, c] * (MUL ? f[b, idx[e], c] : 1)       (learned attention only)
template <bool MUL>
__global__ __launch_bounds__(256) void bk_scale_grad_kernel(const float* __restrict__ dout, const float* __restrict__ k,
                                                            const float* __restrict__ f, int B, int n_src, int C, int E, int Q,
                                                            const int* __restrict__ idx, const int* __restrict__ eq,
                                                            float* __restrict__ da) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= E) return;
    float acc = 0.f;
    for (int b = 0; b < B; ++b)
        for (int c = lane; c < C; c += 64) {
            float v = dout[((long)b * Q + eq[e]) * C + c] * k[((long)b * E + e) * C + c];
            if (MUL) v *= f[((long)b * n_src + idx[e]) * C + c];
            acc += v;
        }
    acc = wave_sum(acc);
    if (lane == 0) da[e] = acc;
}

// ---------------------------------------------------------------------------------------------
// ConditionedNorm (mlp.py:74-124): y[b, s, :] = x[b, s, :] * scale[b, :] + shift[b, :]
// backward: dx = dy * scale;  dscale[b, :] = sum_s dy * x;  dshift[b, :] = sum_s dy      (partials over row chunks, summed by the caller)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cond_affine_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int B, long S, int D, float* __restrict__ y) {
    const long total = (long)B * S * D;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int d = (int)(gid % D);
        const long b = gid / (S * D);
        y[gid] = x[gid] * scale[b * D + d] + shift[b * D + d];
    }
}
// grid (chunks, B); block 256 threads = D-strided lanes; part[(chunk * B + b) * 2 * D + {0..D-1: dscale, D..2D-1: dshift}]
__global__ __launch_bounds__(256) void cond_affine_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const float* __restrict__ scale, int B, long S, int D, int rows_per_chunk,
                                                              float* __restrict__ dx, float* __restrict__ part) {
    const int b = blockIdx.y, chunk = blockIdx.x;
    const long s0 = (long)chunk * rows_per_chunk, s1 = min(S, s0 + rows_per_chunk);
    for (int d = threadIdx.x; d < D; d += 256) {
        const float sc = scale[(long)b * D + d];
        float a0 = 0.f, a1 = 0.f;
        for (long s = s0; s < s1; ++s) {
            const long off = ((long)b * S + s) * D + d;
            const float g = dy[off];
            a0 += g * x[off];
            a1 += g;
            dx[off] = g * sc;
        }
        float* o = part + ((long)chunk * B + b) * 2 * D;
        o[d] = a0;
        o[D + d] = a1;
    }
}

}  // namespace gaot

using namespace gaot;
#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int gaot_rope_inplace(float* x, int32_t B, int32_t S, int64_t ld, int32_t n_heads, int32_t head_dim, const float* cos_sin,
                                 int32_t inverse, gaot_stream_t stream) {
    GAOT_REQUIRE(x && cos_sin && B > 0 && S > 0 && n_heads > 0 && head_dim > 0 && head_dim % 2 == 0, "rope: bad arguments (head_dim even)");
    GAOT_REQUIRE(ld >= (int64_t)n_heads * head_dim && ld % 2 == 0 && (reinterpret_cast<uintptr_t>(x) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(cos_sin) & 7u) == 0, "rope: rows must hold n_heads*head_dim floats, 8-byte aligned");
    const long total = (long)B * S * n_heads * (head_dim / 2);
    hipLaunchKernelGGL(rope_kernel, dim3(cap_blocks(total, 256, 8192)), dim3(256), 0, ST(stream), x, (long)B * S, S, (long)ld, n_heads,
                       head_dim, reinterpret_cast<const float2*>(cos_sin), inverse);
    GAOT_CHECK_LAUNCH("gaot_rope_inplace");
    return GAOT_OK;
}

extern "C" int gaot_edge_dot_score(const float* qn, const float* kn, int32_t C, const int32_t* index32, const int32_t* edge_query,
                                   int32_t E, float scale, float* score, gaot_stream_t stream) {
    GAOT_REQUIRE(C > 0 && E >= 0, "edge_dot_score: bad arguments");
    if (E == 0) return GAOT_OK;
    GAOT_REQUIRE(qn && kn && index32 && edge_query && score, "edge_dot_score: null pointer");
    int lanes = 1;
    while (lanes < 64 && lanes * 4 < C) lanes <<= 1;
    hipLaunchKernelGGL(edge_dot_kernel, dim3(cdiv(E, 256 / lanes)), dim3(256), 0, ST(stream), qn, kn, C, index32, edge_query, E, scale,
                       score, lanes);
    GAOT_CHECK_LAUNCH("gaot_edge_dot_score");
    return GAOT_OK;
}

extern "C" int gaot_segment_max_fwd(const float* h, int32_t C, const int32_t* splits32, int32_t Q, float* out, gaot_stream_t stream) {
    GAOT_REQUIRE(splits32 && out && C > 0 && Q >= 0, "segment_max_fwd: bad arguments");
    if (Q == 0) return GAOT_OK;
    hipLaunchKernelGGL(segment_max_fwd_kernel, dim3(cdiv((long)Q * C, 256)), dim3(256), 0, ST(stream), h, C, splits32, Q, out);
    GAOT_CHECK_LAUNCH("gaot_segment_max_fwd");
    return GAOT_OK;
}

extern "C" int gaot_segment_max_bwd(const float* h, const float* out, const float* dout, int32_t C, const int32_t* splits32, int32_t Q,
                                    float* dh, gaot_stream_t stream) {
    GAOT_REQUIRE(splits32 && out && dout && C > 0 && Q >= 0, "segment_max_bwd: bad arguments");
    if (Q == 0) return GAOT_OK;
    hipLaunchKernelGGL(segment_max_bwd_kernel, dim3(cdiv((long)Q * C, 256)), dim3(256), 0, ST(stream), h, out, dout, C, splits32, Q, dh);
    GAOT_CHECK_LAUNCH("gaot_segment_max_bwd");
    return GAOT_OK;
}

extern "C" int gaot_segment_broadcast(const float* dout, int32_t B, int32_t E, int32_t C, int32_t Q, const int32_t* edge_query,
                                      const float* rowscale, float* dx, gaot_stream_t stream) {
    GAOT_REQUIRE(B > 0 && E >= 0 && C > 0 && Q >= 0, "segment_broadcast: bad arguments");
    if (E == 0) return GAOT_OK;
    GAOT_REQUIRE(dout && edge_query && dx, "segment_broadcast: null pointer");
    hipLaunchKernelGGL(segment_broadcast_kernel, dim3(cap_blocks((long)B * E * C, 256, 8192)), dim3(256), 0, ST(stream), dout, B, E, C, Q,
                       edge_query, rowscale, dx);
    GAOT_CHECK_LAUNCH("gaot_segment_broadcast");
    return GAOT_OK;
}

extern "C" int gaot_scale_mix_fwd(const float* const* scales, int32_t n, const float* w, int32_t B, int32_t Q, int32_t C, float* out,
                                  gaot_stream_t stream) {
    GAOT_REQUIRE(scales && out && n >= 1 && n <= 8 && B > 0 && Q > 0 && C > 0, "scale_mix_fwd: 1..8 scales");
    ScalePtrs p;
    for (int i = 0; i < 8; ++i) { p.t[i] = i < n ? scales[i] : nullptr; p.d[i] = nullptr; }
    hipLaunchKernelGGL(scale_mix_fwd_kernel, dim3(cap_blocks((long)B * Q * C, 256, 8192)), dim3(256), 0, ST(stream), p, n, w, B, Q, C, out);
    GAOT_CHECK_LAUNCH("gaot_scale_mix_fwd");
    return GAOT_OK;
}

extern "C" int gaot_scale_mix_bwd(const float* const* scales, float* const* dscales, int32_t n, const float* w, int32_t B, int32_t Q,
                                  int32_t C, const float* dout, float* dw, gaot_stream_t stream) {
    GAOT_REQUIRE(scales && dscales && dout && n >= 1 && n <= 8 && B > 0 && Q > 0 && C > 0, "scale_mix_bwd: 1..8 scales");
    ScalePtrs p;
    for (int i = 0; i < 8; ++i) { p.t[i] = i < n ? scales[i] : nullptr; p.d[i] = i < n ? dscales[i] : nullptr; }
    hipLaunchKernelGGL(scale_mix_bwd_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, ST(stream), p, n, w, B, Q, C, dout, dw);
    GAOT_CHECK_LAUNCH("gaot_scale_mix_bwd");
    return GAOT_OK;
}

extern "C" int gaot_edge_cat(const float* feat, int32_t W0, const float* f, int32_t B, int32_t n_src, int32_t C, const int32_t* index32,
                             int32_t E, float* x, gaot_stream_t stream) {
    GAOT_REQUIRE(W0 >= 0 && B > 0 && C > 0 && E >= 0, "edge_cat: bad arguments");
    if (E == 0) return GAOT_OK;
    GAOT_REQUIRE(f && index32 && x && (W0 == 0 || feat), "edge_cat: null pointer");
    hipLaunchKernelGGL(edge_cat_kernel, dim3(cap_blocks((long)B * E * (W0 + C), 256, 8192)), dim3(256), 0, ST(stream), feat, W0, f, B,
                       n_src, C, index32, E, x);
    GAOT_CHECK_LAUNCH("gaot_edge_cat");
    return GAOT_OK;
}

extern "C" int gaot_gno_bk_reduce(const float* k, const float* f, int32_t B, int32_t n_src, int32_t C, int32_t E, const int32_t* splits32,
                                  const int32_t* index32, int32_t Q, const float* escale, int32_t mul_f, float* out, gaot_stream_t stream) {
    GAOT_REQUIRE(splits32 && out && B > 0 && C > 0 && Q >= 0 && E >= 0 && (!mul_f || f), "gno_bk_reduce: bad arguments");
    if (Q == 0) return GAOT_OK;
    const dim3 grid(cap_blocks((long)B * Q * C, 256, 16384));
    if (mul_f) hipLaunchKernelGGL(bk_reduce_kernel<true>, grid, dim3(256), 0, ST(stream), k, f, B, n_src, C, E, splits32, index32, Q, escale, out);
    else hipLaunchKernelGGL(bk_reduce_kernel<false>, grid, dim3(256), 0, ST(stream), k, f, B, n_src, C, E, splits32, index32, Q, escale, out);
    GAOT_CHECK_LAUNCH("gaot_gno_bk_reduce");
    return GAOT_OK;
}

extern "C" int gaot_gno_bk_backward(const float* dout, const float* k, const float* f, const float* dx, int32_t W0, int32_t B, int32_t n_src,
                                    int32_t C, int32_t E, int32_t Q, const int32_t* index32, const int32_t* edge_query,
                                    const int32_t* t_splits, const int32_t* t_edge, const float* escale, int32_t mul_f, float* dk,
                                    float* df, float* dscale, gaot_stream_t stream) {
    GAOT_REQUIRE(dout && B > 0 && C > 0 && E >= 0 && Q >= 0 && n_src > 0, "gno_bk_backward: bad arguments");
    if (E == 0) return GAOT_OK;
    if (dk) {
        const dim3 grid(cap_blocks((long)B * E * C, 256, 16384));
        if (mul_f) hipLaunchKernelGGL(bk_edge_grad_kernel<true>, grid, dim3(256), 0, ST(stream), dout, f, B, n_src, C, E, Q, index32, edge_query, escale, dk);
        else hipLaunchKernelGGL(bk_edge_grad_kernel<false>, grid, dim3(256), 0, ST(stream), dout, f, B, n_src, C, E, Q, index32, edge_query, escale, dk);
    }
    if (df) {
        GAOT_REQUIRE(t_splits && t_edge, "gno_bk_backward: df needs the transposed CSR");
        const dim3 grid(cap_blocks((long)B * n_src * C, 256, 16384));
        if (mul_f) hipLaunchKernelGGL(bk_src_grad_kernel<true>, grid, dim3(256), 0, ST(stream), dout, k, dx, W0, B, n_src, C, E, Q, t_splits, t_edge, edge_query, escale, df);
        else hipLaunchKernelGGL(bk_src_grad_kernel<false>, grid, dim3(256), 0, ST(stream), dout, k, dx, W0, B, n_src, C, E, Q, t_splits, t_edge, edge_query, escale, df);
    }
    if (dscale) {
        if (mul_f) hipLaunchKernelGGL(bk_scale_grad_kernel<true>, dim3(cdiv(E, 4)), dim3(256), 0, ST(stream), dout, k, f, B, n_src, C, E, Q, index32, edge_query, dscale);
        else hipLaunchKernelGGL(bk_scale_grad_kernel<false>, dim3(cdiv(E, 4)), dim3(256), 0, ST(stream), dout, k, f, B, n_src, C, E, Q, index32, edge_query, dscale);
    }
    GAOT_CHECK_LAUNCH("gaot_gno_bk_backward");
    return GAOT_OK;
}

extern "C" int gaot_cond_affine_fwd(const float* x, const float* scale, const float* shift, int32_t B, int64_t S, int32_t D, float* y,
                                    gaot_stream_t stream) {
    GAOT_REQUIRE(x && scale && shift && y && B > 0 && S > 0 && D > 0, "cond_affine_fwd: bad arguments");
    hipLaunchKernelGGL(cond_affine_fwd_kernel, dim3(cap_blocks((long)B * S * D, 256, 8192)), dim3(256), 0, ST(stream), x, scale, shift, B,
                       (long)S, D, y);
    GAOT_CHECK_LAUNCH("gaot_cond_affine_fwd");
    return GAOT_OK;
}

extern "C" int32_t gaot_cond_affine_bwd_chunks(int64_t S) { return (int32_t)(S >= 4096 ? 64 : (S >= 256 ? 16 : 1)); }

extern "C" int gaot_cond_affine_bwd(const float* x, const float* dy, const float* scale, int32_t B, int64_t S, int32_t D, float* dx,
                                    float* part, gaot_stream_t stream) {
    GAOT_REQUIRE(x && dy && scale && dx && part && B > 0 && S > 0 && D > 0, "cond_affine_bwd: bad arguments");
    const int chunks = gaot_cond_affine_bwd_chunks(S);
    const int rows = (int)((S + chunks - 1) / chunks);
    hipLaunchKernelGGL(cond_affine_bwd_kernel, dim3(chunks, B), dim3(256), 0, ST(stream), x, dy, scale, B, (long)S, D, rows, dx, part);
    GAOT_CHECK_LAUNCH("gaot_cond_affine_bwd");
    return GAOT_OK;
}

// da[e] = <T[e,:], k[e,:]>;  T[e,:] *= a[e]   (learned attention in the linear transform: T = sum_b dOut (*) f from gaot_gno_edge_grad)
namespace gaot {
__global__ __launch_bounds__(256) void edge_rowdot_scale_kernel(float* __restrict__ T, const float* __restrict__ k, const float* __restrict__ a,
                                                                int E, int C, float* __restrict__ da, int lanes) {
    const int per_block = 256 / lanes;
    const int e = blockIdx.x * per_block + threadIdx.x / lanes;
    const int l = threadIdx.x % lanes;
    float acc = 0.f;
    const float ae = e < E ? a[e] : 0.f;
    if (e < E)
        for (int c = l; c < C; c += lanes) {
            const float t = T[(long)e * C + c];
            acc += t * k[(long)e * C + c];
            T[(long)e * C + c] = t * ae;
        }
    for (int off = lanes >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (e < E && l == 0) da[e] = acc;
}
}  // namespace gaot

extern "C" int gaot_edge_rowdot_scale(float* T, const float* k, const float* a, int32_t E, int32_t C, float* da, gaot_stream_t stream) {
    GAOT_REQUIRE(C > 0 && E >= 0, "edge_rowdot_scale: bad arguments");
    if (E == 0) return GAOT_OK;
    GAOT_REQUIRE(T && k && a && da, "edge_rowdot_scale: null pointer");
    int lanes = 1;
    while (lanes < 64 && lanes * 4 < C) lanes <<= 1;
    hipLaunchKernelGGL(gaot::edge_rowdot_scale_kernel, dim3(cdiv(E, 256 / lanes)), dim3(256), 0, ST(stream), T, k, a, E, C, da, lanes);
    GAOT_CHECK_LAUNCH("gaot_edge_rowdot_scale");
    return GAOT_OK;
}

// ---------------------------------------------------------------------------------------------
// autoregressive rollout glue (gaot.py:371-388 input assembly, 432 re-normalisation, 436-476 stepper modes), one pass each:
//   rollout_input : pn[b,n,:] = [state[b,n,:U], static[b,n,:S], t0n, (dtn)]         (n_time = 1 drops the dt column: cond-norm models)
//   rollout_update: den = stepper(pred, state) de-normalised;  state <- (den - u_mean) / u_std
// The arithmetic is the reference's sequence of separately rounded fp32 operations (no contraction into FMAs).
// ---------------------------------------------------------------------------------------------
namespace gaot {
__global__ __launch_bounds__(256) void rollout_input_kernel(const float* __restrict__ state, int U, const float* __restrict__ stat, int S,
                                                            float t0n, float dtn, int n_time, long rows, float* __restrict__ pn) {
    const int W = U + S + n_time;
    const long total = rows * W;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % W);
        const long r = gid / W;
        pn[gid] = c < U ? state[r * U + c] : (c < U + S ? stat[r * S + (c - U)] : (c == U + S ? t0n : dtn));
    }
}
__global__ __launch_bounds__(256) void rollout_update_kernel(const float* __restrict__ pred, float* __restrict__ state, int U,
                                                             const float* __restrict__ u_mean, const float* __restrict__ u_std,
                                                             const float* __restrict__ a_mean, const float* __restrict__ a_std, float dt,
                                                             int mode, long rows, float* __restrict__ den_out) {
    const long total = rows * U;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int c = (int)(gid % U);
        const float um = u_mean[c], us = u_std[c], p = pred[gid];
        float den;
        if (mode == 0) {
            den = __fadd_rn(__fmul_rn(p, us), um);
        } else {
            const float cur = __fadd_rn(__fmul_rn(state[gid], us), um);
            float inc = __fadd_rn(__fmul_rn(p, a_std[c]), a_mean[c]);
            if (mode == 2) inc = __fmul_rn(dt, inc);
            den = __fadd_rn(cur, inc);
        }
        den_out[gid] = den;
        state[gid] = __fdiv_rn(__fsub_rn(den, um), us);
    }
}

// ---------------------------------------------------------------------------------------------
// The decoder's output projection folded into the recovery block (ops._ProjFold; magno.py:345-350 then 640-641: two linear maps with
// nothing in between):  weff = W Wr_a [OC, Cout],  rproj = rowb W^T + b [Q, OC]  and their gradients.  The operands are tiny (OC <= 4
// output channels, C = Cout = 64) except the row bias [Q, C]: as seven library products and reductions the backward was seven launches of
// 5-8 us each; here it is one pass over rowb / g_rproj whose last workgroup (ticket) finishes the small matrices.  Fixed summation
// orders throughout (deterministic).
// ---------------------------------------------------------------------------------------------
template <int OC>
__global__ __launch_bounds__(256) void proj_fold_fwd_kernel(const float* __restrict__ hw, long ldh, const float* __restrict__ hb,
                                                            const float* __restrict__ wa, long lda, const float* __restrict__ rowb, long ldr,
                                                            int Q, int C, int Cout, float* __restrict__ weff, float* __restrict__ rproj, int lanes) {
    const int rpb = 256 / lanes, row = threadIdx.x / lanes, lr = threadIdx.x % lanes, c = lr * 4;
    const bool cok = c < C;
    f32x4 wq[OC];
#pragma unroll
    for (int o = 0; o < OC; ++o) wq[o] = cok ? *reinterpret_cast<const f32x4*>(hw + o * ldh + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r0 = blockIdx.x * rpb; r0 < Q; r0 += gridDim.x * rpb) {        // (every lane of a group runs the shuffles)
        const int r = r0 + row;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (cok && r < Q) v = *reinterpret_cast<const f32x4*>(rowb + (long)r * ldr + c);
#pragma unroll
        for (int o = 0; o < OC; ++o) {
            float d = (v[0] * wq[o][0] + v[1] * wq[o][1]) + (v[2] * wq[o][2] + v[3] * wq[o][3]);
            for (int off = lanes >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
            if (lr == 0 && r < Q) rproj[(long)r * OC + o] = d + (hb ? hb[o] : 0.f);
        }
    }
    // weff = W Wr_a by the LAST workgroup of the grid (the first ones carry the most rows): every output's C-term sum is cut into
    // `segs` stretches over as many threads (a lone thread walking 64 dependent-latency loads took 25 us), joined in stretch order
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ float part[256];
        const int items = OC * Cout;
        const int segs = items >= 256 ? 1 : 256 / items, per = (C + segs - 1) / segs;
        for (int i0 = 0; i0 < items; i0 += 256 / segs) {
            const int i = i0 + (int)threadIdx.x % (256 / segs), sg = (int)threadIdx.x / (256 / segs);
            float acc = 0.f;
            if (i < items && sg < segs) {
                const int o = i / Cout, j = i % Cout;
                const int c1 = min(C, (sg + 1) * per);
#pragma unroll 8
                for (int cc = sg * per; cc < c1; ++cc) acc += hw[o * ldh + cc] * wa[cc * lda + j];
            }
            __syncthreads();
            part[threadIdx.x] = acc;
            __syncthreads();
            if (sg == 0 && i < items) {
                float t = part[threadIdx.x];
                for (int q = 1; q < segs; ++q) t += part[threadIdx.x + q * (256 / segs)];
                weff[i] = t;
            }
        }
    }
}

// ---- the sums of the backward's small matrices, ONE function each for both forms of the kernel below (the same additions in the same order)
// acc0 + p[0] + p[stride] + ... (n terms, left to right); AHEAD terms are loaded before the first of them is added
template <int AHEAD>
__device__ __forceinline__ float pf_chain(const float* p, long stride, int n, float acc) {
    int k = 0;
    if (AHEAD > 1) {
        for (; k + AHEAD <= n; k += AHEAD) {
            float v[AHEAD];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) v[u] = __builtin_nontemporal_load(p + (long)(k + u) * stride);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) acc += v[u];
        }
    }
#pragma unroll 8
    for (; k < n; ++k) acc += __builtin_nontemporal_load(p + (long)k * stride);
    return acc;
}
// one stretch [j0, j1) of (g_weff Wr_a^T)[o, cc].  The roundings are spelled out, so that they do not depend on what the compiler makes of
// the loop around the call: they are those of the loop as it has always been compiled (unrolled by 8 behind a remainder loop) -- the first
// n mod 8 terms fused multiply-adds, the rest in groups of 8 separately rounded products added in order.
__device__ __forceinline__ float pf_dhw_stretch(const float* __restrict__ g_weff, const float* __restrict__ wa, long lda, int Cout, int o, int cc,
                                                int j0, int j1) {
    const float* __restrict__ gp = g_weff + (long)o * Cout;
    const float* __restrict__ wp = wa + cc * lda;
    float acc = 0.f;
    int j = j0;
    for (const int e = j0 + ((j1 > j0 ? j1 - j0 : 0) & 7); j < e; ++j) acc = __builtin_fmaf(gp[j], wp[j], acc);          // (a stretch past Cout is empty)
    for (; j < j1; j += 8) {
        float pr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pr[u] = __fmul_rn(gp[j + u], wp[j + u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __fadd_rn(acc, pr[u]);
    }
    return acc;
}
// (W^T g_weff)[cc, j]: a chain of fused multiply-adds over the output channels (one channel: the rounded product)
template <int OC>
__device__ __forceinline__ float pf_dwa_item(const float* __restrict__ hw, long ldh, const float* __restrict__ g_weff, int Cout, int cc, int j) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < OC; ++o) acc = __builtin_fmaf(hw[o * ldh + cc], g_weff[(long)o * Cout + j], acc);
    return acc;
}

// SPLIT (default): what does not depend on the partial rows -- dwa = W^T g_weff and the stretch sums of g_weff Wr_a^T -- is computed in
// slices by all workgroups ahead of the ticket (the stretch sums go to the workspace behind the partial rows); the last workgroup only
// adds the partial rows, 16 loads in flight, and joins the two terms of dhw.  false: all of it by the last workgroup, as before
// (gaot_debug_set_proj_fold_split).  The same sums in the same order either way.
template <int OC, bool SPLIT>
__global__ __launch_bounds__(256) void proj_fold_bwd_kernel(const float* __restrict__ g_weff, const float* __restrict__ g_rproj,
                                                            const float* __restrict__ hw, long ldh, const float* __restrict__ wa, long lda,
                                                            const float* __restrict__ rowb, long ldr, int Q, int C, int Cout,
                                                            float* __restrict__ drowb, float* __restrict__ dhw, long ld_dhw, float* __restrict__ dhb,
                                                            float* __restrict__ dwa, long ld_dwa, float* __restrict__ ws, int* __restrict__ ticket,
                                                            int lanes) {
    extern __shared__ __attribute__((aligned(16))) float red[];      // [rows_per_block][OC * C + OC], later the final sums [OC * C + OC]
    __shared__ int last_s;
    const int rpb = 256 / lanes, row = threadIdx.x / lanes, lr = threadIdx.x % lanes, c = lr * 4;
    const bool cok = c < C;
    const int W = OC * C + OC;
    f32x4 wq[OC], pw[OC];
    float ps[OC];
#pragma unroll
    for (int o = 0; o < OC; ++o) {
        wq[o] = cok ? *reinterpret_cast<const f32x4*>(hw + o * ldh + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        pw[o] = f32x4{0.f, 0.f, 0.f, 0.f};
        ps[o] = 0.f;
    }
    // four rows in flight per lane group (a workgroup of a large Q walks dozens of rows: one dependent load round each was 45 us at
    // 131 k rows); the running sums take the rows in the same order whatever the unrolling
    const int stride = gridDim.x * rpb;
    for (int r0 = blockIdx.x * rpb + row; r0 < Q && cok; r0 += 4 * stride) {
        f32x4 v[4]; float g[4][OC];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + u * stride;
            const bool ok = r < Q;
            v[u] = ok ? *reinterpret_cast<const f32x4*>(rowb + (long)r * ldr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < OC; ++o) g[u][o] = ok ? g_rproj[(long)r * OC + o] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + u * stride;
            if (r >= Q) break;
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < OC; ++o) {
                d += wq[o] * g[u][o];          // d rowb = g_rproj W
                pw[o] += v[u] * g[u][o];       // g_rproj^T rowb
                ps[o] += g[u][o];              // column sums of g_rproj (bias gradient)
            }
            if (drowb) *reinterpret_cast<f32x4*>(drowb + (long)r * C + c) = d;
        }
    }
    if (cok) {
#pragma unroll
        for (int o = 0; o < OC; ++o) *reinterpret_cast<f32x4*>(red + row * W + o * C + c) = pw[o];
        if (lr == 0) {
#pragma unroll
            for (int o = 0; o < OC; ++o) red[row * W + OC * C + o] = ps[o];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < W; i += 256) {
        float acc = 0.f;
        for (int rr = 0; rr < rpb; ++rr) acc += red[rr * W + i];
        ws[(long)blockIdx.x * W + i] = acc;
    }
    float* ws2 = ws + (long)gridDim.x * W;          // [stretch][OC * C]: the stretch sums of g_weff Wr_a^T (SPLIT)
    if (SPLIT) {
        if (dwa)
            for (int i = blockIdx.x * 256 + threadIdx.x; i < C * Cout; i += gridDim.x * 256) {
                const int cc = i / Cout, j = i % Cout;
                dwa[cc * ld_dwa + j] = pf_dwa_item<OC>(hw, ldh, g_weff, Cout, cc, j);
            }
        if (dhw) {
            const int items = OC * C, segs = items >= 256 ? 1 : 256 / items, per = (Cout + segs - 1) / segs;
            for (int q = blockIdx.x * 256 + threadIdx.x; q < items * segs; q += gridDim.x * 256) {
                const int i = q % items, sg = q / items;
                ws2[q] = pf_dhw_stretch(g_weff, wa, lda, Cout, i / C, i % C, sg * per, min(Cout, (sg + 1) * per));
            }
        }
    }
    // the last workgroup to get here adds the partial rows in workgroup order and finishes the small matrices
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (int)gridDim.x - 1;
        if (last) {
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        last_s = last;
    }
    __syncthreads();
    if (!last_s) return;
    // (sums cut into stretches over several threads and joined in stretch order, as the forward's: fixed order, short latency chains)
    const int nb = gridDim.x;
    __shared__ float part[256];
    {
        const int segs = W >= 256 ? 1 : 256 / W, cols = 256 / segs, per = (nb + segs - 1) / segs;
        for (int i0 = 0; i0 < W; i0 += cols) {
            const int i = i0 + (int)threadIdx.x % cols, sg = (int)threadIdx.x / cols;
            float acc = 0.f;
            if (i < W && sg < segs) acc = pf_chain<SPLIT ? 16 : 1>(ws + (long)(sg * per) * W + i, W, min(nb, (sg + 1) * per) - sg * per, 0.f);
            __syncthreads();
            part[threadIdx.x] = acc;
            __syncthreads();
            if (sg == 0 && i < W) {
                float t = part[threadIdx.x];
                for (int q = 1; q < segs; ++q) t += part[threadIdx.x + q * cols];
                red[i] = t;
            }
        }
    }
    __syncthreads();
    if (dhb && threadIdx.x < OC) dhb[threadIdx.x] = red[OC * C + threadIdx.x];
    if (SPLIT) {
        if (dhw) {
            const int items = OC * C, segs = items >= 256 ? 1 : 256 / items;
            for (int i = threadIdx.x; i < items; i += 256)          // (g_rproj^T rowb)[o, c], then the stretches of (g_weff Wr_a^T)[o, c] in their order
                dhw[(i / C) * ld_dhw + (i % C)] = pf_chain<4>(ws2 + i, items, segs, red[i]);
        }
        return;
    }
    if (dhw) {
        const int items = OC * C;
        const int segs = items >= 256 ? 1 : 256 / items, cols = 256 / segs, per = (Cout + segs - 1) / segs;
        for (int i0 = 0; i0 < items; i0 += cols) {
            const int i = i0 + (int)threadIdx.x % cols, sg = (int)threadIdx.x / cols;
            float acc = 0.f;
            if (i < items && sg < segs) acc = pf_dhw_stretch(g_weff, wa, lda, Cout, i / C, i % C, sg * per, min(Cout, (sg + 1) * per));      // g_weff Wr_a^T
            __syncthreads();
            part[threadIdx.x] = acc;
            __syncthreads();
            if (sg == 0 && i < items) {
                float t = red[i];                                 // (g_rproj^T rowb)[o, c]
                for (int q = 0; q < segs; ++q) t += part[threadIdx.x + q * cols];
                dhw[(i / C) * ld_dhw + (i % C)] = t;
            }
        }
    }
    if (dwa)
        for (int i = threadIdx.x; i < C * Cout; i += 256) {
            const int cc = i / Cout, j = i % Cout;
            dwa[cc * ld_dwa + j] = pf_dwa_item<OC>(hw, ldh, g_weff, Cout, cc, j);       // W^T g_weff
        }
}
}  // namespace gaot

// A/B switch (gaot_debug_set_proj_fold_split): 1 (default) = proj_fold_bwd_kernel<OC, true>, 0 = the earlier tail; the same bits either way
static int g_pf_split = 1;
extern "C" int gaot_debug_set_proj_fold_split(int on) { const int old = g_pf_split; g_pf_split = on ? 1 : 0; return old; }
static inline int pf_pow2_ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
static inline int pf_blocks(int Q, int rpb) { int nb = (Q + rpb - 1) / rpb; return nb > 256 ? 256 : (nb < 1 ? 1 : nb); }
extern "C" int32_t gaot_proj_fold_workspace(int32_t Q, int32_t C, int32_t out_channels) {
    const int lanes = pf_pow2_ceil(C / 4 > 0 ? C / 4 : 1), rpb = 256 / (lanes < 256 ? lanes : 256);
    const int items = out_channels * C;          // + the stretch sums of g_weff Wr_a^T (proj_fold_bwd_kernel, SPLIT)
    return pf_blocks(Q, rpb > 0 ? rpb : 1) * (out_channels * C + out_channels) + items * (items >= 256 ? 1 : 256 / (items > 0 ? items : 1));
}
static int pf_check(const char* who, int32_t Q, int32_t C, int32_t Cout, int32_t OC, const float* hw, int64_t ldh, const float* wa, const float* rowb, int64_t ldr) {
    GAOT_REQUIRE(Q > 0 && C > 0 && C % 4 == 0 && C <= 256 && Cout > 0 && Cout <= 1024 && OC >= 1 && OC <= 4, "%s: need Q > 0, C %% 4 == 0, C <= 256, 1 <= out_channels <= 4", who);
    GAOT_REQUIRE(hw && wa && rowb && aligned16(hw) && aligned16(rowb) && ldh % 4 == 0 && ldr % 4 == 0, "%s: null or misaligned operand (hw, rowb: 16 bytes, leading dims %% 4)", who);
    return GAOT_OK;
}

extern "C" int gaot_proj_fold_fwd(const float* hw, int64_t ldh, const float* hb, const float* wa, int64_t lda, const float* rowb, int64_t ldr,
                                  int32_t Q, int32_t C, int32_t Cout, int32_t out_channels, float* weff, float* rproj, gaot_stream_t stream) {
    if (int rc = pf_check("proj_fold_fwd", Q, C, Cout, out_channels, hw, ldh, wa, rowb, ldr)) return rc;
    GAOT_REQUIRE(weff && rproj, "proj_fold_fwd: null output");
    const int lanes = pf_pow2_ceil(C / 4), rpb = 256 / lanes;
    int nb = (Q + rpb - 1) / rpb; if (nb > 2048) nb = 2048;
#define PF(OC) hipLaunchKernelGGL((gaot::proj_fold_fwd_kernel<OC>), dim3(nb), dim3(256), 0, ST(stream), hw, (long)ldh, hb, wa, (long)lda, rowb, (long)ldr, Q, C, Cout, weff, rproj, lanes)
    if (out_channels == 1) PF(1); else if (out_channels == 2) PF(2); else if (out_channels == 3) PF(3); else PF(4);
#undef PF
    GAOT_CHECK_LAUNCH("gaot_proj_fold_fwd");
    return GAOT_OK;
}

extern "C" int gaot_proj_fold_bwd(const float* g_weff, const float* g_rproj, const float* hw, int64_t ldh, const float* wa, int64_t lda,
                                  const float* rowb, int64_t ldr, int32_t Q, int32_t C, int32_t Cout, int32_t out_channels, float* drowb,
                                  float* dhw, int64_t ld_dhw, float* dhb, float* dwa, int64_t ld_dwa, float* workspace, int32_t* ticket,
                                  gaot_stream_t stream) {
    if (int rc = pf_check("proj_fold_bwd", Q, C, Cout, out_channels, hw, ldh, wa, rowb, ldr)) return rc;
    GAOT_REQUIRE(g_weff && g_rproj && workspace && ticket && (!drowb || aligned16(drowb)), "proj_fold_bwd: null gradient / workspace / ticket or misaligned drowb");
    const int lanes = pf_pow2_ceil(C / 4), rpb = 256 / lanes;
    const int nb = pf_blocks(Q, rpb);
    const size_t lds = sizeof(float) * (size_t)rpb * (out_channels * C + out_channels);
    GAOT_REQUIRE(lds <= 60 * 1024, "proj_fold_bwd: C = %d too wide for the workgroup reduction", C);
#define PF(OC) do { if (g_pf_split) hipLaunchKernelGGL((gaot::proj_fold_bwd_kernel<OC, true>), dim3(nb), dim3(256), lds, ST(stream), g_weff, g_rproj, hw, (long)ldh, wa, (long)lda, \
                                                     rowb, (long)ldr, Q, C, Cout, drowb, dhw, (long)ld_dhw, dhb, dwa, (long)ld_dwa, workspace, ticket, lanes); \
                    else hipLaunchKernelGGL((gaot::proj_fold_bwd_kernel<OC, false>), dim3(nb), dim3(256), lds, ST(stream), g_weff, g_rproj, hw, (long)ldh, wa, (long)lda, \
                                            rowb, (long)ldr, Q, C, Cout, drowb, dhw, (long)ld_dhw, dhb, dwa, (long)ld_dwa, workspace, ticket, lanes); } while (0)
    if (out_channels == 1) PF(1); else if (out_channels == 2) PF(2); else if (out_channels == 3) PF(3); else PF(4);
#undef PF
    GAOT_CHECK_LAUNCH("gaot_proj_fold_bwd");
    return GAOT_OK;
}

extern "C" int gaot_rollout_input(const float* state, int32_t U, const float* stat, int32_t S, float t0n, float dtn, int32_t n_time,
                                  int64_t rows, float* pn, gaot_stream_t stream) {
    GAOT_REQUIRE(state && pn && U > 0 && S >= 0 && (S == 0 || stat) && (n_time == 1 || n_time == 2) && rows > 0, "rollout_input: bad arguments");
    hipLaunchKernelGGL(gaot::rollout_input_kernel, dim3(cap_blocks(rows * (U + S + n_time), 256, 4096)), dim3(256), 0, ST(stream), state, U, stat, S,
                       t0n, dtn, n_time, (long)rows, pn);
    GAOT_CHECK_LAUNCH("gaot_rollout_input");
    return GAOT_OK;
}

extern "C" int gaot_rollout_update(const float* pred, float* state, int32_t U, const float* u_mean, const float* u_std, const float* a_mean,
                                   const float* a_std, float dt, int32_t mode, int64_t rows, float* den_out, gaot_stream_t stream) {
    GAOT_REQUIRE(pred && state && u_mean && u_std && den_out && U > 0 && rows > 0 && mode >= 0 && mode <= 2 && (mode == 0 || (a_mean && a_std)),
                 "rollout_update: bad arguments (mode 0 output, 1 residual, 2 time_der)");
    hipLaunchKernelGGL(gaot::rollout_update_kernel, dim3(cap_blocks(rows * U, 256, 4096)), dim3(256), 0, ST(stream), pred, state, U, u_mean, u_std,
                       a_mean, a_std, dt, mode, (long)rows, den_out);
    GAOT_CHECK_LAUNCH("gaot_rollout_update");
    return GAOT_OK;
}
