// Shared by the attention translation units (attention.hip, attention_wide.hip): the kernel argument block and the small
// device helpers every attention kernel uses, so both files see one definition.
#pragma once
#include "common.h"

namespace gaot {

constexpr float LOG2E = 1.4426950408889634f;

struct AttnArgs {
    const float *q, *k, *v;
    long ldq, ldk, ldv;
    int B, S, H, Hkv, D;
    float* o; long ldo; float* lse;
    // backward
    const float *oin, *dout; float *dq, *dk, *dv; long lddq, lddk, lddv;
    float* delta; float* dq_part; int n_kblocks;
    float *dk2, *dv2;          // query-split backward (QS = 2): dense [B S][H 32] partials of the second half of the query tiles
    float *o_part, *lse_part;  // key-split forward (KS = 2): per half the normalised output [B S][H D] (dense) and its log-sum-exp [B H S]
    float scale; int vec;
    // attention dropout (attn.py:110-114, dropout_p of F.scaled_dot_product_attention in training): P is multiplied by
    // keep(b, h, q, k) / (1 - p) after the softmax; the mask is a counter-based hash of (*drop_seed, element index), so the
    // backward regenerates it from the same seed word
    const unsigned long long* drop_seed; unsigned drop_thresh; float drop_scale;
    // fp16-piece kernels (pieces = 4): magnitude words of the q | k | v operands (one word: they are one tensor) and of dO
    const float* qkv_amax; const float* dout_amax;
    float* dqkv_amax;          // optional: published magnitude word of dq | dk | dv
};

// splitmix64 finaliser of (seed + linear index of the score): the top 32 bits against the keep threshold
__device__ __forceinline__ float attn_drop_factor(unsigned long long seed, long idx, unsigned thresh, float scale) {
    unsigned long long x = seed + (unsigned long long)idx;
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return (unsigned)(x >> 32) < thresh ? scale : 0.f;
}

// id -> (group, member): groups are dealt to XCDs round-robin, all members of a group stay on the group's XCD.
// With G groups of n members: XCD x = id % 8 serves groups x, x+8, ...; falls back to the plain order when G % 8 != 0.
__device__ __forceinline__ void xcd_group_decode(int id, int G, int n, int& group, int& member) {
    if ((G & 7) == 0) {
        const int x = id & 7, t = id >> 3;        // t-th workgroup on XCD x
        group = x + 8 * (t / n);
        member = t % n;
    } else {
        group = id / n;
        member = id % n;
    }
}

__device__ __forceinline__ f32x4 load4(const float* __restrict__ row, int d, int D, bool row_ok, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok) return v;
    if (vec) { if (d < D) v = *reinterpret_cast<const f32x4*>(row + d); }
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (d + j < D) v[j] = row[d + j];
    }
    return v;
}

// ---- 128 < head_dim <= 256 (attention_wide.hip): the head dimension is split over the four waves of a workgroup.
// Launchers only: no allocation, no synchronisation.  `a` is filled as for the narrower kernels; the backward expects a.delta filled
// (attn_delta_*) and runs two passes, dK / dV per key block and dQ per query block, so it writes no dQ partials (a.dq_part unused).
constexpr int WIDE_DP = 256;     // padded head_dim of the wide kernels
constexpr int WIDE_KB = 32;      // keys per workgroup of the wide backward's dK / dV pass
void attn_wide_fwd_launch(const AttnArgs& a, bool dropout, hipStream_t stream);
void attn_wide_bwd_launch(const AttnArgs& a, bool dropout, hipStream_t stream);

}  // namespace gaot
