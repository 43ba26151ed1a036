// Softmax attention (no mask) forward + backward in exact fp32 on the gfx950 matrix cores.
// Replaces F.scaled_dot_product_attention at attn.py:114 and its autograd.
//
// f32-input MFMA (v_mfma_f32_32x32x2_f32) takes ONE value per lane per operand and its C/D fragment
// puts column (lane&31) in the lane and 16 rows crow(r, lane>>5) in registers.  That makes the flash
// pipeline register-resident with no shuffles:
//   forward : S^T = K Q^T  -> each lane owns one query column, softmax row-max/sum are in-register
//             (+1 cross-half exchange); the SAME registers are the B operand of O^T += V^T P^T.
//   backward: S = Q K^T and dP = dO V^T have one key column per lane; P and dS feed dV^T += dO^T P and
//             dK^T += Q^T dS straight from registers; only dQ = dS K needs dS transposed (through LDS).
// Reduction order inside a tile is free, so k-slots are chosen to make every LDS read conflict-free
// (ds_read_b128 on +4-padded rows for A operands, row-contiguous ds_read_b32 otherwise).
// Everything is deterministic: no atomics; dQ partials per key block are reduced in a fixed order.
#include "attention_common.h"
#include "attention_plan.h"

namespace gaot {

// ---------------------------------------------------------------------------------------------
// forward: workgroup = 4 waves x 32 queries; key/value tiles of 64 rows staged through LDS
// ---------------------------------------------------------------------------------------------
template <int DP, bool DROP = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnArgs p) {
    constexpr int ND = DP / 32;          // 32-wide d tiles
    constexpr int LDT = DP + 4;          // LDS row stride (floats)
    constexpr int KT = 64;               // keys per staged tile
    constexpr int NF4 = KT * DP / 4 / 256;   // float4 per thread per operand tile
    __shared__ __attribute__((aligned(16))) float smem[2 * KT * LDT];
    float* Ks = smem;
    float* Vs = smem + KT * LDT;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    // XCD-aware decode of the 1-D grid: the dispatcher places workgroup id on XCD id % 8; keep all query blocks of one
    // (batch, head) on ONE XCD so its K/V (2 x S x D x 4 B) is fetched into that XCD's L2 once, not eight times.
    int bh, blk;
    xcd_group_decode(blockIdx.x, p.B * p.H, (p.S + 127) / 128, bh, blk);
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int q0 = blk * 128 + wave * 32;
    const int D = p.D;
    const bool vec = p.vec != 0;
    const float c = p.scale * LOG2E;

    // Q^T operand: lane (q = li, half lh) keeps Q[q][8g + 4lh + s]
    float qreg[DP / 2];
    {
        const int qi = q0 + li;
        const float* qrow = p.q + ((long)b * p.S + qi) * p.ldq + (long)h * D;
#pragma unroll
        for (int g = 0; g < DP / 8; ++g) {
            const f32x4 v = load4(qrow, 8 * g + 4 * lh, D, qi < p.S, vec);
            qreg[4 * g + 0] = v[0]; qreg[4 * g + 1] = v[1]; qreg[4 * g + 2] = v[2]; qreg[4 * g + 3] = v[3];
        }
    }
    f32x16 oacc[ND];
#pragma unroll
    for (int t = 0; t < ND; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const float* kbase = p.k + (long)b * p.S * p.ldk + (long)hk * D;
    const float* vbase = p.v + (long)b * p.S * p.ldv + (long)hk * D;
    f32x4 rk[NF4], rv[NF4];
    auto fetch = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            const int row = t / (DP / 4), d = (t % (DP / 4)) * 4;
            const bool ok = kv0 + row < p.S;
            rk[i] = load4(kbase + (long)(kv0 + row) * p.ldk, d, D, ok, vec);
            rv[i] = load4(vbase + (long)(kv0 + row) * p.ldv, d, D, ok, vec);
        }
    };
    const int ntiles = (p.S + KT - 1) / KT;
    fetch(0);
    for (int kt = 0; kt < ntiles; ++kt) {
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            const int row = t / (DP / 4), d = (t % (DP / 4)) * 4;
            *reinterpret_cast<f32x4*>(Ks + row * LDT + d) = rk[i];
            *reinterpret_cast<f32x4*>(Vs + row * LDT + d) = rv[i];
        }
        __syncthreads();
        if (kt + 1 < ntiles) fetch((kt + 1) * KT);
#pragma unroll
        for (int sub = 0; sub < KT / 32; ++sub) {
            const int kvs = kt * KT + sub * 32;   // first key of this 32-row sub-tile
            if (kvs >= p.S) break;
            // ---- S^T[kv][q] = sum_d K[kv][d] Q[q][d]
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
            const float* krow = Ks + (sub * 32 + li) * LDT + 4 * lh;
#pragma unroll
            for (int g = 0; g < DP / 8; ++g) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(krow + 8 * g);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[t], qreg[4 * g + t], s, 0, 0, 0);
            }
            // ---- online softmax over the key rows this lane holds (16) + the other half-wave (16)
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kvs + crow(r, lh) >= p.S) s[r] = -INFINITY;
                mx = fmaxf(mx, s[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = exp2f((m_run - m_new) * c);
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = exp2f((s[r] - m_new) * c); ps += s[r]; }
            ps += __shfl_xor(ps, 32, 64);
            l_run = l_run * alpha + ps;
            m_run = m_new;
#pragma unroll
            for (int t = 0; t < ND; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
            if (DROP) {      // the row sum above is of the undropped probabilities (softmax first, dropout on its output)
                const unsigned long long seed = *p.drop_seed;
                const long base = (((long)b * p.H + h) * p.S + (q0 + li)) * p.S + kvs;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] *= attn_drop_factor(seed, base + crow(r, lh), p.drop_thresh, p.drop_scale);
            }
            // ---- O^T[d][q] += sum_kv V[kv][d] P^T[kv][q]   (P^T registers are the B operand as they are)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* vrow = Vs + (sub * 32 + crow(r, lh)) * LDT + li;
#pragma unroll
                for (int t = 0; t < ND; ++t)
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * t], s[r], oacc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ---- epilogue: normalise, transpose O^T through LDS (wave-private 32 x (DP+1)), coalesced row stores
    const float inv_l = 1.0f / l_run;
    float* Os = smem + wave * 32 * (DP + 1);     // 4 * 32 * (DP+1) floats <= 2*64*(DP+4)
#pragma unroll
    for (int t = 0; t < ND; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Os[li * (DP + 1) + 32 * t + crow(r, lh)] = oacc[t][r] * inv_l;
    __syncthreads();
    for (int rr = lh; rr < 32; rr += 2) {
        const int qi = q0 + rr;
        if (qi >= p.S) break;
        float* orow = p.o + ((long)b * p.S + qi) * p.ldo + (long)h * D;
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            const int d = 32 * t + li;
            if (d < D) orow[d] = Os[rr * (DP + 1) + d];
        }
    }
    if (lh == 0 && q0 + li < p.S)
        p.lse[((long)b * p.H + h) * p.S + q0 + li] = m_run * p.scale + logf(l_run);
}

// ---------------------------------------------------------------------------------------------
// forward, LDS-direct variant for head_dim == 32 with 16-byte aligned q/k/v: K and V tiles (64 keys) go HBM/L2 -> LDS
// with global_load_lds through a 3-stage ring (one raw s_barrier per tile, counted vmcnt); K is stored [key][32] with
// its 16-byte chunks XOR-swizzled by ((key >> 1) & 7) (source-side swizzle, conflict-free ds_read_b128 A operand),
// V is stored as it comes (row-contiguous ds_read_b32).  The online softmax runs once per 64 keys.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_fwd_glds_kernel(const AttnArgs p) {
    constexpr int KT = 64, NS = 3;
    constexpr int ST = 2 * KT * 32;                    // floats per stage (K + V)
    __shared__ __attribute__((aligned(16))) float smem[NS * ST];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, blk;
    xcd_group_decode(blockIdx.x, p.B * p.H, (p.S + 127) / 128, bh, blk);
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int q0 = blk * 128 + wave * 32;
    const float c = p.scale * LOG2E;

    float qreg[16];
    {
        const int qi = q0 + li;
        const float* qrow = p.q + ((long)b * p.S + qi) * p.ldq + (long)h * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = load4(qrow, 8 * g + 4 * lh, 32, qi < p.S, true);
            qreg[4 * g + 0] = v[0]; qreg[4 * g + 1] = v[1]; qreg[4 * g + 2] = v[2]; qreg[4 * g + 3] = v[3];
        }
    }
    // this wave's DMA pieces: chunks t = (q*4 + wave)*64 + lane, q = 0,1 for K and for V; row = t >> 3, chunk = t & 7
    const float* kbase = p.k + (long)b * p.S * p.ldk + (long)hk * 32;
    const float* vbase = p.v + (long)b * p.S * p.ldv + (long)hk * 32;
    int prow[2], kch[2], vch[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int t = (q * 4 + wave) * 64 + lane;
        prow[q] = t >> 3;
        vch[q] = t & 7;
        kch[q] = (t & 7) ^ ((prow[q] >> 1) & 7);
    }
    auto issue = [&](int kt, int stage) {
        float* Ks = smem + stage * ST;
        float* Vs = Ks + KT * 32;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int row = min(kt * KT + prow[q], p.S - 1);       // clamp: padded keys are masked to -inf below
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kbase + (long)row * p.ldk + kch[q] * 4),
                                             (__attribute__((address_space(3))) void*)(Ks + (q * 4 + wave) * 256), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vbase + (long)row * p.ldv + vch[q] * 4),
                                             (__attribute__((address_space(3))) void*)(Vs + (q * 4 + wave) * 256), 16, 0, 0);
        }
    };

    f32x16 oacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (p.S + KT - 1) / KT;
    const int ksw = (li >> 1) & 7;                    // swizzle of this lane's key row (li and li+32 share it)
    issue(0, 0);
    if (ntiles > 1) issue(1, 1);
    int stage = 0;
    for (int kt = 0; kt < ntiles; ++kt) {
        if (kt + 1 < ntiles) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else                 asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kt + 2 < ntiles) issue(kt + 2, stage >= 1 ? stage - 1 : 2);
        const float* Ks = smem + stage * ST;
        const float* Vs = Ks + KT * 32;
        // ---- S^T for 64 keys: two 32-key fragments
        f32x16 s0, s1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = ((2 * g + lh) ^ ksw) << 2;
            const f32x4 k0 = *reinterpret_cast<const f32x4*>(Ks + li * 32 + ch);
            const f32x4 k1 = *reinterpret_cast<const f32x4*>(Ks + (32 + li) * 32 + ch);      // (32+li)>>1 &7 == ksw
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[t], qreg[4 * g + t], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[t], qreg[4 * g + t], s1, 0, 0, 0);
            }
        }
        // ---- online softmax over the 64 keys.  VALU budget matters here (PMC: 10 VALU per MFMA kept the matrix pipe at
        // 57 %): padded keys are masked only on the last tile, exp is the raw v_exp_f32 on fma(s, c, -m*c), and the
        // O rescale is skipped (exactly) whenever no lane's running max moved.
        const int kv0 = kt * KT;
        if (__builtin_amdgcn_readfirstlane(kv0 + KT > p.S)) {      // scalar branch; the asm keeps it from being if-converted
            asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kv0 + crow(r, lh) >= p.S) s0[r] = -INFINITY;
                if (kv0 + 32 + crow(r, lh) >= p.S) s1[r] = -INFINITY;
            }
        }
        float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(s0[r], s1[r]));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float mc = -m_new * c;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s0[r] = __builtin_amdgcn_exp2f(fmaf(s0[r], c, mc));
            s1[r] = __builtin_amdgcn_exp2f(fmaf(s1[r], c, mc));
            ps += s0[r] + s1[r];
        }
        ps += __shfl_xor(ps, 32, 64);
        if (__any(m_new != m_run)) {                   // wave-uniform branch; alpha == 1 exactly when the max is unchanged
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[r] *= alpha;
            m_run = m_new;
        }
        l_run += ps;
        // ---- O^T += V^T P^T
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = crow(r, lh);
            oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[row * 32 + li], s0[r], oacc, 0, 0, 0);
            oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(32 + row) * 32 + li], s1[r], oacc, 0, 0, 0);
        }
        stage = stage == 2 ? 0 : stage + 1;
    }
    __syncthreads();
    const float inv_l = 1.0f / l_run;
    float* Os = smem + wave * 32 * 33;
#pragma unroll
    for (int r = 0; r < 16; ++r) Os[li * 33 + crow(r, lh)] = oacc[r] * inv_l;
    __syncthreads();
    for (int rr = lh; rr < 32; rr += 2) {
        const int qi = q0 + rr;
        if (qi >= p.S) break;
        p.o[((long)b * p.S + qi) * p.ldo + (long)h * 32 + li] = Os[rr * 33 + li];
    }
    if (lh == 0 && q0 + li < p.S)
        p.lse[((long)b * p.H + h) * p.S + q0 + li] = m_run * p.scale + logf(l_run);
}


// ---------------------------------------------------------------------------------------------
// forward on the bf16 matrix pipe, fp32-exact (head_dim == 32, 16-byte aligned q/k/v): every fp32 operand is split exactly
// into three bf16 pieces (common.h split3_pair) and each product is accumulated in fp32 from the six piece products of weight
// >= 2^-16, exactly as in gemm_split.hip: 2.67x the fp32-MFMA rate for the two products of the kernel.
//   S^T = K Q^T : A = K planes from LDS ([key][32 d] bf16, row stride 80 B, one ds_read_b128 per plane and 16-wide d step),
//                 B = the wave's Q rows, split once into registers.
//   O^T += V^T P^T : B = P, split in registers right after the softmax (the k-slot of half-wave hi in step u is key
//                 crow(8u + e, hi), i.e. keys 16u + 4hi + {0..3, 8..11} of the 32-key tile: the lane's own result registers),
//                 A = V^T planes from LDS ([d][64 keys] bf16, row stride 136 B: two conflict-free ds_read_b64 per plane / step).
// K / V tiles (64 keys) are split by all 256 threads on the way from the prefetch registers into one of two LDS stages.
// ---------------------------------------------------------------------------------------------
// pieces of an operand pair: OP = 3 exact (split3_pair), OP = 2 two rounded pieces (split2_pair; third piece zero, never stored or multiplied)
// F16: two fp16 pieces of sc * x (common.h split2h_pair: x carried up to its last bit once sc puts the operand's largest magnitude at ~2^14)
template <int OP, bool F16 = false>
__device__ __forceinline__ void split_op(float x0, float x1, unsigned& a, unsigned& b, unsigned& c, float sc = 1.f) {
    if (F16) { split2h_pair_gemm(x0, x1, sc, a, b); c = 0u; }
    else if (OP == 3) split3_pair(x0, x1, a, b, c);
    else { split2_pair(x0, x1, a, b); c = 0u; }
}
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
    if (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// power-of-two scale (and inverse) that puts a wave-uniform magnitude at ~2^14: the per-tile scale of dS in the fp16-piece backward
__device__ __forceinline__ void pow2_scale(float amax, float& sc, float& inv) {
    int se = 140 - (int)((__float_as_uint(amax) >> 23) & 0xffu);
    se = se > 126 ? 126 : (se < -126 ? -126 : se);
    sc = __uint_as_float((unsigned)(127 + se) << 23);
    inv = __uint_as_float((unsigned)(127 - se) << 23);
}
// probabilities live in [0, 1]: static scale 2^13 -- not 2^15: with scores of ~1e7 (fp32 ulp ~1 in the exponent) a recomputed
// exp2(s c - lse) comes out as 2 or 4 instead of <= 1, and 4 x 2^15 is past fp16's 65 504 (inf -> NaN where the three-piece kernels
// merely return the same garbage the reference does); every P >= 2^-15 keeps full precision, smaller ones an absolute 2^-38
constexpr float P_SCALE = 8192.f, P_INV = 1.f / 8192.f;
constexpr int AS_KROW = 80, AS_VROW = 136;
constexpr int AS_KPL = 64 * AS_KROW, AS_VPL = 32 * AS_VROW;
constexpr int AS_STAGE = 3 * AS_KPL + 3 * AS_VPL;          // bytes

// NW = 4 (128 queries per workgroup, two workgroups per CU) or 8 (256 queries, one workgroup per CU: every K / V tile is split
// half as often per head and each thread stages half as much).
// DH = 32, or 64 for 32 < head_dim <= 64 (p.D % 4 == 0; columns past head_dim are zero-filled on the way in and never stored):
// four 16-wide d steps per score, two 32-row tiles of O^T; one workgroup per CU either way (108 KB of LDS).
// PP = pieces of P in the P V product: 3 = exact split; 2 = two pieces (common.h split2_pair: the second one rounded to nearest),
// five piece products instead of six -- P is a softmax output in [0, 1] carrying ~1e-7 of relative noise from exp2 alone, the
// dropped part is <= 2^-17 of each probability and unbiased
// F16 (with PP = OP = 2): two fp16 pieces of the scaled operands (Q, K, V by the power of two from their magnitude word, P by 2^15), three
// piece products per k-step on the f16 MFMA: fp32-level products at the two-piece kernels' cost.
// KS = 2 [r6]: the KEYS of a query block are shared between two workgroups (first half / second half of the key tiles): shapes whose
// 256-query blocks x batch x heads number 128 .. 255 (the 3-D configuration's 1 x 4 096 tokens x 8 heads of 48) fill the chip with
// eight waves per CU.  Each half leaves its own normalised output and log-sum-exp in the workspace; attn_fwd_combine_kernel joins them
// (o = w1 o1 + w2 o2, w_i = exp(lse_i - lse): the same softmax, two partial sums per row instead of one running sum).
template <int NW, int DH = 32, int PP = 3, int OP = 3, bool F16 = false, int KS = 1>
__global__ __launch_bounds__(64 * NW, (NW == 4 && DH == 32) ? 2 : 1) void attn_fwd_split_kernel(const AttnArgs p) {
    constexpr int KT = 64, NT = 64 * NW, QB = 32 * NW;
    constexpr int NU = DH / 16, NDT = DH / 32, CPR = DH / 4;            // d steps, O tiles, 4-float chunks per row
    constexpr int KROW = DH * 2 + 16, KPL = 64 * KROW, VPL = DH * AS_VROW, STAGE = 3 * KPL + 3 * VPL;
    static_assert(DH != 32 || (KROW == AS_KROW && KPL == AS_KPL && VPL == AS_VPL && STAGE == AS_STAGE), "head_dim 32 layout");
    constexpr int EPI = NW * 32 * (DH + 1) * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE > EPI ? 2 * STAGE : EPI];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, blk, khalf = 0;
    xcd_group_decode(blockIdx.x, p.B * p.H, ((p.S + QB - 1) / QB) * KS, bh, blk);
    if (KS > 1) { khalf = blk % KS; blk /= KS; }
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int q0 = blk * QB + wave * 32;
    const int D = DH == 32 ? 32 : p.D;
    static_assert(!F16 || (PP == 2 && OP == 2), "fp16 pieces come in twos");
    // Q fragments: lane (q = li, hi) holds d = 16u + 8hi + e (e = 0..7) for every d step u, as three packed bf16 planes.  The rows are
    // requested BEFORE the magnitude word is read: one round trip instead of two at the head of the workgroup's life.
    bf16x8 qf[3][NU];
    f32x4 qraw[NU][2];
    {
        const int qi = q0 + li;
        const float* qrow = p.q + ((long)b * p.S + qi) * p.ldq + (long)h * D;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            qraw[u][0] = load4(qrow, 16 * u + 8 * lh, D, qi < p.S, true);
            qraw[u][1] = load4(qrow, 16 * u + 8 * lh + 4, D, qi < p.S, true);
        }
    }
    float sc_in = 1.f, so_in = 1.f;
    if (F16) amax_scale(p.qkv_amax, sc_in, so_in);
    const float sm_scale = p.scale * so_in * so_in;          // scores arrive scaled by sc_in^2
    const float c = sm_scale * LOG2E;
    const float o_inv = F16 ? so_in * P_INV : 1.f;             // the tile's V^T P^T arrives scaled by sc_in * 2^15
    {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const f32x4 v0 = qraw[u][0];
            const f32x4 v1 = qraw[u][1];
            u32x4 ph, pm, pl;
            unsigned a_, b_, c_;
            split_op<OP, F16>(v0[0], v0[1], a_, b_, c_, sc_in); ph[0] = a_; pm[0] = b_; pl[0] = c_;
            split_op<OP, F16>(v0[2], v0[3], a_, b_, c_, sc_in); ph[1] = a_; pm[1] = b_; pl[1] = c_;
            split_op<OP, F16>(v1[0], v1[1], a_, b_, c_, sc_in); ph[2] = a_; pm[2] = b_; pl[2] = c_;
            split_op<OP, F16>(v1[2], v1[3], a_, b_, c_, sc_in); ph[3] = a_; pm[3] = b_; pl[3] = c_;
            qf[0][u] = __builtin_bit_cast(bf16x8, ph); qf[1][u] = __builtin_bit_cast(bf16x8, pm); qf[2][u] = __builtin_bit_cast(bf16x8, pl);
        }
    }
    // staging: K float4 items (key = idx / CPR, chunk = idx % CPR), NKF per thread; V: key PAIR items (kp = idx / CPR, chunk), two
    // float4 each, for the first 32 * CPR threads
    const float* kbase = p.k + (long)b * p.S * p.ldk + (long)hk * D;
    const float* vbase = p.v + (long)b * p.S * p.ldv + (long)hk * D;
    constexpr int NKF = 64 * CPR / NT;            // K float4 per thread per tile
    constexpr int NVI = (32 * CPR + NT - 1) / NT;      // V key-pair items per thread (1; 2 for the 4-wave head_dim-64 form)
    static_assert(NKF >= 1, "staging roles");
    f32x4 rk[NKF], rv[NVI][2];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NKF; ++i) {
            const int idx = tid + i * NT;
            const int krow = min(kt * KT + idx / CPR, p.S - 1);
            rk[i] = load4(kbase + (long)krow * p.ldk, (idx % CPR) * 4, D, true, true);
        }
#pragma unroll
        for (int j = 0; j < NVI; ++j) {
            const int idx = tid + j * NT;
            if (idx < 32 * CPR) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int vrow = min(kt * KT + 2 * (idx / CPR) + i, p.S - 1);
                    rv[j][i] = load4(vbase + (long)vrow * p.ldv, (idx % CPR) * 4, D, true, true);
                }
            }
        }
    };
    auto stage = [&](int stg) {
        unsigned char* Kp = smem + stg * STAGE;
        unsigned char* Vp = Kp + 3 * KPL;
#pragma unroll
        for (int i = 0; i < NKF; ++i) {
            const int idx = tid + i * NT;
            u32x2 h, m, l;
            unsigned a_, b_, c_;
            split_op<OP, F16>(rk[i][0], rk[i][1], a_, b_, c_, sc_in); h[0] = a_; m[0] = b_; l[0] = c_;
            split_op<OP, F16>(rk[i][2], rk[i][3], a_, b_, c_, sc_in); h[1] = a_; m[1] = b_; l[1] = c_;
            unsigned char* dst = Kp + (idx / CPR) * KROW + (idx % CPR) * 8;
            *reinterpret_cast<u32x2*>(dst) = h;
            *reinterpret_cast<u32x2*>(dst + KPL) = m;
            if (OP == 3) *reinterpret_cast<u32x2*>(dst + 2 * KPL) = l;
        }
        // V^T: (key 2kp, key 2kp+1) pairs of the thread's 4 d columns -> one dword per d row and plane
#pragma unroll
        for (int j = 0; j < NVI; ++j) {
            const int idx = tid + j * NT;
            if (idx < 32 * CPR) {
                const int kp = idx / CPR, d0 = (idx % CPR) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned a_, b_, c_;
                    split_op<OP, F16>(rv[j][0][e], rv[j][1][e], a_, b_, c_, sc_in);
                    unsigned char* dst = Vp + (d0 + e) * AS_VROW + kp * 4;
                    *reinterpret_cast<unsigned*>(dst) = a_;
                    *reinterpret_cast<unsigned*>(dst + VPL) = b_;
                    if (OP == 3) *reinterpret_cast<unsigned*>(dst + 2 * VPL) = c_;
                }
            }
        }
    };

    f32x16 oacc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles_all = (p.S + KT - 1) / KT;
    const int kt_per = (ntiles_all + KS - 1) / KS;
    const int kt_begin = khalf * kt_per, ntiles = min(ntiles_all, kt_begin + kt_per);          // this workgroup's key tiles: kt_begin .. ntiles - 1
    fetch(kt_begin);
    stage(0);
    if (kt_begin + 1 < ntiles) fetch(kt_begin + 1);
    __syncthreads();
    for (int kt = kt_begin; kt < ntiles; ++kt) {
        const int stg = (kt - kt_begin) & 1;
        const unsigned char* Kp = smem + stg * STAGE;
        const unsigned char* Vp = Kp + 3 * KPL;
        // ---- S^T for 64 keys: two 32-key fragments, d in 16-wide steps, six piece products each
        f32x16 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const unsigned char* kr = Kp + (32 * t + li) * KROW + u * 32 + lh * 16;
                const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(kr);
                const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(kr + KPL);
                if (OP == 3) {
                    const bf16x8 k2 = *reinterpret_cast<const bf16x8*>(kr + 2 * KPL);
                    s[t] = mfma16<F16>(k2, qf[0][u], s[t]);
                    s[t] = mfma16<F16>(k0, qf[2][u], s[t]);
                    s[t] = mfma16<F16>(k1, qf[1][u], s[t]);
                }
                s[t] = mfma16<F16>(k1, qf[0][u], s[t]);
                s[t] = mfma16<F16>(k0, qf[1][u], s[t]);
                s[t] = mfma16<F16>(k0, qf[0][u], s[t]);
            }
        }
        // ---- online softmax over the 64 keys (fp32)
        const int kv0 = kt * KT;
        if (__builtin_amdgcn_readfirstlane(kv0 + KT > p.S)) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kv0 + crow(r, lh) >= p.S) s[0][r] = -INFINITY;
                if (kv0 + 32 + crow(r, lh) >= p.S) s[1][r] = -INFINITY;
            }
        }
        float mx = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(s[0][r], s[1][r]));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float mc = -m_new * c;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[0][r] = __builtin_amdgcn_exp2f(fmaf(s[0][r], c, mc));
            s[1][r] = __builtin_amdgcn_exp2f(fmaf(s[1][r], c, mc));
            ps += s[0][r] + s[1][r];
        }
        ps += __shfl_xor(ps, 32, 64);
        if (__any(m_new != m_run)) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
            m_run = m_new;
        }
        l_run += ps;
        // the tile's product is accumulated from ZERO on the matrix pipe and added to O on the vector pipe: the bf16 MFMA does
        // not round its accumulator to nearest, and thousands of same-signed increments into one growing accumulator (many equal
        // tokens: P nearly uniform, V rows alike) drift by 1e-5 relative (measured on the C5 shape: 4 096 keys, 92 % equal rows)
        f32x16 ot[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dt][r] = 0.f;
        // ---- O^T += V^T P^T: P split in registers; step u of tile t covers the lane's registers r = 8u .. 8u+7
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                u32x4 ph, pm, pl = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned a_, b_, c_ = 0u;
                    if (PP == 3) split3_pair(s[t][8 * u + 2 * e], s[t][8 * u + 2 * e + 1], a_, b_, c_);
                    else if (F16) split2h_pair_gemm(s[t][8 * u + 2 * e], s[t][8 * u + 2 * e + 1], P_SCALE, a_, b_);
                    else split2_pair(s[t][8 * u + 2 * e], s[t][8 * u + 2 * e + 1], a_, b_);
                    ph[e] = a_; pm[e] = b_; pl[e] = c_;
                }
                const bf16x8 p0 = __builtin_bit_cast(bf16x8, ph), p1 = __builtin_bit_cast(bf16x8, pm), p2 = __builtin_bit_cast(bf16x8, pl);
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    // V^T[d = 32dt + li][keys 32t + 16u + 4hi + {0..3}] and [.. + 8 + {0..3}]
                    const unsigned char* vr = Vp + (32 * dt + li) * AS_VROW + (32 * t + 16 * u + 4 * lh) * 2;
                    bf16x8 v[3];
#pragma unroll
                    for (int pl_ = 0; pl_ < OP; ++pl_) {
                        const u32x2 lo = *reinterpret_cast<const u32x2*>(vr + pl_ * VPL);
                        const u32x2 hi2 = *reinterpret_cast<const u32x2*>(vr + pl_ * VPL + 16);
                        v[pl_] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi2[0], hi2[1]});
                    }
                    if (OP == 3) ot[dt] = mfma16<F16>(v[2], p0, ot[dt]);
                    if (PP == 3) ot[dt] = mfma16<F16>(v[0], p2, ot[dt]);
                    if (OP == 3 || PP == 3) ot[dt] = mfma16<F16>(v[1], p1, ot[dt]);   // second x second piece: <= 2^-18 of the term
                    ot[dt] = mfma16<F16>(v[1], p0, ot[dt]);
                    ot[dt] = mfma16<F16>(v[0], p1, ot[dt]);
                    ot[dt] = mfma16<F16>(v[0], p0, ot[dt]);
                }
            }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] = F16 ? fmaf(ot[dt][r], o_inv, oacc[dt][r]) : oacc[dt][r] + ot[dt][r];
        // next tile: registers -> the other stage (its previous readers finished before the last barrier), prefetch the one after
        if (kt + 1 < ntiles) stage(stg ^ 1);
        if (kt + 2 < ntiles) fetch(kt + 2);
        __syncthreads();
    }
    const float inv_l = 1.0f / l_run;
    float* Os = reinterpret_cast<float*>(smem) + wave * 32 * (DH + 1);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) Os[li * (DH + 1) + 32 * dt + crow(r, lh)] = oacc[dt][r] * inv_l;
    __syncthreads();
    float* o_dst = KS > 1 ? p.o_part + (long)khalf * p.B * p.S * p.H * D : p.o;
    const long o_ld = KS > 1 ? (long)p.H * D : p.ldo;
    for (int rr = lh; rr < 32; rr += 2) {
        const int qi = q0 + rr;
        if (qi >= p.S) break;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            if (32 * dt + li < D) o_dst[((long)b * p.S + qi) * o_ld + (long)h * D + 32 * dt + li] = Os[rr * (DH + 1) + 32 * dt + li];
    }
    if (lh == 0 && q0 + li < p.S)
        (KS > 1 ? p.lse_part + (long)khalf * p.B * p.H * p.S : p.lse)[((long)b * p.H + h) * p.S + q0 + li] = m_run * sm_scale + logf(l_run);
}

// joins the two halves of the key-split forward: per (row, head) w_i = exp(lse_i - lse), o = w1 o1 + w2 o2 (four columns per thread)
__global__ __launch_bounds__(256) void attn_fwd_combine_kernel(const AttnArgs p) {
    const int D = p.D, c4n = D >> 2;
    const long total = (long)p.B * p.S * p.H * c4n;
    const long half_o = (long)p.B * p.S * p.H * D, half_l = (long)p.B * p.H * p.S;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n) * 4;
        const long rh = i / c4n;
        const int h = (int)(rh % p.H);
        const long row = rh / p.H;                 // b * S + s
        const long b = row / p.S, sq = row - b * p.S;
        const long li_ = (b * p.H + h) * p.S + sq;
        const float l1 = p.lse_part[li_], l2 = p.lse_part[half_l + li_];
        const float m = fmaxf(l1, l2);
        const float w1 = expf(l1 - m), w2 = expf(l2 - m);
        const float inv = 1.f / (w1 + w2);
        const f32x4 a = *reinterpret_cast<const f32x4*>(p.o_part + row * ((long)p.H * D) + (long)h * D + c);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(p.o_part + half_o + row * ((long)p.H * D) + (long)h * D + c);
        *reinterpret_cast<f32x4*>(p.o + row * p.ldo + (long)h * D + c) = (a * (w1 * inv)) + (bb * (w2 * inv));
        if (c == 0) p.lse[li_] = m + logf(w1 + w2);
    }
}

// ---------------------------------------------------------------------------------------------
// software-pipelined forward (8 waves x 32 queries, S a multiple of 64): the loop body is ONE basic block in which
//   S^T(t+1) = K(t+1) Q^T      (24 MFMAs, independent of everything else in the iteration)
//   softmax(t), split of P(t)   (VALU)
//   O^T += V(t)^T P(t)^T        (24 MFMAs)
//   staging of V(t+1), K(t+2)   (VALU + LDS writes)
// sit side by side, so the matrix pipe works on the next tile's scores while the vector pipe does this tile's softmax.  No
// branch in the loop: the O rescale is unconditional (alpha == 1 exactly when the running max did not move), tiles past the
// end are staged from clamped rows and never used.  No packed-fp32 instruction in the loop (common.h: they serialise the
// matrix pipe with the vector stream).  Same arithmetic per tile as attn_fwd_split_kernel.
// ABL (tools/attn_ablate.hip only): 1 no S MFMAs, 2 no PV MFMAs, 4 no P split, 8 no K/V staging, 16 no exp, 32 no barrier
// ---------------------------------------------------------------------------------------------
template <int ABL = 0>
__global__ __launch_bounds__(512, 1) void attn_fwd_split_pipe_kernel(const AttnArgs p) {
    constexpr int NW = 8, KT = 64, QB = 32 * NW;
    constexpr int KST = 3 * AS_KPL, VST = 3 * AS_VPL;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * KST + 2 * VST];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, blk;
    xcd_group_decode(blockIdx.x, p.B * p.H, (p.S + QB - 1) / QB, bh, blk);
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int q0 = blk * QB + wave * 32;
    const float c = p.scale * LOG2E;

    bf16x8 qf[3][2];
    {
        const int qi = q0 + li;
        const float* qrow = p.q + ((long)b * p.S + qi) * p.ldq + (long)h * 32;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 v0 = load4(qrow, 16 * u + 8 * lh, 32, qi < p.S, true);
            const f32x4 v1 = load4(qrow, 16 * u + 8 * lh + 4, 32, qi < p.S, true);
            u32x4 ph, pm, pl;
            unsigned a_, b_, c_;
            split3_pair(v0[0], v0[1], a_, b_, c_); ph[0] = a_; pm[0] = b_; pl[0] = c_;
            split3_pair(v0[2], v0[3], a_, b_, c_); ph[1] = a_; pm[1] = b_; pl[1] = c_;
            split3_pair(v1[0], v1[1], a_, b_, c_); ph[2] = a_; pm[2] = b_; pl[2] = c_;
            split3_pair(v1[2], v1[3], a_, b_, c_); ph[3] = a_; pm[3] = b_; pl[3] = c_;
            qf[0][u] = __builtin_bit_cast(bf16x8, ph); qf[1][u] = __builtin_bit_cast(bf16x8, pm); qf[2][u] = __builtin_bit_cast(bf16x8, pl);
        }
    }
    const float* kbase = p.k + (long)b * p.S * p.ldk + (long)hk * 32;
    const float* vbase = p.v + (long)b * p.S * p.ldv + (long)hk * 32;
    // staging roles: K item (key = tid >> 3, 4-d chunk = tid & 7) for every thread; V^T item (key pair kp = tid >> 3, chunk)
    // for the first 256 threads
    const bool vthread = tid < 256;
    const int srow = tid >> 3, sch = tid & 7;
    f32x4 rk, rv[2];
    auto fetch_k = [&](int kt) {
        rk = *reinterpret_cast<const f32x4*>(kbase + (long)min(kt * KT + srow, p.S - 1) * p.ldk + sch * 4);
    };
    auto fetch_v = [&](int kt) {
        if (vthread) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                rv[i] = *reinterpret_cast<const f32x4*>(vbase + (long)min(kt * KT + 2 * srow + i, p.S - 1) * p.ldv + sch * 4);
        }
    };
    auto stage_k = [&](int stg) {
        u32x2 hh, mm, ll;
        unsigned a_, b_, c_;
        split3_pair(rk[0], rk[1], a_, b_, c_); hh[0] = a_; mm[0] = b_; ll[0] = c_;
        split3_pair(rk[2], rk[3], a_, b_, c_); hh[1] = a_; mm[1] = b_; ll[1] = c_;
        unsigned char* dst = smem + stg * KST + srow * AS_KROW + sch * 8;
        *reinterpret_cast<u32x2*>(dst) = hh;
        *reinterpret_cast<u32x2*>(dst + AS_KPL) = mm;
        *reinterpret_cast<u32x2*>(dst + 2 * AS_KPL) = ll;
    };
    auto stage_v = [&](int stg) {
        if (vthread) {
            unsigned char* Vp = smem + 2 * KST + stg * VST;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_, c_;
                split3_pair(rv[0][e], rv[1][e], a_, b_, c_);
                unsigned char* dst = Vp + (sch * 4 + e) * AS_VROW + srow * 4;
                *reinterpret_cast<unsigned*>(dst) = a_;
                *reinterpret_cast<unsigned*>(dst + AS_VPL) = b_;
                *reinterpret_cast<unsigned*>(dst + 2 * AS_VPL) = c_;
            }
        }
    };
    auto scores = [&](int stg, f32x16 (&s)[2]) {
        const unsigned char* Kp = smem + stg * KST;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const unsigned char* kr = Kp + (32 * t + li) * AS_KROW + u * 32 + lh * 16;
                const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(kr);
                const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(kr + AS_KPL);
                const bf16x8 k2 = *reinterpret_cast<const bf16x8*>(kr + 2 * AS_KPL);
                if (ABL & 1) { s[t][4 * u] += __builtin_bit_cast(f32x4, k0)[0] + __builtin_bit_cast(f32x4, k1)[1] + __builtin_bit_cast(f32x4, k2)[2]; continue; }
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k2, qf[0][u], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, qf[2][u], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1, qf[1][u], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1, qf[0][u], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, qf[1][u], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, qf[0][u], s[t], 0, 0, 0);
            }
        }
    };

    f32x16 oacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = p.S / KT;
    // prologue: K(0), V(0) staged; S(0) computed; K(1) staged; K(2), V(1) in flight
    fetch_k(0); fetch_v(0);
    stage_k(0); stage_v(0);
    fetch_k(1); fetch_v(1);
    __syncthreads();
    f32x16 s[2], sn[2];
    scores(0, s);
    stage_k(1);
    fetch_k(2);
    __syncthreads();
    for (int kt = 0; kt < ntiles; ++kt) {
        const int stg = kt & 1;
        // ---- (0) LDS reads of the K(kt + 1) fragments, issued ahead of the region that uses them
        bf16x8 kfr[2][2][3];
        {
            const unsigned char* Kp = smem + (stg ^ 1) * KST;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const unsigned char* kr = Kp + (32 * t + li) * AS_KROW + u * 32 + lh * 16;
#pragma unroll
                    for (int pl_ = 0; pl_ < 3; ++pl_) kfr[t][u][pl_] = *reinterpret_cast<const bf16x8*>(kr + pl_ * AS_KPL);
                }
        }
        // ---- (1) floating-point region, no MFMA in it: online softmax over the 64 keys of tile kt.  (Floating-point vector
        // instructions of one wave do not overlap with MFMAs of the other wave of the SIMD, integer ones do:
        // tools/pipe_overlap.hip.  Both waves run this code in step, so the matrix work goes where the integer work is.)
        float mx = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; r += 1) mx = fmaxf(fmaxf(mx, s[0][r]), s[1][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float mc = -m_new * c;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = fmaf(s[t][r], c, mc);
                s[t][r] = (ABL & 16) ? a : __builtin_amdgcn_exp2f(a);
                ps += s[t][r];          // plain C on purpose: inline asm reading a v_exp_f32 result misses the trans-use wait state
            }
        ps += __shfl_xor(ps, 32, 64);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        __builtin_amdgcn_sched_barrier(0);
        // ---- (2) matrix + integer region: P split, O^T += V^T P^T, S^T(kt + 1) = K(kt + 1) Q^T, staging
        const unsigned char* Vp = smem + 2 * KST + stg * VST;
        // the tile's P V product starts from zero and joins O on the vector pipe (attn_fwd_split_kernel: the bf16 MFMA does not
        // round its accumulator to nearest; long same-signed accumulations drift)
        f32x16 ot;
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[r] = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sn[t][r] = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                u32x4 ph, pm, pl;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned a_, b_, c_;
                    if (ABL & 4) { a_ = __float_as_uint(s[t][8 * u + 2 * e]); b_ = __float_as_uint(s[t][8 * u + 2 * e + 1]); c_ = a_ ^ b_; }
                    else split3_pair(s[t][8 * u + 2 * e], s[t][8 * u + 2 * e + 1], a_, b_, c_);
                    ph[e] = a_; pm[e] = b_; pl[e] = c_;
                }
                const bf16x8 p0 = __builtin_bit_cast(bf16x8, ph), p1 = __builtin_bit_cast(bf16x8, pm), p2 = __builtin_bit_cast(bf16x8, pl);
                const unsigned char* vr = Vp + li * AS_VROW + (32 * t + 16 * u + 4 * lh) * 2;
                bf16x8 v[3];
#pragma unroll
                for (int pl_ = 0; pl_ < 3; ++pl_) {
                    const u32x2 lo = *reinterpret_cast<const u32x2*>(vr + pl_ * AS_VPL);
                    const u32x2 hi2 = *reinterpret_cast<const u32x2*>(vr + pl_ * AS_VPL + 16);
                    v[pl_] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi2[0], hi2[1]});
                }
                if (!(ABL & 2)) {
                    ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[2], p0, ot, 0, 0, 0);
                    ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[0], p2, ot, 0, 0, 0);
                    ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[1], p1, ot, 0, 0, 0);
                    ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[1], p0, ot, 0, 0, 0);
                    ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[0], p1, ot, 0, 0, 0);
                    ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v[0], p0, ot, 0, 0, 0);
                } else {
                    const f32x4 z = __builtin_bit_cast(f32x4, v[0]) + __builtin_bit_cast(f32x4, v[1]) + __builtin_bit_cast(f32x4, v[2]) + __builtin_bit_cast(f32x4, p0) + __builtin_bit_cast(f32x4, p1) + __builtin_bit_cast(f32x4, p2);
                    ot[4 * (2 * t + u)] += z[0]; ot[4 * (2 * t + u) + 1] += z[1]; ot[4 * (2 * t + u) + 2] += z[2]; ot[4 * (2 * t + u) + 3] += z[3];
                }
                if (!(ABL & 1)) {
                    sn[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[t][u][2], qf[0][u], sn[t], 0, 0, 0);
                    sn[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[t][u][0], qf[2][u], sn[t], 0, 0, 0);
                    sn[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[t][u][1], qf[1][u], sn[t], 0, 0, 0);
                    sn[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[t][u][1], qf[0][u], sn[t], 0, 0, 0);
                    sn[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[t][u][0], qf[1][u], sn[t], 0, 0, 0);
                    sn[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[t][u][0], qf[0][u], sn[t], 0, 0, 0);
                } else {
                    sn[t][4 * u] += __builtin_bit_cast(f32x4, kfr[t][u][0])[0] + __builtin_bit_cast(f32x4, kfr[t][u][1])[1] + __builtin_bit_cast(f32x4, kfr[t][u][2])[2];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[r] = oacc[r] * alpha + ot[r];      // alpha == 1 exactly when the running max did not move; plain C (hazards: see above)
        // staging for the iterations to come (rows clamped: tiles past the end are harmless copies of the last row)
        if (!(ABL & 8)) {
            stage_v(stg ^ 1);          // V(kt + 1): its slot held V(kt - 1), read before the last barrier
            stage_k(stg);              // K(kt + 2): its slot held K(kt), read before the last barrier
            fetch_v(kt + 2);
            fetch_k(kt + 3);
        }
        if (!(ABL & 32)) __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) s[t] = sn[t];
    }
    const float inv_l = 1.0f / l_run;
    float* Os = reinterpret_cast<float*>(smem) + wave * 32 * 33;          // 8 * 4224 B <= the K stages
#pragma unroll
    for (int r = 0; r < 16; ++r) Os[li * 33 + crow(r, lh)] = oacc[r] * inv_l;
    __syncthreads();
    for (int rr = lh; rr < 32; rr += 2) {
        const int qi = q0 + rr;
        if (qi >= p.S) break;
        p.o[((long)b * p.S + qi) * p.ldo + (long)h * 32 + li] = Os[rr * 33 + li];
    }
    if (lh == 0 && q0 + li < p.S)
        p.lse[((long)b * p.H + h) * p.S + q0 + li] = m_run * p.scale + logf(l_run);
}

// ---------------------------------------------------------------------------------------------
// backward helpers
// ---------------------------------------------------------------------------------------------
// delta[b,h,s] = sum_d dO * O       (one thread per (b,s,h); rows are short)
__global__ void attn_delta_kernel(const AttnArgs p) {
    const long total = (long)p.B * p.S * p.H;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int h = (int)(gid % p.H);
    const long bs = gid / p.H;
    const int s = (int)(bs % p.S), b = (int)(bs / p.S);
    const float* o = p.oin + bs * p.ldo + (long)h * p.D;
    const float* g = p.dout + bs * p.ldo + (long)h * p.D;
    float acc = 0.f;
    for (int d = 0; d < p.D; ++d) acc += o[d] * g[d];
    p.delta[((long)b * p.H + h) * p.S + s] = acc;
}

// 16-byte variant: LPR lanes per (b,s,h) row, shuffle-reduced (coalesced 16 B per lane)
__global__ void attn_delta_vec_kernel(const AttnArgs p, int lpr) {
    const long total = (long)p.B * p.S * p.H;
    const long gid = ((long)blockIdx.x * blockDim.x + threadIdx.x) / lpr;
    const int sub = threadIdx.x % lpr;
    float acc = 0.f;
    if (gid < total) {
        const int h = (int)(gid % p.H);
        const long bs = gid / p.H;
        const float* o = p.oin + bs * p.ldo + (long)h * p.D;
        const float* g = p.dout + bs * p.ldo + (long)h * p.D;
        for (int d = sub * 4; d < p.D; d += lpr * 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(o + d), b = *reinterpret_cast<const f32x4*>(g + d);
            acc += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
        }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (gid < total && sub == 0) {
        const int h = (int)(gid % p.H);
        const long bs = gid / p.H;
        p.delta[((long)(bs / p.S) * p.H + h) * p.S + (bs % p.S)] = acc;
    }
}

// dq[b,s,h,:] = scale * sum_kb part[kb][b,h,s,:]
__global__ void attn_dq_reduce_kernel(const AttnArgs p, int DP) {
    const long total = (long)p.B * p.H * p.S * DP;
    float am = 0.f;
    for (long gid = (long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long)gridDim.x * blockDim.x) {
        const int d = (int)(gid % DP);
        if (d >= p.D) continue;
        const long bhs = gid / DP;
        const int s = (int)(bhs % p.S);
        const long bh = bhs / p.S;
        const int h = (int)(bh % p.H), b = (int)(bh / p.H);
        float acc = 0.f;
        for (int kb = 0; kb < p.n_kblocks; ++kb) acc += p.dq_part[(long)kb * total + gid];
        p.dq[((long)b * p.S + s) * p.lddq + (long)h * p.D + d] = acc * p.scale;
        am = fmaxf(am, fabsf(acc * p.scale));
    }
    if (p.dqkv_amax) amax_publish(p.dqkv_amax, am, threadIdx.x & 63, (int)blockIdx.x * 4 + (threadIdx.x >> 6));
}

// 16-byte form (head_dim % 4 == 0, aligned dq): a thread sums one float4 over the slabs, four slabs in flight; one atomic per workgroup
// for the word.  DP4 = padded head_dim / 4 (8: head_dim 32; 16 / 32: head_dim <= 64 / <= 128, whose padding columns are skipped).
template <int DP4>
__global__ __launch_bounds__(256) void attn_dq_reduce_vec_kernel(const AttnArgs p) {
    __shared__ float amred[4];
    const int total4 = p.B * p.H * p.S * DP4;                 // float4 items (checked on the host: fits an int)
    const long slab4 = (long)total4;
    float am = 0.f;
    for (int gid = blockIdx.x * 256 + threadIdx.x; gid < total4; gid += gridDim.x * 256) {
        const int d4 = gid % DP4, bhs = gid / DP4;
        if (DP4 != 8 && d4 * 4 >= p.D) continue;
        const int s_ = bhs % p.S, bh = bhs / p.S;
        const int h = bh % p.H, b = bh / p.H;
        const f32x4* src = reinterpret_cast<const f32x4*>(p.dq_part) + gid;
        f32x4 acc = src[0];
        int kb = 1;
        for (; kb + 3 < p.n_kblocks; kb += 4) {
            const f32x4 t0 = src[(long)kb * slab4], t1 = src[(long)(kb + 1) * slab4], t2 = src[(long)(kb + 2) * slab4], t3 = src[(long)(kb + 3) * slab4];
            acc += t0; acc += t1; acc += t2; acc += t3;
        }
        for (; kb < p.n_kblocks; ++kb) acc += src[(long)kb * slab4];
        acc *= p.scale;
        *reinterpret_cast<f32x4*>(p.dq + ((long)b * p.S + s_) * p.lddq + h * p.D + d4 * 4) = acc;
        am = fmaxf(am, fmaxf(fmaxf(fabsf(acc[0]), fabsf(acc[1])), fmaxf(fabsf(acc[2]), fabsf(acc[3]))));
    }
    if (p.dqkv_amax) amax_publish_block<4>(p.dqkv_amax, am, amred);
}

// ---------------------------------------------------------------------------------------------
// backward main: workgroup = 4 waves, each owns 32 keys (block = 128 keys); loops over query tiles of 32
// ---------------------------------------------------------------------------------------------
template <int DP, bool DROP = false>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const AttnArgs p) {
    constexpr int ND = DP / 32;
    constexpr int LDT = DP + 4;
    constexpr int NF4 = (32 * DP / 4 + 255) / 256;   // float4 per thread per 32-row tile (1 for DP=32, 2 for 64)
    constexpr int F4_PER_TILE = 32 * DP / 4;
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    float* Qs = dyn;                               // [32][LDT]
    float* Gs = Qs + 32 * LDT;                     // dO tile [32][LDT]
    float* lse_s = Gs + 32 * LDT;                  // [32]
    float* del_s = lse_s + 32;                     // [32]
    float* Kw = del_s + 32;                        // per wave [32][DP]
    float* Sw = Kw + 4 * 32 * DP;                  // per wave dS^T staging [32][33]
    float* Pq = Sw + 4 * 32 * 33;                  // per wave dQ partial [32][PQW]: at most 64 columns at a time (head_dim 128: two passes)
    constexpr int PQW = DP < 64 ? DP : 64, NCH = DP / PQW, TPC = PQW / 32;      // partial width, passes, 32-wide d tiles per pass

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int bh, kblk;
    xcd_group_decode(blockIdx.x, p.B * p.H, p.n_kblocks, bh, kblk);     // key blocks of one (b,h) share Q / dO: same XCD
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int kv0 = kblk * 128 + wave * 32;
    const int D = p.D;
    const bool vec = p.vec != 0;
    const float c = p.scale * LOG2E;
    float* Kmine = Kw + wave * 32 * DP;
    float* Smine = Sw + wave * 32 * 33;
    float* Pmine = Pq + wave * 32 * PQW;

    // K^T / V^T operands for this lane's key (column li): K[kv][8g + 4lh + s]
    float kreg[DP / 2], vreg[DP / 2];
    const bool kv_ok = kv0 + li < p.S;
    {
        const float* krow = p.k + ((long)b * p.S + kv0 + li) * p.ldk + (long)hk * D;
        const float* vrow = p.v + ((long)b * p.S + kv0 + li) * p.ldv + (long)hk * D;
#pragma unroll
        for (int g = 0; g < DP / 8; ++g) {
            const f32x4 a = load4(krow, 8 * g + 4 * lh, D, kv_ok, vec);
            const f32x4 w = load4(vrow, 8 * g + 4 * lh, D, kv_ok, vec);
#pragma unroll
            for (int t = 0; t < 4; ++t) { kreg[4 * g + t] = a[t]; vreg[4 * g + t] = w[t]; }
        }
        // the wave's K tile, row-major, for the dQ product (B operand read row-contiguously)
        for (int t = lane; t < 32 * DP / 4; t += 64) {
            const int row = t / (DP / 4), d = (t % (DP / 4)) * 4;
            const f32x4 a = load4(p.k + ((long)b * p.S + kv0 + row) * p.ldk + (long)hk * D, d, D, kv0 + row < p.S, vec);
            *reinterpret_cast<f32x4*>(Kmine + row * DP + d) = a;
        }
    }
    f32x16 dvacc[ND], dkacc[ND];
#pragma unroll
    for (int t = 0; t < ND; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dvacc[t][r] = 0.f; dkacc[t][r] = 0.f; }

    const float* qbase = p.q + (long)b * p.S * p.ldq + (long)h * D;
    const float* gbase = p.dout + (long)b * p.S * p.ldo + (long)h * D;
    const float* lse_b = p.lse + ((long)b * p.H + h) * p.S;
    const float* del_b = p.delta + ((long)b * p.H + h) * p.S;
    f32x4 rq[NF4], rg[NF4];
    float rl = 0.f, rd = 0.f;
    auto fetch = [&](int q0) {
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            if (t < F4_PER_TILE) {
                const int row = t / (DP / 4), d = (t % (DP / 4)) * 4;
                const bool ok = q0 + row < p.S;
                rq[i] = load4(qbase + (long)(q0 + row) * p.ldq, d, D, ok, vec);
                rg[i] = load4(gbase + (long)(q0 + row) * p.ldo, d, D, ok, vec);
            }
        }
        if (tid < 32) {
            const bool ok = q0 + tid < p.S;
            rl = ok ? lse_b[q0 + tid] * LOG2E : INFINITY;   // +inf -> P = 0 for padded queries
            rd = ok ? del_b[q0 + tid] : 0.f;
        }
    };
    const int nq = (p.S + 31) / 32;
    const long part_stride = (long)p.B * p.H * p.S * DP;
    float* part = p.dq_part + (long)kblk * part_stride + ((long)b * p.H + h) * p.S * DP;

    fetch(0);
    for (int qt = 0; qt < nq; ++qt) {
        const int q0 = qt * 32;
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            if (t < F4_PER_TILE) {
                const int row = t / (DP / 4), d = (t % (DP / 4)) * 4;
                *reinterpret_cast<f32x4*>(Qs + row * LDT + d) = rq[i];
                *reinterpret_cast<f32x4*>(Gs + row * LDT + d) = rg[i];
            }
        }
        if (tid < 32) { lse_s[tid] = rl; del_s[tid] = rd; }
        __syncthreads();                                    // barrier A
        if (qt + 1 < nq) fetch(q0 + 32);

        // ---- S[q][kv] and dP[q][kv]
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
        {
            const float* qrow = Qs + li * LDT + 4 * lh;
            const float* grow = Gs + li * LDT + 4 * lh;
#pragma unroll
            for (int g = 0; g < DP / 8; ++g) {
                const f32x4 qa = *reinterpret_cast<const f32x4*>(qrow + 8 * g);
                const f32x4 ga = *reinterpret_cast<const f32x4*>(grow + 8 * g);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[t], kreg[4 * g + t], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[t], vreg[4 * g + t], dp, 0, 0, 0);
                }
            }
        }
        // ---- P = exp(S*scale - lse), dS = P * (dP - delta)   (rows q = crow(r,lh), column kv = li)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = crow(r, lh);
            float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse_s[qr]));
            if (!kv_ok) pv = 0.f;
            if (DROP) {      // O = (P o M) V: dV takes P o M, dS = P o (M o dP - delta); delta = rowsum(dO o O) as without dropout
                const float m = attn_drop_factor(*p.drop_seed, (((long)b * p.H + h) * p.S + (q0 + qr)) * p.S + kv0 + li, p.drop_thresh, p.drop_scale);
                s[r] = pv * m;
                dp[r] = pv * (dp[r] * m - del_s[qr]);
            } else {
                s[r] = pv;
                dp[r] = pv * (dp[r] - del_s[qr]);
            }
        }
        // ---- dV^T[d][kv] += dO^T[d][q] P[q][kv] ; dK^T[d][kv] += Q^T[d][q] dS[q][kv]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* grow = Gs + crow(r, lh) * LDT + li;
            const float* qrow = Qs + crow(r, lh) * LDT + li;
#pragma unroll
            for (int t = 0; t < ND; ++t) {
                dvacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[32 * t], s[r], dvacc[t], 0, 0, 0);
                dkacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[32 * t], dp[r], dkacc[t], 0, 0, 0);
            }
        }
        // ---- dQ[q][d] partial = sum_kv dS[q][kv] K[kv][d] : dS goes through wave-private LDS to flip lanes
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[crow(r, lh) * 33 + li] = dp[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x16 dq[ND];
#pragma unroll
        for (int t = 0; t < ND; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[t][r] = 0.f;
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) {
            const int kvs = t16 + 16 * lh;
            const float a = Smine[li * 33 + kvs];
#pragma unroll
            for (int t = 0; t < ND; ++t)
                dq[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Kmine[kvs * DP + 32 * t + li], dq[t], 0, 0, 0);
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch > 0) __syncthreads();                    // the previous pass's partials have been summed
#pragma unroll
            for (int t = 0; t < TPC; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) Pmine[crow(r, lh) * PQW + 32 * t + li] = dq[ch * TPC + t][r];
            __syncthreads();                                // barrier B
            // fixed-order sum of the four waves' partials -> this key block's slice of the dQ workspace
            for (int t = tid; t < 32 * PQW; t += 256) {
                const int row = t / PQW;
                if (q0 + row < p.S)
                    part[(long)(q0 + row) * DP + ch * PQW + (t % PQW)] = Pq[t] + Pq[32 * PQW + t] + Pq[2 * 32 * PQW + t] + Pq[3 * 32 * PQW + t];
            }
        }
    }
    // ---- epilogue: dK^T, dV^T -> [kv][d] through wave-private LDS, coalesced row stores (per QUERY head h)
    __syncthreads();
    float* T = Kmine;   // 32*DP floats; transposed staging with stride DP+1 would overflow -> two passes over Smine-sized rows
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            // stage one 32(d) x 32(kv) block transposed into Smine [kv][33]
#pragma unroll
            for (int r = 0; r < 16; ++r) Smine[li * 33 + crow(r, lh)] = (pass == 0 ? dkacc[t][r] * p.scale : dvacc[t][r]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int rr = lh; rr < 32; rr += 2) {
                const int kv = kv0 + rr;
                const int d = 32 * t + li;
                if (kv < p.S && d < D) {
                    if (pass == 0) p.dk[((long)b * p.S + kv) * p.lddk + (long)h * D + d] = Smine[rr * 33 + li];
                    else           p.dv[((long)b * p.S + kv) * p.lddv + (long)h * D + d] = Smine[rr * 33 + li];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    (void)T;
}

// ---------------------------------------------------------------------------------------------
// backward on the bf16 matrix pipe (head_dim == 32, 16-byte aligned operands), same structure as attn_bwd_kernel: a
// workgroup = 4 waves x 32 keys, loop over 32-query tiles.  S, dP, dV^T, dK^T run as six bf16 piece products each
// (fp32-exact, see gemm_split.hip): K / V live in registers as split B operands; the Q / dO tile is staged as split planes in
// BOTH orientations ([q][d] for S / dP, [d][q] for dV^T / dK^T, whose k-slots are the lane's own P / dS registers); P and dS
// are split in registers.  dQ keeps the fp32 MFMA path (dS through the wave-private LDS transpose against the fp32 K tile):
// its operand would need a third, per-wave set of planes and the workgroup would no longer fit twice on a CU.
// ---------------------------------------------------------------------------------------------
constexpr int AB_KROW = 80, AB_TROW = 72;
constexpr int AB_KPL = 32 * AB_KROW, AB_TPL = 32 * AB_TROW;
constexpr int AB_LDS = 2 * 3 * AB_KPL + 2 * 3 * AB_TPL + 64 * 4 + 4 * 32 * 32 * 4 + 4 * 32 * 33 * 4;

__global__ __launch_bounds__(256, 2) void attn_bwd_split_kernel(const AttnArgs p) {
    constexpr int DP = 32;
    __shared__ __attribute__((aligned(16))) unsigned char smem[AB_LDS];
    unsigned char* Qk = smem;                       // 3 planes [q][32 d]
    unsigned char* Gk = Qk + 3 * AB_KPL;            // dO
    unsigned char* Qt = Gk + 3 * AB_KPL;            // 3 planes [d][32 q]
    unsigned char* Gt = Qt + 3 * AB_TPL;
    float* lse_s = reinterpret_cast<float*>(Gt + 3 * AB_TPL);
    float* del_s = lse_s + 32;
    float* Kw = del_s + 32;                         // per wave fp32 K tile [32][32] (dQ product)
    float* Sw = Kw + 4 * 32 * 32;                   // per wave dS^T staging [32][33]; reused as the wave's dQ partial [32][32]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, kblk;
    xcd_group_decode(blockIdx.x, p.B * p.H, p.n_kblocks, bh, kblk);
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int kv0 = kblk * 128 + wave * 32;
    const float c = p.scale * LOG2E;
    float* Kmine = Kw + wave * 32 * 32;
    float* Smine = Sw + wave * 32 * 33;
    float* Pmine = Smine;

    // K^T / V^T as split B operands: lane (kv = li, hi) holds d = 16u + 8hi + e
    bf16x8 kf[3][2], vf[3][2];
    const bool kv_ok = kv0 + li < p.S;
    {
        const float* krow = p.k + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldk + (long)hk * 32;
        const float* vrow = p.v + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldv + (long)hk * 32;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(krow + 16 * u + 8 * lh), a1 = *reinterpret_cast<const f32x4*>(krow + 16 * u + 8 * lh + 4);
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(vrow + 16 * u + 8 * lh), w1 = *reinterpret_cast<const f32x4*>(vrow + 16 * u + 8 * lh + 4);
            u32x4 ph, pm, pl, vh, vm, vl;
            unsigned a_, b_, c_;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                split3_pair(a0[2 * e], a0[2 * e + 1], a_, b_, c_); ph[e] = a_; pm[e] = b_; pl[e] = c_;
                split3_pair(a1[2 * e], a1[2 * e + 1], a_, b_, c_); ph[2 + e] = a_; pm[2 + e] = b_; pl[2 + e] = c_;
                split3_pair(w0[2 * e], w0[2 * e + 1], a_, b_, c_); vh[e] = a_; vm[e] = b_; vl[e] = c_;
                split3_pair(w1[2 * e], w1[2 * e + 1], a_, b_, c_); vh[2 + e] = a_; vm[2 + e] = b_; vl[2 + e] = c_;
            }
            kf[0][u] = __builtin_bit_cast(bf16x8, ph); kf[1][u] = __builtin_bit_cast(bf16x8, pm); kf[2][u] = __builtin_bit_cast(bf16x8, pl);
            vf[0][u] = __builtin_bit_cast(bf16x8, vh); vf[1][u] = __builtin_bit_cast(bf16x8, vm); vf[2][u] = __builtin_bit_cast(bf16x8, vl);
        }
        // the wave's fp32 K tile, row-major, for the dQ product
        for (int t = lane; t < 32 * 8; t += 64) {
            const int row = t >> 3, d = (t & 7) * 4;
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (kv0 + row < p.S) a = *reinterpret_cast<const f32x4*>(p.k + ((long)b * p.S + kv0 + row) * p.ldk + (long)hk * 32 + d);
            *reinterpret_cast<f32x4*>(Kmine + row * 32 + d) = a;
        }
    }
    f32x16 dvacc, dkacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dvacc[r] = 0.f; dkacc[r] = 0.f; }

    const float* qbase = p.q + (long)b * p.S * p.ldq + (long)h * 32;
    const float* gbase = p.dout + (long)b * p.S * p.ldo + (long)h * 32;
    const float* lse_b = p.lse + ((long)b * p.H + h) * p.S;
    const float* del_b = p.delta + ((long)b * p.H + h) * p.S;
    // prefetch registers: k-major pieces (row = tid >> 3, chunk = tid & 7) of Q and dO; transposed pieces: threads 0..127 take
    // Q rows (2qp, 2qp+1), threads 128..255 the same of dO (qp = (tid & 127) >> 3, chunk = tid & 7)
    f32x4 rq, rg, rt[2];
    float rl = 0.f, rd = 0.f;
    auto fetch = [&](int q0) {
        {
            const int row = tid >> 3, d = (tid & 7) * 4;
            const bool ok = q0 + row < p.S;
            const long r = min(q0 + row, p.S - 1);
            rq = *reinterpret_cast<const f32x4*>(qbase + r * p.ldq + d);
            rg = *reinterpret_cast<const f32x4*>(gbase + r * p.ldo + d);
            if (!ok) { rq = f32x4{0.f, 0.f, 0.f, 0.f}; rg = rq; }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = 2 * ((tid & 127) >> 3) + i, d = (tid & 7) * 4;
            const bool ok = q0 + row < p.S;
            const long r = min(q0 + row, p.S - 1);
            rt[i] = tid < 128 ? *reinterpret_cast<const f32x4*>(qbase + r * p.ldq + d) : *reinterpret_cast<const f32x4*>(gbase + r * p.ldo + d);
            if (!ok) rt[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (tid < 32) {
            const bool ok = q0 + tid < p.S;
            rl = ok ? lse_b[q0 + tid] * LOG2E : INFINITY;   // +inf -> P = 0 for padded queries
            rd = ok ? del_b[q0 + tid] : 0.f;
        }
    };
    const int nq = (p.S + 31) / 32;
    const long part_stride = (long)p.B * p.H * p.S * DP;
    float* part = p.dq_part + (long)kblk * part_stride + ((long)b * p.H + h) * p.S * DP;

    fetch(0);
    for (int qt = 0; qt < nq; ++qt) {
        const int q0 = qt * 32;
        // ---- stage the tile as split planes, both orientations
        {
            const int row = tid >> 3, ch = tid & 7;
            u32x2 h2, m2, l2;
            unsigned a_, b_, c_;
            split3_pair(rq[0], rq[1], a_, b_, c_); h2[0] = a_; m2[0] = b_; l2[0] = c_;
            split3_pair(rq[2], rq[3], a_, b_, c_); h2[1] = a_; m2[1] = b_; l2[1] = c_;
            unsigned char* dq_ = Qk + row * AB_KROW + ch * 8;
            *reinterpret_cast<u32x2*>(dq_) = h2; *reinterpret_cast<u32x2*>(dq_ + AB_KPL) = m2; *reinterpret_cast<u32x2*>(dq_ + 2 * AB_KPL) = l2;
            split3_pair(rg[0], rg[1], a_, b_, c_); h2[0] = a_; m2[0] = b_; l2[0] = c_;
            split3_pair(rg[2], rg[3], a_, b_, c_); h2[1] = a_; m2[1] = b_; l2[1] = c_;
            unsigned char* dg_ = Gk + row * AB_KROW + ch * 8;
            *reinterpret_cast<u32x2*>(dg_) = h2; *reinterpret_cast<u32x2*>(dg_ + AB_KPL) = m2; *reinterpret_cast<u32x2*>(dg_ + 2 * AB_KPL) = l2;
            // transposed: (q = 2qp, 2qp+1) pairs of this thread's 4 d columns
            const int qp = (tid & 127) >> 3, d0 = ch * 4;
            unsigned char* tb = (tid < 128 ? Qt : Gt) + qp * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                split3_pair(rt[0][e], rt[1][e], a_, b_, c_);
                unsigned char* dst = tb + (d0 + e) * AB_TROW;
                *reinterpret_cast<unsigned*>(dst) = a_;
                *reinterpret_cast<unsigned*>(dst + AB_TPL) = b_;
                *reinterpret_cast<unsigned*>(dst + 2 * AB_TPL) = c_;
            }
        }
        if (tid < 32) { lse_s[tid] = rl; del_s[tid] = rd; }
        __syncthreads();                                    // barrier A
        if (qt + 1 < nq) fetch(q0 + 32);

        // ---- S[q][kv] and dP[q][kv]: A = Q / dO planes (lane -> query row), B = K^T / V^T register planes
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned char* qr = Qk + li * AB_KROW + u * 32 + lh * 16;
            const unsigned char* gr = Gk + li * AB_KROW + u * 32 + lh * 16;
            const bf16x8 q0_ = *reinterpret_cast<const bf16x8*>(qr), q1_ = *reinterpret_cast<const bf16x8*>(qr + AB_KPL), q2_ = *reinterpret_cast<const bf16x8*>(qr + 2 * AB_KPL);
            const bf16x8 g0_ = *reinterpret_cast<const bf16x8*>(gr), g1_ = *reinterpret_cast<const bf16x8*>(gr + AB_KPL), g2_ = *reinterpret_cast<const bf16x8*>(gr + 2 * AB_KPL);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q2_, kf[0][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g2_, vf[0][u], dp, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q0_, kf[2][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g0_, vf[2][u], dp, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q1_, kf[1][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g1_, vf[1][u], dp, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q1_, kf[0][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g1_, vf[0][u], dp, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q0_, kf[1][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g0_, vf[1][u], dp, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q0_, kf[0][u], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g0_, vf[0][u], dp, 0, 0, 0);
        }
        // ---- P = exp(S*scale - lse), dS = P * (dP - delta)   (rows q = crow(r,lh), column kv = li)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = crow(r, lh);
            float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse_s[qr]));
            if (!kv_ok) pv = 0.f;
            s[r] = pv;
            dp[r] = pv * (dp[r] - del_s[qr]);
        }
        // ---- dV^T[d][kv] += dO^T[d][q] P[q][kv] ; dK^T[d][kv] += Q^T[d][q] dS[q][kv]: the k-slots of step u are the lane's own
        // registers r = 8u .. 8u+7 (queries 16u + 4hi + {0..3, 8..11}); A from the transposed planes (two 8-byte reads each)
        // this q tile's dV^T / dK^T contributions start from zero on the matrix pipe and join the running sums on the vector pipe
        // (the bf16 MFMA does not round its accumulator to nearest: S / 32 tiles of same-signed increments would drift)
        f32x16 dvt, dkt;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dvt[r] = 0.f; dkt[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            u32x4 ph, pm, pl, sh, sm, sl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_, c_;
                split3_pair(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], a_, b_, c_); ph[e] = a_; pm[e] = b_; pl[e] = c_;
                split3_pair(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], a_, b_, c_); sh[e] = a_; sm[e] = b_; sl[e] = c_;
            }
            const bf16x8 p0 = __builtin_bit_cast(bf16x8, ph), p1 = __builtin_bit_cast(bf16x8, pm), p2 = __builtin_bit_cast(bf16x8, pl);
            const bf16x8 d0 = __builtin_bit_cast(bf16x8, sh), d1 = __builtin_bit_cast(bf16x8, sm), d2 = __builtin_bit_cast(bf16x8, sl);
            const unsigned char* gr = Gt + li * AB_TROW + (16 * u + 4 * lh) * 2;
            const unsigned char* qr = Qt + li * AB_TROW + (16 * u + 4 * lh) * 2;
            bf16x8 ga[3], qa[3];
#pragma unroll
            for (int pl_ = 0; pl_ < 3; ++pl_) {
                const u32x2 g_lo = *reinterpret_cast<const u32x2*>(gr + pl_ * AB_TPL), g_hi = *reinterpret_cast<const u32x2*>(gr + pl_ * AB_TPL + 16);
                const u32x2 q_lo = *reinterpret_cast<const u32x2*>(qr + pl_ * AB_TPL), q_hi = *reinterpret_cast<const u32x2*>(qr + pl_ * AB_TPL + 16);
                ga[pl_] = __builtin_bit_cast(bf16x8, u32x4{g_lo[0], g_lo[1], g_hi[0], g_hi[1]});
                qa[pl_] = __builtin_bit_cast(bf16x8, u32x4{q_lo[0], q_lo[1], q_hi[0], q_hi[1]});
            }
            dvt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[2], p0, dvt, 0, 0, 0);
            dkt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[2], d0, dkt, 0, 0, 0);
            dvt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[0], p2, dvt, 0, 0, 0);
            dkt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[0], d2, dkt, 0, 0, 0);
            dvt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[1], p1, dvt, 0, 0, 0);
            dkt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[1], d1, dkt, 0, 0, 0);
            dvt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[1], p0, dvt, 0, 0, 0);
            dkt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[1], d0, dkt, 0, 0, 0);
            dvt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[0], p1, dvt, 0, 0, 0);
            dkt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[0], d1, dkt, 0, 0, 0);
            dvt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[0], p0, dvt, 0, 0, 0);
            dkt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[0], d0, dkt, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) { dvacc[r] += dvt[r]; dkacc[r] += dkt[r]; }
        // ---- dQ[q][d] partial = sum_kv dS[q][kv] K[kv][d] on the fp32 MFMA: dS through wave-private LDS to flip lanes
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[crow(r, lh) * 33 + li] = dp[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x16 dq;
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[r] = 0.f;
        float sa[16];
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) sa[t16] = Smine[li * 33 + t16 + 16 * lh];
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16)
            dq = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[t16], Kmine[(t16 + 16 * lh) * 32 + li], dq, 0, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                     // every lane has read its dS row before the tile is overwritten
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int r = 0; r < 16; ++r) Pmine[crow(r, lh) * 32 + li] = dq[r];
        __syncthreads();                                    // barrier B
        for (int t = tid; t < 32 * DP; t += 256) {
            const int row = t / DP;
            if (q0 + row < p.S)
                part[(long)(q0 + row) * DP + (t % DP)] = (Sw[t] + Sw[32 * 33 + t]) + (Sw[2 * 32 * 33 + t] + Sw[3 * 32 * 33 + t]);
        }
    }
    // ---- epilogue: dK^T, dV^T -> [kv][d] through wave-private LDS, coalesced row stores (per QUERY head h)
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[li * 33 + crow(r, lh)] = (pass == 0 ? dkacc[r] * p.scale : dvacc[r]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int rr = lh; rr < 32; rr += 2) {
            const int kv = kv0 + rr;
            if (kv < p.S) {
                if (pass == 0) p.dk[((long)b * p.S + kv) * p.lddk + (long)h * 32 + li] = Smine[rr * 33 + li];
                else           p.dv[((long)b * p.S + kv) * p.lddv + (long)h * 32 + li] = Smine[rr * 33 + li];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---------------------------------------------------------------------------------------------
// backward for 32 < head_dim <= 64 on the bf16 matrix pipe (DH = 64; head_dim % 4 == 0, columns past head_dim zero-filled):
// the 4-wave kernel above with four 16-wide d steps per score, two 32-row tiles of dK^T / dV^T / dQ, one workgroup per CU
// (120 KB of LDS, ~320 registers).  Same staging roles, same fixed-order dQ reduction over the wave partials.
// ---------------------------------------------------------------------------------------------
// PP / OP: pieces of P / dS and of the Q / K / V / dO operands, as in attn_bwd_split8_kernel (the dQ product stays on the fp32 MFMA)
// F16 (with PP = OP = 2): fp16 pieces of the scaled operands, as attn_bwd_split8_kernel
template <int DH, int PP = 3, int OP = 3, bool F16 = false>
__global__ __launch_bounds__(256, 1) void attn_bwd_split_dh_kernel(const AttnArgs p) {
    constexpr int NU = DH / 16, NDT = DH / 32, CPR = DH / 4;
    constexpr int KROW = DH * 2 + 16, KPL = 32 * KROW;             // k-major planes [32 q][DH d]
    constexpr int TPL = DH * AB_TROW;                              // transposed planes [DH d][32 q]
    constexpr int NKI = 32 * CPR / 256;                            // k-major float4 items per thread and tensor (2)
    constexpr int NTI = 16 * CPR / 256 * 2;                        // transposed items per thread: (Q, dO) x ... (see below)
    static_assert(DH == 64, "attn_bwd_split_dh_kernel: DH = 64");
    constexpr int SWF = 32 * DH > 32 * 33 ? 32 * DH : 32 * 33;     // floats per wave of the dS^T staging / dQ partial tile
    // two-piece mode: the dQ product runs on the bf16 pipe too -- the wave's K rows as two bf16 planes [32 kv][DH] (row stride KPROW) in
    // place of the fp32 tile, dS^T as two planes [kv][32 q] in the staging region, both read through transposing LDS reads
    constexpr bool DQ16 = PP == 2 && OP == 2;
    constexpr int KPROW = DH * 2 + 16, KPPL = 32 * KPROW;
    constexpr int KWB = DQ16 ? (2 * KPPL > 32 * DH * 4 ? 2 * KPPL : 32 * DH * 4) : 32 * DH * 4;      // bytes per wave
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 3 * KPL + 2 * 3 * TPL + 64 * 4 + 4 * KWB + 4 * SWF * 4];
    unsigned char* Qk = smem;
    unsigned char* Gk = Qk + 3 * KPL;
    unsigned char* Qt = Gk + 3 * KPL;
    unsigned char* Gt = Qt + 3 * TPL;
    float* lse_s = reinterpret_cast<float*>(Gt + 3 * TPL);
    float* del_s = lse_s + 32;
    float* Kw = del_s + 32;                         // per wave fp32 K tile [32][DH] (dQ product), or its two bf16 planes
    float* Sw = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(Kw) + 4 * KWB);   // per wave dS^T staging; reused as the wave's dQ partial [32][DH]
    (void)NTI;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, kblk;
    xcd_group_decode(blockIdx.x, p.B * p.H, p.n_kblocks, bh, kblk);
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int kv0 = kblk * 128 + wave * 32;
    const int D = p.D;
    static_assert(!F16 || (PP == 2 && OP == 2), "fp16 pieces come in twos");
    float sc_in = 1.f, so_in = 1.f, sc_g = 1.f, so_g = 1.f;
    if (F16) { amax_scale(p.qkv_amax, sc_in, so_in); amax_scale(p.dout_amax, sc_g, so_g); }
    const float c = p.scale * LOG2E * so_in * so_in;
    const float dp_inv = so_g * so_in, dv_inv = F16 ? so_g * P_INV : 1.f;
    float* Kmine = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(Kw) + wave * KWB);
    unsigned char* Kpl = reinterpret_cast<unsigned char*>(Kmine);
    float* Smine = Sw + wave * SWF;
    float* Pmine = Smine;

    // K^T / V^T as split B operands: lane (kv = li, hi) holds d = 16u + 8hi + e
    bf16x8 kf[3][NU], vf[3][NU];
    const bool kv_ok = kv0 + li < p.S;
    {
        const float* krow = p.k + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldk + (long)hk * D;
        const float* vrow = p.v + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldv + (long)hk * D;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const f32x4 a0 = load4(krow, 16 * u + 8 * lh, D, true, true), a1 = load4(krow, 16 * u + 8 * lh + 4, D, true, true);
            const f32x4 w0 = load4(vrow, 16 * u + 8 * lh, D, true, true), w1 = load4(vrow, 16 * u + 8 * lh + 4, D, true, true);
            u32x4 ph, pm, pl, vh, vm, vl;
            unsigned a_, b_, c_;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                split_op<OP, F16>(a0[2 * e], a0[2 * e + 1], a_, b_, c_, sc_in); ph[e] = a_; pm[e] = b_; pl[e] = c_;
                split_op<OP, F16>(a1[2 * e], a1[2 * e + 1], a_, b_, c_, sc_in); ph[2 + e] = a_; pm[2 + e] = b_; pl[2 + e] = c_;
                split_op<OP, F16>(w0[2 * e], w0[2 * e + 1], a_, b_, c_, sc_in); vh[e] = a_; vm[e] = b_; vl[e] = c_;
                split_op<OP, F16>(w1[2 * e], w1[2 * e + 1], a_, b_, c_, sc_in); vh[2 + e] = a_; vm[2 + e] = b_; vl[2 + e] = c_;
            }
            kf[0][u] = __builtin_bit_cast(bf16x8, ph); kf[1][u] = __builtin_bit_cast(bf16x8, pm); kf[2][u] = __builtin_bit_cast(bf16x8, pl);
            vf[0][u] = __builtin_bit_cast(bf16x8, vh); vf[1][u] = __builtin_bit_cast(bf16x8, vm); vf[2][u] = __builtin_bit_cast(bf16x8, vl);
        }
        // the wave's K tile, row-major, for the dQ product: fp32, or two rounded bf16 planes
        for (int t = lane; t < 32 * CPR; t += 64) {
            const int row = t / CPR, d = (t % CPR) * 4;
            const f32x4 a = load4(p.k + ((long)b * p.S + min(kv0 + row, p.S - 1)) * p.ldk + (long)hk * D, d, D, kv0 + row < p.S, true);
            if (DQ16) {
                unsigned h0, m0, h1, m1;
                if (F16) { split2h_pair_gemm(a[0], a[1], sc_in, h0, m0); split2h_pair_gemm(a[2], a[3], sc_in, h1, m1); }
                else { split2_pair(a[0], a[1], h0, m0); split2_pair(a[2], a[3], h1, m1); }
                *reinterpret_cast<u32x2*>(Kpl + row * KPROW + d * 2) = u32x2{h0, h1};
                *reinterpret_cast<u32x2*>(Kpl + KPPL + row * KPROW + d * 2) = u32x2{m0, m1};
            } else *reinterpret_cast<f32x4*>(Kmine + row * DH + d) = a;
        }
    }
    f32x16 dvacc[NDT], dkacc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dvacc[dt][r] = 0.f; dkacc[dt][r] = 0.f; }

    const float* qbase = p.q + (long)b * p.S * p.ldq + (long)h * D;
    const float* gbase = p.dout + (long)b * p.S * p.ldo + (long)h * D;
    const float* lse_b = p.lse + ((long)b * p.H + h) * p.S;
    const float* del_b = p.delta + ((long)b * p.H + h) * p.S;
    // prefetch registers.  k-major pieces: item idx = tid + 256 i -> (row = idx / CPR, chunk = idx % CPR) of Q and of dO.
    // transposed pieces: item (qp = tid / CPR, chunk = tid % CPR) -> rows (2qp, 2qp+1), of Q and of dO (every thread does both).
    f32x4 rq[NKI], rg[NKI], rtq[2], rtg[2];
    float rl = 0.f, rd = 0.f;
    auto fetch = [&](int q0) {
#pragma unroll
        for (int i = 0; i < NKI; ++i) {
            const int idx = tid + 256 * i, row = idx / CPR, d = (idx % CPR) * 4;
            const bool ok = q0 + row < p.S;
            const long r = min(q0 + row, p.S - 1);
            rq[i] = load4(qbase + r * p.ldq, d, D, ok, true);
            rg[i] = load4(gbase + r * p.ldo, d, D, ok, true);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = 2 * (tid / CPR) + i, d = (tid % CPR) * 4;
            const bool ok = q0 + row < p.S;
            const long r = min(q0 + row, p.S - 1);
            rtq[i] = load4(qbase + r * p.ldq, d, D, ok, true);
            rtg[i] = load4(gbase + r * p.ldo, d, D, ok, true);
        }
        if (tid < 32) {
            const bool ok = q0 + tid < p.S;
            rl = ok ? lse_b[q0 + tid] * LOG2E : INFINITY;   // +inf -> P = 0 for padded queries
            rd = ok ? del_b[q0 + tid] : 0.f;
        }
    };
    const int nq = (p.S + 31) / 32;
    const long part_stride = (long)p.B * p.H * p.S * DH;
    float* part = p.dq_part + (long)kblk * part_stride + ((long)b * p.H + h) * p.S * DH;

    fetch(0);
    for (int qt = 0; qt < nq; ++qt) {
        const int q0 = qt * 32;
        // ---- stage the tile as split planes, both orientations
        {
            unsigned a_, b_, c_;
#pragma unroll
            for (int i = 0; i < NKI; ++i) {
                const int idx = tid + 256 * i, row = idx / CPR, ch = idx % CPR;
                u32x2 h2, m2, l2;
                split_op<OP, F16>(rq[i][0], rq[i][1], a_, b_, c_, sc_in); h2[0] = a_; m2[0] = b_; l2[0] = c_;
                split_op<OP, F16>(rq[i][2], rq[i][3], a_, b_, c_, sc_in); h2[1] = a_; m2[1] = b_; l2[1] = c_;
                unsigned char* dq_ = Qk + row * KROW + ch * 8;
                *reinterpret_cast<u32x2*>(dq_) = h2; *reinterpret_cast<u32x2*>(dq_ + KPL) = m2;
                if (OP == 3) *reinterpret_cast<u32x2*>(dq_ + 2 * KPL) = l2;
                split_op<OP, F16>(rg[i][0], rg[i][1], a_, b_, c_, sc_g); h2[0] = a_; m2[0] = b_; l2[0] = c_;
                split_op<OP, F16>(rg[i][2], rg[i][3], a_, b_, c_, sc_g); h2[1] = a_; m2[1] = b_; l2[1] = c_;
                unsigned char* dg_ = Gk + row * KROW + ch * 8;
                *reinterpret_cast<u32x2*>(dg_) = h2; *reinterpret_cast<u32x2*>(dg_ + KPL) = m2;
                if (OP == 3) *reinterpret_cast<u32x2*>(dg_ + 2 * KPL) = l2;
            }
            // transposed: (q = 2qp, 2qp+1) pairs of this thread's 4 d columns, for Q and for dO
            const int qp = tid / CPR, d0 = (tid % CPR) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                split_op<OP, F16>(rtq[0][e], rtq[1][e], a_, b_, c_, sc_in);
                unsigned char* dst = Qt + (d0 + e) * AB_TROW + qp * 4;
                *reinterpret_cast<unsigned*>(dst) = a_;
                *reinterpret_cast<unsigned*>(dst + TPL) = b_;
                if (OP == 3) *reinterpret_cast<unsigned*>(dst + 2 * TPL) = c_;
                split_op<OP, F16>(rtg[0][e], rtg[1][e], a_, b_, c_, sc_g);
                dst = Gt + (d0 + e) * AB_TROW + qp * 4;
                *reinterpret_cast<unsigned*>(dst) = a_;
                *reinterpret_cast<unsigned*>(dst + TPL) = b_;
                if (OP == 3) *reinterpret_cast<unsigned*>(dst + 2 * TPL) = c_;
            }
        }
        if (tid < 32) { lse_s[tid] = rl; del_s[tid] = rd; }
        __syncthreads();                                    // barrier A
        if (qt + 1 < nq) fetch(q0 + 32);

        // ---- S[q][kv] and dP[q][kv]: A = Q / dO planes (lane -> query row), B = K^T / V^T register planes
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const unsigned char* qr = Qk + li * KROW + u * 32 + lh * 16;
            const unsigned char* gr = Gk + li * KROW + u * 32 + lh * 16;
            const bf16x8 q0_ = *reinterpret_cast<const bf16x8*>(qr), q1_ = *reinterpret_cast<const bf16x8*>(qr + KPL);
            const bf16x8 g0_ = *reinterpret_cast<const bf16x8*>(gr), g1_ = *reinterpret_cast<const bf16x8*>(gr + KPL);
            if (OP == 3) {
                const bf16x8 q2_ = *reinterpret_cast<const bf16x8*>(qr + 2 * KPL), g2_ = *reinterpret_cast<const bf16x8*>(gr + 2 * KPL);
                s = mfma16<F16>(q2_, kf[0][u], s);
                dp = mfma16<F16>(g2_, vf[0][u], dp);
                s = mfma16<F16>(q0_, kf[2][u], s);
                dp = mfma16<F16>(g0_, vf[2][u], dp);
                s = mfma16<F16>(q1_, kf[1][u], s);
                dp = mfma16<F16>(g1_, vf[1][u], dp);
            }
            s = mfma16<F16>(q1_, kf[0][u], s);
            dp = mfma16<F16>(g1_, vf[0][u], dp);
            s = mfma16<F16>(q0_, kf[1][u], s);
            dp = mfma16<F16>(g0_, vf[1][u], dp);
            s = mfma16<F16>(q0_, kf[0][u], s);
            dp = mfma16<F16>(g0_, vf[0][u], dp);
        }
        // ---- P = exp(S*scale - lse), dS = P * (dP - delta)   (rows q = crow(r,lh), column kv = li)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = crow(r, lh);
            float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse_s[qr]));
            if (!kv_ok) pv = 0.f;
            s[r] = pv;
            dp[r] = F16 ? pv * fmaf(dp[r], dp_inv, -del_s[qr]) : pv * (dp[r] - del_s[qr]);
        }
        float sc_ds = 1.f, ds_inv = 1.f;          // fp16 pieces: the tile's own power-of-two scale for dS (attn_bwd_split8_kernel)
        if (F16) {
            float mx = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fabsf(dp[r]));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            pow2_scale(mx, sc_ds, ds_inv);
        }
        const float dk_inv = ds_inv * so_in;
        // ---- dV^T[d][kv] += dO^T[d][q] P[q][kv] ; dK^T[d][kv] += Q^T[d][q] dS[q][kv]: the k-slots of step u are the lane's own
        // registers r = 8u .. 8u+7 (queries 16u + 4hi + {0..3, 8..11}); A from the transposed planes (two 8-byte reads each)
        // this q tile's dV^T / dK^T contributions start from zero on the matrix pipe and join the running sums on the vector pipe
        // (the bf16 MFMA does not round its accumulator to nearest: S / 32 tiles of same-signed increments would drift)
        f32x16 dvt[NDT], dkt[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dvt[dt][r] = 0.f; dkt[dt][r] = 0.f; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            u32x4 ph, pm, pl, sh, sm, sl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_, c_;
                split_op<PP, F16>(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], a_, b_, c_, P_SCALE); ph[e] = a_; pm[e] = b_; pl[e] = c_;
                split_op<PP, F16>(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], a_, b_, c_, sc_ds); sh[e] = a_; sm[e] = b_; sl[e] = c_;
            }
            const bf16x8 p0 = __builtin_bit_cast(bf16x8, ph), p1 = __builtin_bit_cast(bf16x8, pm), p2 = __builtin_bit_cast(bf16x8, pl);
            const bf16x8 d0 = __builtin_bit_cast(bf16x8, sh), d1 = __builtin_bit_cast(bf16x8, sm), d2 = __builtin_bit_cast(bf16x8, sl);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const unsigned char* gr = Gt + (32 * dt + li) * AB_TROW + (16 * u + 4 * lh) * 2;
                const unsigned char* qr = Qt + (32 * dt + li) * AB_TROW + (16 * u + 4 * lh) * 2;
                bf16x8 ga[3], qa[3];
#pragma unroll
                for (int pl_ = 0; pl_ < OP; ++pl_) {
                    const u32x2 g_lo = *reinterpret_cast<const u32x2*>(gr + pl_ * TPL), g_hi = *reinterpret_cast<const u32x2*>(gr + pl_ * TPL + 16);
                    const u32x2 q_lo = *reinterpret_cast<const u32x2*>(qr + pl_ * TPL), q_hi = *reinterpret_cast<const u32x2*>(qr + pl_ * TPL + 16);
                    ga[pl_] = __builtin_bit_cast(bf16x8, u32x4{g_lo[0], g_lo[1], g_hi[0], g_hi[1]});
                    qa[pl_] = __builtin_bit_cast(bf16x8, u32x4{q_lo[0], q_lo[1], q_hi[0], q_hi[1]});
                }
                if (OP == 3) {
                    dvt[dt] = mfma16<F16>(ga[2], p0, dvt[dt]);
                    dkt[dt] = mfma16<F16>(qa[2], d0, dkt[dt]);
                }
                if (PP == 3) {
                    dvt[dt] = mfma16<F16>(ga[0], p2, dvt[dt]);
                    dkt[dt] = mfma16<F16>(qa[0], d2, dkt[dt]);
                }
                if (OP == 3 || PP == 3) {
                    dvt[dt] = mfma16<F16>(ga[1], p1, dvt[dt]);
                    dkt[dt] = mfma16<F16>(qa[1], d1, dkt[dt]);
                }
                dvt[dt] = mfma16<F16>(ga[1], p0, dvt[dt]);
                dkt[dt] = mfma16<F16>(qa[1], d0, dkt[dt]);
                dvt[dt] = mfma16<F16>(ga[0], p1, dvt[dt]);
                dkt[dt] = mfma16<F16>(qa[0], d1, dkt[dt]);
                dvt[dt] = mfma16<F16>(ga[0], p0, dvt[dt]);
                dkt[dt] = mfma16<F16>(qa[0], d0, dkt[dt]);
            }
        }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dvacc[dt][r] = F16 ? fmaf(dvt[dt][r], dv_inv, dvacc[dt][r]) : dvacc[dt][r] + dvt[dt][r];
                dkacc[dt][r] = F16 ? fmaf(dkt[dt][r], dk_inv, dkacc[dt][r]) : dkacc[dt][r] + dkt[dt][r];
            }
        // ---- dQ[q][d] partial = sum_kv dS[q][kv] K[kv][d]: dS through wave-private LDS to flip lanes
        f32x16 dq[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
        if (DQ16) {
            // dS^T pieces [kv = li][q] (the pieces the dK product has just formed are gone: re-split, 8 pairs), 8-byte stores; both operands come
            // back through transposing reads: k-slot e = key 16u + 8 (e >> 2) + 4 hi + (e & 3)
            unsigned char* dSp = reinterpret_cast<unsigned char*>(Smine);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                unsigned h_[4], m_[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (F16) split2h_pair_gemm(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], sc_ds, h_[e], m_[e]);
                    else split2_pair(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], h_[e], m_[e]);
                }
                unsigned char* dst = dSp + li * AB_KROW + (16 * u + 4 * lh) * 2;
                *reinterpret_cast<u32x2*>(dst) = u32x2{h_[0], h_[1]};
                *reinterpret_cast<u32x2*>(dst + 16) = u32x2{h_[2], h_[3]};
                *reinterpret_cast<u32x2*>(dst + AB_KPL) = u32x2{m_[0], m_[1]};
                *reinterpret_cast<u32x2*>(dst + AB_KPL + 16) = u32x2{m_[2], m_[3]};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int tr_s = lds_tr_lane_offset(lane, AB_KROW), tr_k = lds_tr_lane_offset(lane, KPROW);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                bf16x8 da[2];
#pragma unroll
                for (int pl_ = 0; pl_ < 2; ++pl_)
                    da[pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(dSp + pl_ * AB_KPL + (16 * u) * AB_KROW + tr_s), lds_tr(dSp + pl_ * AB_KPL + (16 * u + 8) * AB_KROW + tr_s)));
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    bf16x8 kb[2];
#pragma unroll
                    for (int pl_ = 0; pl_ < 2; ++pl_)
                        kb[pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(Kpl + pl_ * KPPL + (16 * u) * KPROW + 32 * dt * 2 + tr_k),
                                                                   lds_tr(Kpl + pl_ * KPPL + (16 * u + 8) * KPROW + 32 * dt * 2 + tr_k)));
                    dq[dt] = mfma16<F16>(da[1], kb[0], dq[dt]);
                    dq[dt] = mfma16<F16>(da[0], kb[1], dq[dt]);
                    dq[dt] = mfma16<F16>(da[0], kb[0], dq[dt]);
                }
            }
        } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[crow(r, lh) * 33 + li] = dp[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float sa[16];
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) sa[t16] = Smine[li * 33 + t16 + 16 * lh];
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
                dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[t16], Kmine[(t16 + 16 * lh) * DH + 32 * dt + li], dq[dt], 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                     // every lane has read its dS row before the tile is overwritten
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) Pmine[crow(r, lh) * DH + 32 * dt + li] = F16 ? dq[dt][r] * dk_inv : dq[dt][r];
        __syncthreads();                                    // barrier B
        for (int t = tid; t < 32 * DH; t += 256) {
            const int row = t / DH;
            if (q0 + row < p.S)
                part[(long)(q0 + row) * DH + (t % DH)] = (Sw[t] + Sw[SWF + t]) + (Sw[2 * SWF + t] + Sw[3 * SWF + t]);
        }
    }
    // ---- epilogue: dK^T, dV^T -> [kv][d] through wave-private LDS, coalesced row stores (per QUERY head h)
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 2 * NDT; ++pass) {
        const int dt = pass >> 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[li * 33 + crow(r, lh)] = ((pass & 1) == 0 ? dkacc[dt][r] * p.scale : dvacc[dt][r]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int rr = lh; rr < 32; rr += 2) {
            const int kv = kv0 + rr;
            if (kv < p.S && 32 * dt + li < D) {
                if ((pass & 1) == 0) p.dk[((long)b * p.S + kv) * p.lddk + (long)h * D + 32 * dt + li] = Smine[rr * 33 + li];
                else                 p.dv[((long)b * p.S + kv) * p.lddv + (long)h * D + 32 * dt + li] = Smine[rr * 33 + li];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---------------------------------------------------------------------------------------------
// backward, 8 waves x 32 keys = 256 keys per workgroup (one workgroup per CU): the Q / dO tile is staged once per 256 keys,
// the dQ slabs halve, and with 150 KB of LDS per workgroup the dQ product moves onto the bf16 pipe as well: dS is written as
// three bf16 planes [q][kv] (2-byte stores straight from the packed split registers), K^T planes [d][kv] are built once per
// wave, dQ = dS K is six bf16 piece products like the other four.
// ---------------------------------------------------------------------------------------------
constexpr int AB8_SHARED = 2 * 3 * AB_KPL + 2 * 3 * AB_TPL + 64 * 4;          // Q / dO planes (both orientations) + lse / delta
constexpr int AB8_WAVE = 2 * 3 * AB_KPL;                                        // K^T planes + dS planes (dQ partial aliases dS)
constexpr int AB8_LDS = AB8_SHARED + 8 * AB8_WAVE;

// PP = pieces of P and of dS = P (dP - delta) in the dV, dK and dQ products (3: exact split, 2: split2_pair, see the forward)
// TR: the dO^T / Q^T operands of dV / dK and the dS operand of dQ come through TRANSPOSING LDS reads (common.h lds_tr) instead of
// separately staged transposed planes: no second (transposed) copy of the Q / dO tile is loaded, split and written per q tile, and dS goes
// to LDS as [kv][q] with 8-byte stores (a lane's four consecutive queries) instead of [q][kv] with 2-byte ones (8 stores per tile and
// wave instead of 64)
// F16 (with PP = OP = 2, TR): two fp16 pieces of the scaled operands -- Q, K, V by the power of two from the qkv magnitude word, dO by its
// own word, P by 2^15, dS by a per-tile power of two from the wave's own maximum (the tile products join the running sums on the vector
// pipe anyway: the inverse scales ride that fused multiply-add) -- three piece products per k-step on the f16 MFMA.  (P by 2^13, see P_SCALE.)
// QS = 2: the query tiles of a 256-key block are shared between TWO workgroups (first half / second half of the sequence) -- batches that give
// only 128 .. 255 workgroups (4 x 1 024 tokens x 8 heads: BASELINE configs[3]'s per-GPU shape) fill the chip again.  The dQ slabs do not
// change (a query tile's slab row is still written by exactly one workgroup per key block); the first half writes its dK / dV where they
// belong, the second half into two spare dQ slabs of the workspace (it is sized for 128-key blocks, this kernel uses 256-key ones), and a
// small kernel adds them: dK = first + second in that order, no atomics.  (The first form added both halves by atomics into zeroed memory:
// bit-reproducible on one box, but the SAME training run ended at 0.7481867 on one box and 0.7482677 on another -- wherever two float
// atomics meet, the sum is not the same number on every chip.)
template <int PP = 3, int OP = 3, bool TR = false, bool F16 = false, int QS = 1>
__global__ __launch_bounds__(512, 1) void attn_bwd_split8_kernel(const AttnArgs p) {
    constexpr int DP = 32, NW = 8;
    __shared__ __attribute__((aligned(16))) unsigned char smem[AB8_LDS];
    unsigned char* Qk = smem;
    unsigned char* Gk = Qk + 3 * AB_KPL;
    unsigned char* Qt = Gk + 3 * AB_KPL;
    unsigned char* Gt = Qt + 3 * AB_TPL;
    float* lse_s = reinterpret_cast<float*>(Gt + 3 * AB_TPL);
    float* del_s = lse_s + 32;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, kblk, qhalf = 0;
    xcd_group_decode(blockIdx.x, p.B * p.H, p.n_kblocks * QS, bh, kblk);
    if (QS > 1) { qhalf = kblk % QS; kblk /= QS; }
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int kv0 = kblk * 256 + wave * 32;
    static_assert(!F16 || (PP == 2 && OP == 2), "fp16 pieces come in twos");
    // this wave's K / V rows are requested first, then both magnitude words, and only then does anything wait: one round trip at the head of
    // the workgroup's life instead of three
    f32x4 kraw[2][2], vraw[2][2];
    {
        const float* krow = p.k + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldk + (long)hk * 32;
        const float* vrow = p.v + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldv + (long)hk * 32;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            kraw[u][0] = *reinterpret_cast<const f32x4*>(krow + 16 * u + 8 * lh); kraw[u][1] = *reinterpret_cast<const f32x4*>(krow + 16 * u + 8 * lh + 4);
            vraw[u][0] = *reinterpret_cast<const f32x4*>(vrow + 16 * u + 8 * lh); vraw[u][1] = *reinterpret_cast<const f32x4*>(vrow + 16 * u + 8 * lh + 4);
        }
    }
    float sc_in = 1.f, so_in = 1.f, sc_g = 1.f, so_g = 1.f;
    if (F16) {
        const unsigned w_in = amax_peek(p.qkv_amax), w_g = amax_peek(p.dout_amax);
        amax_finish(w_in, sc_in, so_in);
        amax_finish(w_g, sc_g, so_g);
    }
    const float c = p.scale * LOG2E * so_in * so_in;         // scores arrive scaled by sc_in^2
    const float dp_inv = so_g * so_in;                       // dO V^T arrives scaled by sc_g * sc_in
    const float dv_inv = F16 ? so_g * P_INV : 1.f;           // dO^T P by sc_g * 2^15
    unsigned char* Ktp = smem + AB8_SHARED + wave * AB8_WAVE;        // 3 planes [d][32 kv]
    unsigned char* dSp = Ktp + 3 * AB_KPL;                           // 3 planes [q][32 kv]
    float* Pmine = reinterpret_cast<float*>(dSp);                    // [32 q][32 d] fp32 after the dQ MFMAs
    const int tr_off = lds_tr_lane_offset(lane, AB_KROW);

    bf16x8 kf[3][2], vf[3][2];
    const bool kv_ok = kv0 + li < p.S;
    {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 a0 = kraw[u][0], a1 = kraw[u][1];
            const f32x4 w0 = vraw[u][0], w1 = vraw[u][1];
            u32x4 ph, pm, pl, vh, vm, vl;
            unsigned a_, b_, c_;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                split_op<OP, F16>(a0[2 * e], a0[2 * e + 1], a_, b_, c_, sc_in); ph[e] = a_; pm[e] = b_; pl[e] = c_;
                split_op<OP, F16>(a1[2 * e], a1[2 * e + 1], a_, b_, c_, sc_in); ph[2 + e] = a_; pm[2 + e] = b_; pl[2 + e] = c_;
                split_op<OP, F16>(w0[2 * e], w0[2 * e + 1], a_, b_, c_, sc_in); vh[e] = a_; vm[e] = b_; vl[e] = c_;
                split_op<OP, F16>(w1[2 * e], w1[2 * e + 1], a_, b_, c_, sc_in); vh[2 + e] = a_; vm[2 + e] = b_; vl[2 + e] = c_;
            }
            kf[0][u] = __builtin_bit_cast(bf16x8, ph); kf[1][u] = __builtin_bit_cast(bf16x8, pm); kf[2][u] = __builtin_bit_cast(bf16x8, pl);
            vf[0][u] = __builtin_bit_cast(bf16x8, vh); vf[1][u] = __builtin_bit_cast(bf16x8, vm); vf[2][u] = __builtin_bit_cast(bf16x8, vl);
        }
        // K^T planes of this wave's 32 keys: item (key pair kp, 4-d chunk ch), two items per lane
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int item = lane + 64 * it, kp = item >> 3, d0 = (item & 7) * 4;
            f32x4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0;
            if (kv0 + 2 * kp < p.S) r0 = *reinterpret_cast<const f32x4*>(p.k + ((long)b * p.S + kv0 + 2 * kp) * p.ldk + (long)hk * 32 + d0);
            if (kv0 + 2 * kp + 1 < p.S) r1 = *reinterpret_cast<const f32x4*>(p.k + ((long)b * p.S + kv0 + 2 * kp + 1) * p.ldk + (long)hk * 32 + d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_, c_;
                split_op<OP, F16>(r0[e], r1[e], a_, b_, c_, sc_in);
                unsigned char* dst = Ktp + (d0 + e) * AB_KROW + kp * 4;
                *reinterpret_cast<unsigned*>(dst) = a_;
                *reinterpret_cast<unsigned*>(dst + AB_KPL) = b_;
                if (OP == 3) *reinterpret_cast<unsigned*>(dst + 2 * AB_KPL) = c_;
            }
        }
    }
    f32x16 dvacc, dkacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dvacc[r] = 0.f; dkacc[r] = 0.f; }

    const float* qbase = p.q + (long)b * p.S * p.ldq + (long)h * 32;
    const float* gbase = p.dout + (long)b * p.S * p.ldo + (long)h * 32;
    const float* lse_b = p.lse + ((long)b * p.H + h) * p.S;
    const float* del_b = p.delta + ((long)b * p.H + h) * p.S;
    // staging roles: kind = tid >> 8 (0: Q, 1: dO); k-major piece (row = (tid & 255) >> 3, chunk = tid & 7) for everyone;
    // transposed piece (rows 2qp, 2qp+1; qp = (tid & 127) >> 3) for the threads with (tid & 255) < 128
    const int kind = tid >> 8, t8 = tid & 255;
    const bool tthread = t8 < 128;
    const float* sbase = kind == 0 ? qbase : gbase;
    const long sld = kind == 0 ? p.ldq : p.ldo;
    f32x4 rk1, rt[2], ro = {0.f, 0.f, 0.f, 0.f};
    float rl = 0.f, rd = 0.f;
    // F16: delta[q] = sum_d dO[q][d] O[q][d] is formed HERE from the dO tile the kind-1 threads stage anyway (+ the matching O chunk): no
    // separate delta launch, no delta array
    const float* obase = p.oin + (long)b * p.S * p.ldo + (long)h * 32;
    auto fetch = [&](int q0) {
        {
            const int row = t8 >> 3, d = (tid & 7) * 4;
            rk1 = *reinterpret_cast<const f32x4*>(sbase + (long)min(q0 + row, p.S - 1) * sld + d);
            if (q0 + row >= p.S) rk1 = f32x4{0.f, 0.f, 0.f, 0.f};
            if (F16 && kind == 1) ro = *reinterpret_cast<const f32x4*>(obase + (long)min(q0 + row, p.S - 1) * p.ldo + d);
        }
        if (!TR && tthread) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = 2 * (t8 >> 3) + i, d = (tid & 7) * 4;
                rt[i] = *reinterpret_cast<const f32x4*>(sbase + (long)min(q0 + row, p.S - 1) * sld + d);
                if (q0 + row >= p.S) rt[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        if (tid < 32) {
            const bool ok = q0 + tid < p.S;
            rl = ok ? lse_b[q0 + tid] * LOG2E : INFINITY;
            rd = (ok && !F16) ? del_b[q0 + tid] : 0.f;
        }
    };
    const int nq = (p.S + 31) / 32;
    const long part_stride = (long)p.B * p.H * p.S * DP;
    float* part = p.dq_part + (long)kblk * part_stride + ((long)b * p.H + h) * p.S * DP;

    const int nq_each = (nq + QS - 1) / QS;
    const int qt_begin = qhalf * nq_each, qt_end = min(nq, qt_begin + nq_each);
    fetch(qt_begin * 32);
    for (int qt = qt_begin; qt < qt_end; ++qt) {
        const int q0 = qt * 32;
        {
            const int row = t8 >> 3, ch = tid & 7;
            u32x2 h2, m2, l2;
            unsigned a_, b_, c_;
            const float sc_st = kind == 0 ? sc_in : sc_g;
            split_op<OP, F16>(rk1[0], rk1[1], a_, b_, c_, sc_st); h2[0] = a_; m2[0] = b_; l2[0] = c_;
            split_op<OP, F16>(rk1[2], rk1[3], a_, b_, c_, sc_st); h2[1] = a_; m2[1] = b_; l2[1] = c_;
            unsigned char* dk_ = (kind == 0 ? Qk : Gk) + row * AB_KROW + ch * 8;
            *reinterpret_cast<u32x2*>(dk_) = h2; *reinterpret_cast<u32x2*>(dk_ + AB_KPL) = m2;
            if (OP == 3) *reinterpret_cast<u32x2*>(dk_ + 2 * AB_KPL) = l2;
            if (!TR && tthread) {
                const int qp = t8 >> 3, d0 = ch * 4;
                unsigned char* tb = (kind == 0 ? Qt : Gt) + qp * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    split_op<OP, F16>(rt[0][e], rt[1][e], a_, b_, c_, sc_st);
                    unsigned char* dst = tb + (d0 + e) * AB_TROW;
                    *reinterpret_cast<unsigned*>(dst) = a_;
                    *reinterpret_cast<unsigned*>(dst + AB_TPL) = b_;
                    if (OP == 3) *reinterpret_cast<unsigned*>(dst + 2 * AB_TPL) = c_;
                }
            }
        }
        if (tid < 32) { lse_s[tid] = rl; if (!F16) del_s[tid] = rd; }
        if (F16 && kind == 1) {          // rows of the dO tile: eight consecutive lanes hold one row's 32 d
            // (explicit fused multiply-adds: left to the compiler, which products it contracts differs from one instantiation to the next)
            float dsum = fmaf(rk1[0], ro[0], fmaf(rk1[1], ro[1], fmaf(rk1[2], ro[2], rk1[3] * ro[3])));
            dsum += __shfl_xor(dsum, 1, 64); dsum += __shfl_xor(dsum, 2, 64); dsum += __shfl_xor(dsum, 4, 64);
            if ((tid & 7) == 0) del_s[t8 >> 3] = dsum;
        }
        __syncthreads();                                    // barrier A
        if (qt + 1 < qt_end) fetch(q0 + 32);

        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned char* qr = Qk + li * AB_KROW + u * 32 + lh * 16;
            const unsigned char* gr = Gk + li * AB_KROW + u * 32 + lh * 16;
            const bf16x8 q0_ = *reinterpret_cast<const bf16x8*>(qr), q1_ = *reinterpret_cast<const bf16x8*>(qr + AB_KPL);
            const bf16x8 g0_ = *reinterpret_cast<const bf16x8*>(gr), g1_ = *reinterpret_cast<const bf16x8*>(gr + AB_KPL);
            if (OP == 3) {
                const bf16x8 q2_ = *reinterpret_cast<const bf16x8*>(qr + 2 * AB_KPL), g2_ = *reinterpret_cast<const bf16x8*>(gr + 2 * AB_KPL);
                s = mfma16<F16>(q2_, kf[0][u], s);
                dp = mfma16<F16>(g2_, vf[0][u], dp);
                s = mfma16<F16>(q0_, kf[2][u], s);
                dp = mfma16<F16>(g0_, vf[2][u], dp);
                s = mfma16<F16>(q1_, kf[1][u], s);
                dp = mfma16<F16>(g1_, vf[1][u], dp);
            }
            s = mfma16<F16>(q1_, kf[0][u], s);
            dp = mfma16<F16>(g1_, vf[0][u], dp);
            s = mfma16<F16>(q0_, kf[1][u], s);
            dp = mfma16<F16>(g0_, vf[1][u], dp);
            s = mfma16<F16>(q0_, kf[0][u], s);
            dp = mfma16<F16>(g0_, vf[0][u], dp);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = crow(r, lh);
            float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse_s[qr]));
            if (!kv_ok) pv = 0.f;
            s[r] = pv;
            dp[r] = F16 ? pv * fmaf(dp[r], dp_inv, -del_s[qr]) : pv * (dp[r] - del_s[qr]);
        }
        // fp16 pieces: this tile's dS gets its own power-of-two scale from the wave's maximum (dS = P (dP - delta) spans many binades
        // below any bound known in advance); wave-uniform, undone where the tile's products join the running sums
        float sc_ds = 1.f, ds_inv = 1.f;
        if (F16) {
            float mx = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fabsf(dp[r]));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            pow2_scale(mx, sc_ds, ds_inv);
        }
        const float dk_inv = ds_inv * so_in, dq_inv = ds_inv * so_in;          // Q^T dS by sc_in * sc_ds; dS K likewise
        // this q tile's dV^T / dK^T contributions start from zero on the matrix pipe and join the running sums on the vector pipe
        // (the bf16 MFMA does not round its accumulator to nearest: S / 32 tiles of same-signed increments would drift)
        f32x16 dvt, dkt;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dvt[r] = 0.f; dkt[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            u32x4 ph, pm, pl = {0u, 0u, 0u, 0u}, sh, sm, sl = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_, c_ = 0u;
                if (PP == 3) split3_pair(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], a_, b_, c_);
                else if (F16) split2h_pair_gemm(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], P_SCALE, a_, b_);
                else split2_pair(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], a_, b_);
                ph[e] = a_; pm[e] = b_; pl[e] = c_;
                if (PP == 3) split3_pair(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], a_, b_, c_);
                else if (F16) split2h_pair_gemm(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], sc_ds, a_, b_);
                else split2_pair(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], a_, b_);
                sh[e] = a_; sm[e] = b_; sl[e] = c_;
                if (!TR) {
                // dS pieces for the dQ product: rows q = crow(8u + 2e, hi) and q + 1, column kv = li, 2-byte stores
                unsigned char* dst = dSp + crow(8 * u + 2 * e, lh) * AB_KROW + li * 2;
                *reinterpret_cast<unsigned short*>(dst) = (unsigned short)(a_ & 0xffffu);
                *reinterpret_cast<unsigned short*>(dst + AB_KROW) = (unsigned short)(a_ >> 16);
                *reinterpret_cast<unsigned short*>(dst + AB_KPL) = (unsigned short)(b_ & 0xffffu);
                *reinterpret_cast<unsigned short*>(dst + AB_KPL + AB_KROW) = (unsigned short)(b_ >> 16);
                if (PP == 3) {
                    *reinterpret_cast<unsigned short*>(dst + 2 * AB_KPL) = (unsigned short)(c_ & 0xffffu);
                    *reinterpret_cast<unsigned short*>(dst + 2 * AB_KPL + AB_KROW) = (unsigned short)(c_ >> 16);
                }
                }
            }
            if (TR) {
                // dS^T pieces [kv = li][q]: registers 8u .. 8u + 3 are queries 16u + 4hi + 0..3, 8u + 4 .. 8u + 7 the same, eight up
                unsigned char* dst = dSp + li * AB_KROW + (16 * u + 4 * lh) * 2;
                *reinterpret_cast<u32x2*>(dst) = u32x2{sh[0], sh[1]};
                *reinterpret_cast<u32x2*>(dst + 16) = u32x2{sh[2], sh[3]};
                *reinterpret_cast<u32x2*>(dst + AB_KPL) = u32x2{sm[0], sm[1]};
                *reinterpret_cast<u32x2*>(dst + AB_KPL + 16) = u32x2{sm[2], sm[3]};
                if (PP == 3) {
                    *reinterpret_cast<u32x2*>(dst + 2 * AB_KPL) = u32x2{sl[0], sl[1]};
                    *reinterpret_cast<u32x2*>(dst + 2 * AB_KPL + 16) = u32x2{sl[2], sl[3]};
                }
            }
            const bf16x8 p0 = __builtin_bit_cast(bf16x8, ph), p1 = __builtin_bit_cast(bf16x8, pm), p2 = __builtin_bit_cast(bf16x8, pl);
            const bf16x8 d0 = __builtin_bit_cast(bf16x8, sh), d1 = __builtin_bit_cast(bf16x8, sm), d2 = __builtin_bit_cast(bf16x8, sl);
            const unsigned char* gr = Gt + li * AB_TROW + (16 * u + 4 * lh) * 2;
            const unsigned char* qr = Qt + li * AB_TROW + (16 * u + 4 * lh) * 2;
            bf16x8 ga[3], qa[3];
#pragma unroll
            for (int pl_ = 0; pl_ < OP; ++pl_) {
                if (TR) {         // dO^T / Q^T fragments straight from the k-major planes [q][d]: column d = li, rows q = 16u + 4hi + 0..3 and + 8
                    ga[pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(Gk + pl_ * AB_KPL + (16 * u) * AB_KROW + tr_off), lds_tr(Gk + pl_ * AB_KPL + (16 * u + 8) * AB_KROW + tr_off)));
                    qa[pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(Qk + pl_ * AB_KPL + (16 * u) * AB_KROW + tr_off), lds_tr(Qk + pl_ * AB_KPL + (16 * u + 8) * AB_KROW + tr_off)));
                } else {
                const u32x2 g_lo = *reinterpret_cast<const u32x2*>(gr + pl_ * AB_TPL), g_hi = *reinterpret_cast<const u32x2*>(gr + pl_ * AB_TPL + 16);
                const u32x2 q_lo = *reinterpret_cast<const u32x2*>(qr + pl_ * AB_TPL), q_hi = *reinterpret_cast<const u32x2*>(qr + pl_ * AB_TPL + 16);
                ga[pl_] = __builtin_bit_cast(bf16x8, u32x4{g_lo[0], g_lo[1], g_hi[0], g_hi[1]});
                qa[pl_] = __builtin_bit_cast(bf16x8, u32x4{q_lo[0], q_lo[1], q_hi[0], q_hi[1]});
                }
            }
            if (OP == 3) {
                dvt = mfma16<F16>(ga[2], p0, dvt);
                dkt = mfma16<F16>(qa[2], d0, dkt);
            }
            if (PP == 3) {
                dvt = mfma16<F16>(ga[0], p2, dvt);
                dkt = mfma16<F16>(qa[0], d2, dkt);
            }
            if (OP == 3 || PP == 3) {
                dvt = mfma16<F16>(ga[1], p1, dvt);
                dkt = mfma16<F16>(qa[1], d1, dkt);
            }
            dvt = mfma16<F16>(ga[1], p0, dvt);
            dkt = mfma16<F16>(qa[1], d0, dkt);
            dvt = mfma16<F16>(ga[0], p1, dvt);
            dkt = mfma16<F16>(qa[0], d1, dkt);
            dvt = mfma16<F16>(ga[0], p0, dvt);
            dkt = mfma16<F16>(qa[0], d0, dkt);
        }
        // ---- dQ[q][d] partial = sum_kv dS[q][kv] K[kv][d]: A = dS planes (lane -> q), B = K^T planes (lane -> d), kv = 16u + 8hi + e
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x16 dq;
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[r] = 0.f;
        bf16x8 da[2][3], kb[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int pl_ = 0; pl_ < 3; ++pl_) {
                if (TR) {         // k-slot e = key 16u + 8 (e >> 2) + 4 hi + (e & 3) in both operands
                    if (pl_ < PP) da[u][pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(dSp + pl_ * AB_KPL + (16 * u) * AB_KROW + tr_off), lds_tr(dSp + pl_ * AB_KPL + (16 * u + 8) * AB_KROW + tr_off)));
                    else da[u][pl_] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                    const unsigned char* kr = Ktp + pl_ * AB_KPL + li * AB_KROW + (16 * u + 4 * lh) * 2;
                    if (pl_ < OP) kb[u][pl_] = __builtin_bit_cast(bf16x8, join8(*reinterpret_cast<const u32x2*>(kr), *reinterpret_cast<const u32x2*>(kr + 16)));
                    else kb[u][pl_] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                } else {
                if (pl_ < PP) da[u][pl_] = *reinterpret_cast<const bf16x8*>(dSp + pl_ * AB_KPL + li * AB_KROW + u * 32 + lh * 16);
                else da[u][pl_] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                if (pl_ < OP) kb[u][pl_] = *reinterpret_cast<const bf16x8*>(Ktp + pl_ * AB_KPL + li * AB_KROW + u * 32 + lh * 16);
                else kb[u][pl_] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
            }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (PP == 3) dq = mfma16<F16>(da[u][2], kb[u][0], dq);
            if (OP == 3) dq = mfma16<F16>(da[u][0], kb[u][2], dq);
            if (OP == 3 || PP == 3) dq = mfma16<F16>(da[u][1], kb[u][1], dq);
            dq = mfma16<F16>(da[u][1], kb[u][0], dq);
            dq = mfma16<F16>(da[u][0], kb[u][1], dq);
            dq = mfma16<F16>(da[u][0], kb[u][0], dq);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                     // every lane holds its dS fragments: the planes may be overwritten
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int r = 0; r < 16; ++r) Pmine[crow(r, lh) * 32 + li] = F16 ? dq[r] * dq_inv : dq[r];
        // the tile's dV / dK join the running sums here rather than right behind their MFMAs: nothing waits for the matrix pipe (-1 %)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dvacc[r] = F16 ? fmaf(dvt[r], dv_inv, dvacc[r]) : dvacc[r] + dvt[r];
            dkacc[r] = F16 ? fmaf(dkt[r], dk_inv, dkacc[r]) : dkacc[r] + dkt[r];
        }
        __syncthreads();                                    // barrier B
        // fixed-order sum of the eight waves' partials -> this key block's slice of the dQ workspace
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = tid + i * 512;
            const int row = t / DP;
            if (q0 + row < p.S) {
                float acc = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w)
                    acc += reinterpret_cast<const float*>(smem + AB8_SHARED + w * AB8_WAVE + 3 * AB_KPL)[t];
                part[(long)(q0 + row) * DP + (t % DP)] = acc;
            }
        }
    }
    // ---- epilogue: dK^T, dV^T -> [kv][d] through the wave's (now free) dS region, coalesced row stores
    __syncthreads();
    float* Smine = reinterpret_cast<float*>(dSp);            // [32][33] floats = 4224 B <= 7680
    float am = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[li * 33 + crow(r, lh)] = (pass == 0 ? dkacc[r] * p.scale : dvacc[r]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int rr = lh; rr < 32; rr += 2) {
            const int kv = kv0 + rr;
            if (kv < p.S) {
                const float val = Smine[rr * 33 + li];
                float* dst = pass == 0 ? p.dk + ((long)b * p.S + kv) * p.lddk + (long)h * 32 + li : p.dv + ((long)b * p.S + kv) * p.lddv + (long)h * 32 + li;
                if (QS > 1 && qhalf == 1) dst = (pass == 0 ? p.dk2 : p.dv2) + ((long)b * p.S + kv) * ((long)p.H * 32) + (long)h * 32 + li;
                *dst = val;
                am = fmaxf(am, fabsf(val));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // (QS contributions per element: QS times the largest one bounds the sum -- the word holds max |x| or a bound)
    if (F16 && p.dqkv_amax) { __syncthreads(); amax_publish_block<8>(p.dqkv_amax, am * (float)QS, reinterpret_cast<float*>(smem)); }
}

// ---------------------------------------------------------------------------------------------
// [r6] the fp16-piece backward of attn_bwd_split8_kernel<2, 2, true, true, QS> (same arithmetic per wave, same fragments, bit-identical dK /
// dV and dQ slabs at NW = 8) re-cut around ONE workgroup barrier per query tile instead of two, with a loop body that is one basic block:
//   * the Q / dO tile planes, lse / delta and the waves' dQ partial tiles are double-buffered: after barrier t every wave (a) splits tile
//     t + 1 (in its prefetch registers since the iteration before) into the other plane buffer and fetches tile t + 2, (b) sums the eight
//     partials of tile t - 1 into the dQ slab, (c) computes tile t -- three independent streams the scheduler interleaves; the former
//     barrier A (tile staged) and the serial reduce phase behind barrier B are gone;
//   * the wave maximum of |dS| (the tile's fp16 scale) and the delta row sums run on the DPP path (common.h wave_max_nonneg / oct_sum)
//     instead of six + three dependent ds_bpermute round trips per tile;
//   * the K^T fragments of the dQ product stay in registers (16) instead of four LDS reads per tile: the per-wave LDS is the dS^T planes and
//     two dQ partial tiles; LDS cut to what the mode uses: 20.5 KB shared + 13 KB per wave (NW = 8: 124.5 KB; NW = 4: 72.5 KB, two per CU);
//   * no predicated stores or loads in the loop: rows past the sequence end and the reduce of "tile -1" store to a dump line at the head of
//     the workspace (the delta array this mode does not use), every lane of a row writes the row's lse / delta word.
// ---------------------------------------------------------------------------------------------
template <int NW> struct AH16 {
    static constexpr int QG = 2 * 2 * AB_KPL;                        // one buffer: Q and dO, two pieces each, k-major
    static constexpr int SHARED = 2 * QG + 2 * 64 * 4;               // two buffers + two x (lse | delta)
    static constexpr int PM = 32 * 32 * 4;                           // a wave's dQ partial tile
    static constexpr int WAVE = 2 * AB_KPL + 2 * PM;                 // dS^T planes (K^T planes while the prologue builds its fragments; epilogue tile) + 2 partial tiles
    static constexpr int LDS = SHARED + NW * WAVE;
};
#define SPLIT2H(x0, x1, sc, a, b) do { if (VAR & 1) split2h_pair_mix(x0, x1, sc, a, b); else split2h_pair(x0, x1, sc, a, b); } while (0)
// VAR (tuning): bit 0 = second pieces through v_fma_mix{lo,hi}_f16, bit 1 = P masked and scaled by one multiply
template <int NW, int QS = 1, int VAR = 0>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void attn_bwd_h16_kernel(const AttnArgs p) {
    constexpr int DP = 32, NT = 64 * NW, KPT = 512 / NT;          // KPT: staged tensors (Q, dO) per thread
    static_assert(NW == 4 || NW == 8, "four or eight waves");
    using G = AH16<NW>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[G::LDS];
    float* aux = reinterpret_cast<float*>(smem + 2 * G::QG);       // [buffer][lse 32 | delta 32]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, kblk, qhalf = 0;
    xcd_group_decode(blockIdx.x, p.B * p.H, p.n_kblocks * QS, bh, kblk);
    if (QS > 1) { qhalf = kblk % QS; kblk /= QS; }
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int kv0 = kblk * (32 * NW) + wave * 32;
    f32x4 kraw[2][2], vraw[2][2];
    {
        const float* krow = p.k + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldk + (long)hk * 32;
        const float* vrow = p.v + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldv + (long)hk * 32;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            kraw[u][0] = *reinterpret_cast<const f32x4*>(krow + 16 * u + 8 * lh); kraw[u][1] = *reinterpret_cast<const f32x4*>(krow + 16 * u + 8 * lh + 4);
            vraw[u][0] = *reinterpret_cast<const f32x4*>(vrow + 16 * u + 8 * lh); vraw[u][1] = *reinterpret_cast<const f32x4*>(vrow + 16 * u + 8 * lh + 4);
        }
    }
    float sc_in = 1.f, so_in = 1.f, sc_g = 1.f, so_g = 1.f;
    {
        const unsigned w_in = amax_peek(p.qkv_amax), w_g = amax_peek(p.dout_amax);
        amax_finish(w_in, sc_in, so_in);
        amax_finish(w_g, sc_g, so_g);
    }
    const float c = p.scale * LOG2E * so_in * so_in;
    const float dp_inv = so_g * so_in;
    const float dv_inv = so_g * P_INV;
    unsigned char* dSp = smem + G::SHARED + wave * G::WAVE;                      // 2 planes [kv][32 q]
    unsigned char* Pm = dSp + 2 * AB_KPL;                                        // 2 x [32 q][32 d] fp32
    const int tr_off = lds_tr_lane_offset(lane, AB_KROW);

    bf16x8 kf[2][2], vf[2][2], kb[2][2];
    const bool kv_ok = kv0 + li < p.S;
    const float p_mask = kv_ok ? P_SCALE : 0.f;
    {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 a0 = kraw[u][0], a1 = kraw[u][1];
            const f32x4 w0 = vraw[u][0], w1 = vraw[u][1];
            u32x4 ph, pm, vh, vm;
            unsigned a_, b_;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                SPLIT2H(a0[2 * e], a0[2 * e + 1], sc_in, a_, b_); ph[e] = a_; pm[e] = b_;
                SPLIT2H(a1[2 * e], a1[2 * e + 1], sc_in, a_, b_); ph[2 + e] = a_; pm[2 + e] = b_;
                SPLIT2H(w0[2 * e], w0[2 * e + 1], sc_in, a_, b_); vh[e] = a_; vm[e] = b_;
                SPLIT2H(w1[2 * e], w1[2 * e + 1], sc_in, a_, b_); vh[2 + e] = a_; vm[2 + e] = b_;
            }
            kf[0][u] = __builtin_bit_cast(bf16x8, ph); kf[1][u] = __builtin_bit_cast(bf16x8, pm);
            vf[0][u] = __builtin_bit_cast(bf16x8, vh); vf[1][u] = __builtin_bit_cast(bf16x8, vm);
        }
        // K^T planes [d][32 kv] of this wave's keys through its dS^T region, then the dQ product's B fragments for good
        unsigned char* Ktp = dSp;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int item = lane + 64 * it, kp = item >> 3, d0 = (item & 7) * 4;
            f32x4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0;
            if (kv0 + 2 * kp < p.S) r0 = *reinterpret_cast<const f32x4*>(p.k + ((long)b * p.S + kv0 + 2 * kp) * p.ldk + (long)hk * 32 + d0);
            if (kv0 + 2 * kp + 1 < p.S) r1 = *reinterpret_cast<const f32x4*>(p.k + ((long)b * p.S + kv0 + 2 * kp + 1) * p.ldk + (long)hk * 32 + d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_;
                SPLIT2H(r0[e], r1[e], sc_in, a_, b_);
                unsigned char* dst = Ktp + (d0 + e) * AB_KROW + kp * 4;
                *reinterpret_cast<unsigned*>(dst) = a_;
                *reinterpret_cast<unsigned*>(dst + AB_KPL) = b_;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int pl_ = 0; pl_ < 2; ++pl_) {
                const unsigned char* kr = Ktp + pl_ * AB_KPL + li * AB_KROW + (16 * u + 4 * lh) * 2;
                kb[u][pl_] = __builtin_bit_cast(bf16x8, join8(*reinterpret_cast<const u32x2*>(kr), *reinterpret_cast<const u32x2*>(kr + 16)));
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                     // the fragments are in registers: the region is the dS^T planes from here on
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    f32x16 dvacc, dkacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dvacc[r] = 0.f; dkacc[r] = 0.f; }

    const float* qbase = p.q + (long)b * p.S * p.ldq + (long)h * 32;
    const float* gbase = p.dout + (long)b * p.S * p.ldo + (long)h * 32;
    const float* obase = p.oin + (long)b * p.S * p.ldo + (long)h * 32;
    const float* lse_b = p.lse + ((long)b * p.H + h) * p.S;
    // staging: row = (tid & 255) >> 3, 4-d chunk = tid & 7; 512 threads: kind = tid >> 8 (0: Q, 1: dO; wave-uniform); 256 threads: every thread both
    const int t8 = tid & 255, srow = t8 >> 3, sch = tid & 7;
    f32x4 rk[KPT], ro = {0.f, 0.f, 0.f, 0.f};
    float rl = 0.f;
    auto fetch = [&](int q0) {
        const long r_ = min(q0 + srow, p.S - 1);
        const bool ok = q0 + srow < p.S;
#pragma unroll
        for (int kk = 0; kk < KPT; ++kk) {
            const int kind = KPT == 2 ? kk : (tid >> 8);
            rk[kk] = *reinterpret_cast<const f32x4*>((kind == 0 ? qbase + r_ * p.ldq : gbase + r_ * p.ldo) + sch * 4);
            if (!ok) rk[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // (512 threads: the Q-staging waves load a line they have just asked for in place of O -- no branch in the loop)
        ro = *reinterpret_cast<const f32x4*>(((KPT == 2 || (tid >> 8) == 1) ? obase + r_ * p.ldo : qbase + r_ * p.ldq) + sch * 4);
        const float lv = lse_b[r_];          // (unconditional: a predicated load would put a branch and a full wait into the loop)
        rl = ok ? lv * LOG2E : INFINITY;
    };
    // split the prefetched tile into plane buffer `buf`; every lane of a row writes the row's lse (Q side) / delta (dO side) word
    auto stage = [&](int buf) {
        unsigned char* Qk = smem + buf * G::QG;
        unsigned char* Gk = Qk + 2 * AB_KPL;
        float* ax = aux + buf * 64;
#pragma unroll
        for (int kk = 0; kk < KPT; ++kk) {
            const int kind = KPT == 2 ? kk : (tid >> 8);
            const float sc_st = kind == 0 ? sc_in : sc_g;
            u32x2 h2, m2;
            unsigned a_, b_;
            SPLIT2H(rk[kk][0], rk[kk][1], sc_st, a_, b_); h2[0] = a_; m2[0] = b_;
            SPLIT2H(rk[kk][2], rk[kk][3], sc_st, a_, b_); h2[1] = a_; m2[1] = b_;
            unsigned char* dk_ = (kind == 0 ? Qk : Gk) + srow * AB_KROW + sch * 8;
            *reinterpret_cast<u32x2*>(dk_) = h2; *reinterpret_cast<u32x2*>(dk_ + AB_KPL) = m2;
            // delta[q] = sum_d dO[q][d] O[q][d]: eight consecutive lanes hold one row's 32 d
            const float dsum = oct_sum(fmaf(rk[kk][0], ro[0], fmaf(rk[kk][1], ro[1], fmaf(rk[kk][2], ro[2], rk[kk][3] * ro[3]))));          // (as attn_bwd_split8_kernel: explicit, not the compiler's choice of contractions)
            ax[kind * 32 + srow] = kind == 0 ? rl : dsum;
        }
    };
    const int nq = (p.S + 31) / 32;
    const long part_stride = (long)p.B * p.H * p.S * DP;
    float* part = p.dq_part + (long)kblk * part_stride + ((long)b * p.H + h) * p.S * DP;
    float* dump = p.delta;          // the head of the workspace: this mode keeps no delta array (>= 1 024 floats: checked by the launcher)
    // fixed-order sum of the waves' partials of the tile at q0 -> this key block's slice of the dQ workspace
    auto reduce = [&](int buf, int q0, bool live) {
#pragma unroll
        for (int i = 0; i < 1024 / NT; ++i) {
            const int t = tid + i * NT;
            const int row = t / DP;
            float acc = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w)
                acc += reinterpret_cast<const float*>(smem + G::SHARED + w * G::WAVE + 2 * AB_KPL + buf * G::PM)[t];
            float* dst = (live && q0 + row < p.S) ? part + (long)(q0 + row) * DP + (t % DP) : dump + t;
            *dst = acc;
        }
    };
    const int nq_each = (nq + QS - 1) / QS;
    const int qt_begin = qhalf * nq_each, qt_end = min(nq, qt_begin + nq_each);
    fetch(qt_begin * 32);
    stage(0);
    fetch(qt_begin * 32 + 32);
    __syncthreads();
    for (int qt = qt_begin; qt < qt_end; ++qt) {
        const int cur = (qt - qt_begin) & 1;
        const unsigned char* Qk = smem + cur * G::QG;
        const unsigned char* Gk = Qk + 2 * AB_KPL;
        const float* lse_s = aux + cur * 64;
        const float* del_s = lse_s + 32;
        stage(cur ^ 1);                         // tile qt + 1 (past the end: zeros / a clamped row, never read)
        fetch(qt * 32 + 64);
        reduce(cur ^ 1, qt * 32 - 32, qt > qt_begin);

        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned char* qr = Qk + li * AB_KROW + u * 32 + lh * 16;
            const unsigned char* gr = Gk + li * AB_KROW + u * 32 + lh * 16;
            const bf16x8 q0_ = *reinterpret_cast<const bf16x8*>(qr), q1_ = *reinterpret_cast<const bf16x8*>(qr + AB_KPL);
            const bf16x8 g0_ = *reinterpret_cast<const bf16x8*>(gr), g1_ = *reinterpret_cast<const bf16x8*>(gr + AB_KPL);
            s = mfma16<true>(q1_, kf[0][u], s);
            dp = mfma16<true>(g1_, vf[0][u], dp);
            s = mfma16<true>(q0_, kf[1][u], s);
            dp = mfma16<true>(g0_, vf[1][u], dp);
            s = mfma16<true>(q0_, kf[0][u], s);
            dp = mfma16<true>(g0_, vf[0][u], dp);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = crow(r, lh);
            // P arrives masked (keys past the sequence end) AND scaled by 2^13 from one multiply; dS = P (dP - delta) carries the same factor
            // into its own power-of-two tile scale (exact: the scale is formed from the scaled values)
            float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse_s[qr]));
            if (VAR & 2) pv *= p_mask; else if (!kv_ok) pv = 0.f;
            s[r] = pv;
            dp[r] = pv * fmaf(dp[r], dp_inv, -del_s[qr]);
        }
        float sc_ds = 1.f, ds_inv = 1.f;
        {
            float mx = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fabsf(dp[r]));
            pow2_scale(wave_max_nonneg(mx), sc_ds, ds_inv);
        }
        const float dk_inv = (VAR & 2) ? ds_inv * so_in * P_INV : ds_inv * so_in, dq_inv = dk_inv;          // (ds_inv undoes sc_ds, formed from 2^13 dS: the pieces are those of sc dS)
        f32x16 dvt, dkt;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dvt[r] = 0.f; dkt[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            u32x4 ph, pm, sh, sm;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_;
                if (VAR & 2) { if (VAR & 1) split2h_pre(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], a_, b_); else split2h_pair(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], 1.f, a_, b_); } else SPLIT2H(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], P_SCALE, a_, b_); ph[e] = a_; pm[e] = b_;
                SPLIT2H(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], sc_ds, a_, b_); sh[e] = a_; sm[e] = b_;
            }
            {   // dS^T pieces [kv = li][q]: registers 8u .. 8u + 3 are queries 16u + 4hi + 0..3, 8u + 4 .. 8u + 7 the same, eight up
                unsigned char* dst = dSp + li * AB_KROW + (16 * u + 4 * lh) * 2;
                *reinterpret_cast<u32x2*>(dst) = u32x2{sh[0], sh[1]};
                *reinterpret_cast<u32x2*>(dst + 16) = u32x2{sh[2], sh[3]};
                *reinterpret_cast<u32x2*>(dst + AB_KPL) = u32x2{sm[0], sm[1]};
                *reinterpret_cast<u32x2*>(dst + AB_KPL + 16) = u32x2{sm[2], sm[3]};
            }
            const bf16x8 p0 = __builtin_bit_cast(bf16x8, ph), p1 = __builtin_bit_cast(bf16x8, pm);
            const bf16x8 d0 = __builtin_bit_cast(bf16x8, sh), d1 = __builtin_bit_cast(bf16x8, sm);
            bf16x8 ga[2], qa[2];
#pragma unroll
            for (int pl_ = 0; pl_ < 2; ++pl_) {
                ga[pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(Gk + pl_ * AB_KPL + (16 * u) * AB_KROW + tr_off), lds_tr(Gk + pl_ * AB_KPL + (16 * u + 8) * AB_KROW + tr_off)));
                qa[pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(Qk + pl_ * AB_KPL + (16 * u) * AB_KROW + tr_off), lds_tr(Qk + pl_ * AB_KPL + (16 * u + 8) * AB_KROW + tr_off)));
            }
            dvt = mfma16<true>(ga[1], p0, dvt);
            dkt = mfma16<true>(qa[1], d0, dkt);
            dvt = mfma16<true>(ga[0], p1, dvt);
            dkt = mfma16<true>(qa[0], d1, dkt);
            dvt = mfma16<true>(ga[0], p0, dvt);
            dkt = mfma16<true>(qa[0], d0, dkt);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x16 dq;
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[r] = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 da[2];
#pragma unroll
            for (int pl_ = 0; pl_ < 2; ++pl_)
                da[pl_] = __builtin_bit_cast(bf16x8, join8(lds_tr(dSp + pl_ * AB_KPL + (16 * u) * AB_KROW + tr_off), lds_tr(dSp + pl_ * AB_KPL + (16 * u + 8) * AB_KROW + tr_off)));
            dq = mfma16<true>(da[1], kb[u][0], dq);
            dq = mfma16<true>(da[0], kb[u][1], dq);
            dq = mfma16<true>(da[0], kb[u][0], dq);
        }
        float* Pmine = reinterpret_cast<float*>(Pm + cur * G::PM);
#pragma unroll
        for (int r = 0; r < 16; ++r) Pmine[crow(r, lh) * 32 + li] = dq[r] * dq_inv;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dvacc[r] = fmaf(dvt[r], dv_inv, dvacc[r]);
            dkacc[r] = fmaf(dkt[r], dk_inv, dkacc[r]);
        }
        __syncthreads();          // the tile's partials are written, tile qt + 1 is staged, everyone is done with tile qt's planes and tile qt - 1's partials
    }
    reduce((qt_end - 1 - qt_begin) & 1, qt_end * 32 - 32, qt_end > qt_begin);
    // ---- epilogue: dK^T, dV^T -> [kv][d] through the wave's (now free) dS region, coalesced row stores
    float* Smine = reinterpret_cast<float*>(dSp);            // [32][33] floats = 4 224 B <= 5 120
    float am = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[li * 33 + crow(r, lh)] = (pass == 0 ? dkacc[r] * p.scale : dvacc[r]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int rr = lh; rr < 32; rr += 2) {
            const int kv = kv0 + rr;
            if (kv < p.S) {
                const float val = Smine[rr * 33 + li];
                float* dst = pass == 0 ? p.dk + ((long)b * p.S + kv) * p.lddk + (long)h * 32 + li : p.dv + ((long)b * p.S + kv) * p.lddv + (long)h * 32 + li;
                if (QS > 1 && qhalf == 1) dst = (pass == 0 ? p.dk2 : p.dv2) + ((long)b * p.S + kv) * ((long)p.H * 32) + (long)h * 32 + li;
                *dst = val;
                am = fmaxf(am, fabsf(val));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (p.dqkv_amax) { __syncthreads(); amax_publish_block<NW>(p.dqkv_amax, am * (float)QS, reinterpret_cast<float*>(smem)); }
}

// ---------------------------------------------------------------------------------------------
#undef SPLIT2H
// backward for 32 < head_dim <= 64 with two rounded pieces of everything, 8 waves x 32 keys = 256 keys per workgroup (one workgroup
// per CU, two waves per SIMD -- the 4-wave kernel above runs one; half the Q / dO tile staging per key and half the dQ slabs).
// Everything a wave keeps per key lives in LDS except V: K as two bf16 planes [32 kv][64 d] (B operand of S through 16-byte row
// reads, B operand of dQ through transposing reads), dS^T planes; the Q / dO tile is staged k-major only and read row-wise (S, dP)
// and through transposing reads (dK, dV).  158 KB of LDS.
// ---------------------------------------------------------------------------------------------
constexpr int AD8_KROW = 64 * 2 + 16, AD8_KPL = 32 * AD8_KROW;                     // a [32 rows][64 d] bf16 plane
constexpr int AD8_SHARED = 2 * 2 * AD8_KPL + 64 * 4;                                // Q and dO, two pieces each + lse / delta
constexpr int AD8_WAVE = 2 * AD8_KPL + 32 * 64 * 4;                                 // K planes + (dS^T planes | dQ partial [32][64] fp32)
constexpr int AD8_LDS = AD8_SHARED + 8 * AD8_WAVE;
// [r6] F16: two fp16 pieces of the scaled operands (as attn_bwd_split_dh_kernel<64, 2, 2, true>: the same scales, the same per-tile
// scale of dS, the inverse scales on the fused multiply-adds that join the tile products to the running sums).  QS = 2: the query tiles
// of a 256-key block go to two workgroups (as attn_bwd_split8_kernel<.., QS = 2>): batch x heads x key blocks of 128 .. 255 fill the chip
// with eight waves per CU (the 3-D configuration: 1 x 8 heads x 16 blocks); the second half's dK / dV go to two spare dQ slabs and
// attn_add_cols_kernel adds them in a fixed order.
template <bool F16 = false, int QS = 1>
__global__ __launch_bounds__(512, 1) void attn_bwd_split8_dh_kernel(const AttnArgs p) {
    constexpr int DH = 64, NU = 4, NDT = 2, CPR = 16, NW = 8;
    __shared__ __attribute__((aligned(16))) unsigned char smem[AD8_LDS];
    unsigned char* Qk = smem;
    unsigned char* Gk = Qk + 2 * AD8_KPL;
    float* lse_s = reinterpret_cast<float*>(Gk + 2 * AD8_KPL);
    float* del_s = lse_s + 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    int bh, kblk, qhalf = 0;
    xcd_group_decode(blockIdx.x, p.B * p.H, p.n_kblocks * QS, bh, kblk);
    if (QS > 1) { qhalf = kblk % QS; kblk /= QS; }
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int kv0 = kblk * 256 + wave * 32;
    const int D = p.D;
    float sc_in = 1.f, so_in = 1.f, sc_g = 1.f, so_g = 1.f;
    if (F16) { amax_scale(p.qkv_amax, sc_in, so_in); amax_scale(p.dout_amax, sc_g, so_g); }
    const float c = p.scale * LOG2E * so_in * so_in;
    const float dp_inv = so_g * so_in, dv_inv = F16 ? so_g * P_INV : 1.f;
    unsigned char* Kpl = smem + AD8_SHARED + wave * AD8_WAVE;         // two planes [32 kv][64 d]
    unsigned char* dSp = Kpl + 2 * AD8_KPL;                            // two planes [32 kv][32 q] (row stride AB_KROW); dQ partial after the MFMAs
    float* Pmine = reinterpret_cast<float*>(dSp);
    const int tr_k = lds_tr_lane_offset(lane, AD8_KROW), tr_s = lds_tr_lane_offset(lane, AB_KROW);

    // V^T as the split B operand of dP: lane (kv = li, hi) holds d = 16u + 8hi + e; K goes to the wave's planes
    bf16x8 vf[2][NU];
    const bool kv_ok = kv0 + li < p.S;
    {
        const float* vrow = p.v + ((long)b * p.S + min(kv0 + li, p.S - 1)) * p.ldv + (long)hk * D;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const f32x4 w0 = load4(vrow, 16 * u + 8 * lh, D, true, true), w1 = load4(vrow, 16 * u + 8 * lh + 4, D, true, true);
            u32x4 vh, vm;
            unsigned a_, b_;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (F16) { split2h_pair_gemm(w0[2 * e], w0[2 * e + 1], sc_in, a_, b_); vh[e] = a_; vm[e] = b_; split2h_pair_gemm(w1[2 * e], w1[2 * e + 1], sc_in, a_, b_); vh[2 + e] = a_; vm[2 + e] = b_; }
                else { split2_pair(w0[2 * e], w0[2 * e + 1], a_, b_); vh[e] = a_; vm[e] = b_; split2_pair(w1[2 * e], w1[2 * e + 1], a_, b_); vh[2 + e] = a_; vm[2 + e] = b_; }
            }
            vf[0][u] = __builtin_bit_cast(bf16x8, vh); vf[1][u] = __builtin_bit_cast(bf16x8, vm);
        }
        for (int t = lane; t < 32 * CPR; t += 64) {
            const int row = t / CPR, d = (t % CPR) * 4;
            const f32x4 a = load4(p.k + ((long)b * p.S + min(kv0 + row, p.S - 1)) * p.ldk + (long)hk * D, d, D, kv0 + row < p.S, true);
            unsigned h0, m0, h1, m1;
            if (F16) { split2h_pair_gemm(a[0], a[1], sc_in, h0, m0); split2h_pair_gemm(a[2], a[3], sc_in, h1, m1); }
            else { split2_pair(a[0], a[1], h0, m0); split2_pair(a[2], a[3], h1, m1); }
            *reinterpret_cast<u32x2*>(Kpl + row * AD8_KROW + d * 2) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(Kpl + AD8_KPL + row * AD8_KROW + d * 2) = u32x2{m0, m1};
        }
    }
    f32x16 dvacc[NDT], dkacc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dvacc[dt][r] = 0.f; dkacc[dt][r] = 0.f; }

    const float* qbase = p.q + (long)b * p.S * p.ldq + (long)h * D;
    const float* gbase = p.dout + (long)b * p.S * p.ldo + (long)h * D;
    const float* lse_b = p.lse + ((long)b * p.H + h) * p.S;
    const float* del_b = p.delta + ((long)b * p.H + h) * p.S;
    // staging: one float4 of Q and one of dO per thread (row = tid >> 4, chunk = tid & 15)
    f32x4 rq, rg;
    float rl = 0.f, rd = 0.f;
    auto fetch = [&](int q0) {
        const int row = tid >> 4, d = (tid & 15) * 4;
        const bool ok = q0 + row < p.S;
        const long r = min(q0 + row, p.S - 1);
        rq = load4(qbase + r * p.ldq, d, D, ok, true);
        rg = load4(gbase + r * p.ldo, d, D, ok, true);
        if (tid < 32) {
            const bool okq = q0 + tid < p.S;
            rl = okq ? lse_b[q0 + tid] * LOG2E : INFINITY;
            rd = okq ? del_b[q0 + tid] : 0.f;
        }
    };
    const int nq = (p.S + 31) / 32;
    const long part_stride = (long)p.B * p.H * p.S * DH;
    float* part = p.dq_part + (long)kblk * part_stride + ((long)b * p.H + h) * p.S * DH;

    const int nq_each = (nq + QS - 1) / QS;
    const int qt_begin = qhalf * nq_each, qt_end = min(nq, qt_begin + nq_each);
    fetch(qt_begin * 32);
    for (int qt = qt_begin; qt < qt_end; ++qt) {
        const int q0 = qt * 32;
        {
            const int row = tid >> 4, ch = tid & 15;
            unsigned h0, m0, h1, m1;
            if (F16) { split2h_pair_gemm(rq[0], rq[1], sc_in, h0, m0); split2h_pair_gemm(rq[2], rq[3], sc_in, h1, m1); }
            else { split2_pair(rq[0], rq[1], h0, m0); split2_pair(rq[2], rq[3], h1, m1); }
            *reinterpret_cast<u32x2*>(Qk + row * AD8_KROW + ch * 8) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(Qk + AD8_KPL + row * AD8_KROW + ch * 8) = u32x2{m0, m1};
            if (F16) { split2h_pair_gemm(rg[0], rg[1], sc_g, h0, m0); split2h_pair_gemm(rg[2], rg[3], sc_g, h1, m1); }
            else { split2_pair(rg[0], rg[1], h0, m0); split2_pair(rg[2], rg[3], h1, m1); }
            *reinterpret_cast<u32x2*>(Gk + row * AD8_KROW + ch * 8) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(Gk + AD8_KPL + row * AD8_KROW + ch * 8) = u32x2{m0, m1};
        }
        if (tid < 32) { lse_s[tid] = rl; del_s[tid] = rd; }
        __syncthreads();                                    // barrier A
        if (qt + 1 < qt_end) fetch(q0 + 32);

        // ---- S[q][kv] and dP[q][kv]: A = Q / dO planes (lane -> query row), B = K planes (LDS) / V^T (registers)
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const unsigned char* qr = Qk + li * AD8_KROW + u * 32 + lh * 16;
            const unsigned char* gr = Gk + li * AD8_KROW + u * 32 + lh * 16;
            const unsigned char* kr = Kpl + li * AD8_KROW + u * 32 + lh * 16;
            const bf16x8 q0_ = *reinterpret_cast<const bf16x8*>(qr), q1_ = *reinterpret_cast<const bf16x8*>(qr + AD8_KPL);
            const bf16x8 g0_ = *reinterpret_cast<const bf16x8*>(gr), g1_ = *reinterpret_cast<const bf16x8*>(gr + AD8_KPL);
            const bf16x8 k0_ = *reinterpret_cast<const bf16x8*>(kr), k1_ = *reinterpret_cast<const bf16x8*>(kr + AD8_KPL);
            s = mfma16<F16>(q1_, k0_, s);
            dp = mfma16<F16>(g1_, vf[0][u], dp);
            s = mfma16<F16>(q0_, k1_, s);
            dp = mfma16<F16>(g0_, vf[1][u], dp);
            s = mfma16<F16>(q0_, k0_, s);
            dp = mfma16<F16>(g0_, vf[0][u], dp);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = crow(r, lh);
            float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse_s[qr]));
            if (!kv_ok) pv = 0.f;
            s[r] = pv;
            dp[r] = F16 ? pv * fmaf(dp[r], dp_inv, -del_s[qr]) : pv * (dp[r] - del_s[qr]);
        }
        float sc_ds = 1.f, ds_inv = 1.f;          // fp16 pieces: the tile's own power-of-two scale for dS
        if (F16) {
            float mx = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fabsf(dp[r]));
            pow2_scale(wave_max_nonneg(mx), sc_ds, ds_inv);
        }
        const float dk_inv = ds_inv * so_in;
        // ---- dV^T / dK^T: the tile's contributions start from zero on the matrix pipe and join the running sums on the vector pipe.
        // All pieces first (P and dS die with them), then one 32-row d tile at a time: 32 accumulator registers live instead of 64, the
        // same MFMA order per accumulator
        bf16x8 pp[2][2], dd[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            u32x4 ph, pm, sh, sm;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a_, b_;
                if (F16) { split2h_pair_gemm(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], P_SCALE, a_, b_); ph[e] = a_; pm[e] = b_; split2h_pair_gemm(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], sc_ds, a_, b_); sh[e] = a_; sm[e] = b_; }
                else { split2_pair(s[8 * u + 2 * e], s[8 * u + 2 * e + 1], a_, b_); ph[e] = a_; pm[e] = b_; split2_pair(dp[8 * u + 2 * e], dp[8 * u + 2 * e + 1], a_, b_); sh[e] = a_; sm[e] = b_; }
            }
            // dS^T pieces [kv = li][q]: registers 8u .. 8u + 3 are queries 16u + 4hi + 0..3, 8u + 4 .. 8u + 7 the same, eight up
            unsigned char* dst = dSp + li * AB_KROW + (16 * u + 4 * lh) * 2;
            *reinterpret_cast<u32x2*>(dst) = u32x2{sh[0], sh[1]};
            *reinterpret_cast<u32x2*>(dst + 16) = u32x2{sh[2], sh[3]};
            *reinterpret_cast<u32x2*>(dst + AB_KPL) = u32x2{sm[0], sm[1]};
            *reinterpret_cast<u32x2*>(dst + AB_KPL + 16) = u32x2{sm[2], sm[3]};
            pp[u][0] = __builtin_bit_cast(bf16x8, ph); pp[u][1] = __builtin_bit_cast(bf16x8, pm);
            dd[u][0] = __builtin_bit_cast(bf16x8, sh); dd[u][1] = __builtin_bit_cast(bf16x8, sm);
        }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            f32x16 dvt, dkt;
#pragma unroll
            for (int r = 0; r < 16; ++r) { dvt[r] = 0.f; dkt[r] = 0.f; }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                // dO^T / Q^T fragments from the k-major planes: column d = 32dt + li, rows q = 16u + 4hi + 0..3 and + 8
                const unsigned char* gb = Gk + (16 * u) * AD8_KROW + 32 * dt * 2 + tr_k;
                const unsigned char* qb = Qk + (16 * u) * AD8_KROW + 32 * dt * 2 + tr_k;
                const bf16x8 ga0 = __builtin_bit_cast(bf16x8, join8(lds_tr(gb), lds_tr(gb + 8 * AD8_KROW)));
                const bf16x8 ga1 = __builtin_bit_cast(bf16x8, join8(lds_tr(gb + AD8_KPL), lds_tr(gb + AD8_KPL + 8 * AD8_KROW)));
                const bf16x8 qa0 = __builtin_bit_cast(bf16x8, join8(lds_tr(qb), lds_tr(qb + 8 * AD8_KROW)));
                const bf16x8 qa1 = __builtin_bit_cast(bf16x8, join8(lds_tr(qb + AD8_KPL), lds_tr(qb + AD8_KPL + 8 * AD8_KROW)));
                dvt = mfma16<F16>(ga1, pp[u][0], dvt);
                dkt = mfma16<F16>(qa1, dd[u][0], dkt);
                dvt = mfma16<F16>(ga0, pp[u][1], dvt);
                dkt = mfma16<F16>(qa0, dd[u][1], dkt);
                dvt = mfma16<F16>(ga0, pp[u][0], dvt);
                dkt = mfma16<F16>(qa0, dd[u][0], dkt);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dvacc[dt][r] = F16 ? fmaf(dvt[r], dv_inv, dvacc[dt][r]) : dvacc[dt][r] + dvt[r];
                dkacc[dt][r] = F16 ? fmaf(dkt[r], dk_inv, dkacc[dt][r]) : dkacc[dt][r] + dkt[r];
            }
        }
        // ---- dQ[q][d] partial = sum_kv dS[q][kv] K[kv][d]: both operands through transposing reads (k-slot e = key 16u + 8 (e >> 2) + 4 hi + (e & 3))
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x16 dq[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bf16x8 da0 = __builtin_bit_cast(bf16x8, join8(lds_tr(dSp + (16 * u) * AB_KROW + tr_s), lds_tr(dSp + (16 * u + 8) * AB_KROW + tr_s)));
            const bf16x8 da1 = __builtin_bit_cast(bf16x8, join8(lds_tr(dSp + AB_KPL + (16 * u) * AB_KROW + tr_s), lds_tr(dSp + AB_KPL + (16 * u + 8) * AB_KROW + tr_s)));
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const unsigned char* kb = Kpl + (16 * u) * AD8_KROW + 32 * dt * 2 + tr_k;
                const bf16x8 kb0 = __builtin_bit_cast(bf16x8, join8(lds_tr(kb), lds_tr(kb + 8 * AD8_KROW)));
                const bf16x8 kb1 = __builtin_bit_cast(bf16x8, join8(lds_tr(kb + AD8_KPL), lds_tr(kb + AD8_KPL + 8 * AD8_KROW)));
                dq[dt] = mfma16<F16>(da1, kb0, dq[dt]);
                dq[dt] = mfma16<F16>(da0, kb1, dq[dt]);
                dq[dt] = mfma16<F16>(da0, kb0, dq[dt]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                     // every lane holds its dS fragments: the planes may be overwritten
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) Pmine[crow(r, lh) * DH + 32 * dt + li] = F16 ? dq[dt][r] * dk_inv : dq[dt][r];
        __syncthreads();                                    // barrier B
        // fixed-order sum of the eight waves' partials -> this key block's slice of the dQ workspace
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = tid + i * 512;
            const int row = t / DH;
            if (q0 + row < p.S) {
                float acc = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w)
                    acc += reinterpret_cast<const float*>(smem + AD8_SHARED + w * AD8_WAVE + 2 * AD8_KPL)[t];
                part[(long)(q0 + row) * DH + (t % DH)] = acc;
            }
        }
    }
    // ---- epilogue: dK^T, dV^T -> [kv][d] through the wave's (now free) dS region, coalesced row stores
    __syncthreads();
    float* Smine = reinterpret_cast<float*>(dSp);            // [32][33] floats
    float am = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2 * NDT; ++pass) {
        const int dt = pass >> 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) Smine[li * 33 + crow(r, lh)] = ((pass & 1) == 0 ? dkacc[dt][r] * p.scale : dvacc[dt][r]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int rr = lh; rr < 32; rr += 2) {
            const int kv = kv0 + rr;
            if (kv < p.S && 32 * dt + li < D) {
                const float val = Smine[rr * 33 + li];
                float* dst = (pass & 1) == 0 ? p.dk + ((long)b * p.S + kv) * p.lddk + (long)h * D + 32 * dt + li : p.dv + ((long)b * p.S + kv) * p.lddv + (long)h * D + 32 * dt + li;
                if (QS > 1 && qhalf == 1) dst = ((pass & 1) == 0 ? p.dk2 : p.dv2) + ((long)b * p.S + kv) * ((long)p.H * D) + (long)h * D + 32 * dt + li;
                *dst = val;
                am = fmaxf(am, fabsf(val));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // (QS contributions per element: QS times the largest one bounds the sum -- the word holds max |x| or a bound)
    if (F16 && p.dqkv_amax) { __syncthreads(); amax_publish_block<8>(p.dqkv_amax, am * (float)QS, reinterpret_cast<float*>(smem)); }
}

// a[r][c] += a2[r][c], b[r][c] += b2[r][c] over [rows][4 c4]: a, b pitched column blocks (dK / dV inside the fused dqkv buffer), a2, b2 dense
// (the second half's partials of the query-split backward)
__global__ void attn_add_cols_kernel(float* a, long lda, const float* a2, float* b, long ldb, const float* b2, long rows, int c4) {
    const long n = rows * c4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / c4; const int c = (int)(i - r * c4) * 4;
        f32x4* pa = reinterpret_cast<f32x4*>(a + r * lda + c);
        f32x4* pb = reinterpret_cast<f32x4*>(b + r * ldb + c);
        *pa = *pa + *reinterpret_cast<const f32x4*>(a2 + r * (long)c4 * 4 + c);
        *pb = *pb + *reinterpret_cast<const f32x4*>(b2 + r * (long)c4 * 4 + c);
    }
}

// S == 1: one key, so the softmax is 1 and out[b,h,:] = v[b,hk,:] -- a copy, exact by construction (the general kernels reach it only to
// fp32 rounding: two fp16 pieces carry 22 bits of v, and exp2(fma(s, c, -rn(m c))) is 1 - 2^-24 where rn(m c) rounded up); lse = scale <q, k>.
// One wave per (b, h); scalar loads and stores: any base, any pitch.
__global__ __launch_bounds__(64) void attn_fwd_one_key_kernel(const AttnArgs p) {
    const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const float* q = p.q + (long)b * p.ldq + (long)h * p.D;
    const float* k = p.k + (long)b * p.ldk + (long)hk * p.D;
    const float* v = p.v + (long)b * p.ldv + (long)hk * p.D;
    float* o = p.o + (long)b * p.ldo + (long)h * p.D;
    float acc = 0.f;
    for (int d = threadIdx.x; d < p.D; d += 64) { acc = fmaf(q[d], k[d], acc); o[d] = v[d]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (threadIdx.x == 0) p.lse[bh] = acc * p.scale;
}

}  // namespace gaot

// ---- host side: validate, gather the facts, ask attention_plan.h, launch what the plan names
using namespace gaot;
#define ST(s) reinterpret_cast<hipStream_t>(s)

static AttnSwitches g_sw;          // the kernel-selection switches (attention_plan.h) behind the gaot_debug_set_attention_* setters
extern "C" int gaot_debug_set_attention_p_pieces(int n) {
    const int old = g_sw.p_pieces;
    g_sw.p_pieces = (n == 33 || n == 22 || n == 23 || n == 32) ? n : (n == 3 ? 33 : (n == 2 ? 22 : FOLLOW_CALL));
    return old;
}
extern "C" int gaot_debug_set_attention_operand_pieces(int n) { const int old = g_sw.operand_pieces; g_sw.operand_pieces = n == 3 ? 3 : (n == 2 ? 2 : FOLLOW_CALL); return old; }
extern "C" int gaot_debug_set_attention_tr(int on) { const int old = g_sw.tr; g_sw.tr = on != 0; return old; }
extern "C" int gaot_debug_set_attention_qsplit(int on) { const int old = g_sw.qsplit; g_sw.qsplit = on != 0; return old; }
extern "C" int gaot_debug_set_attention_pipe(int on) { const int old = g_sw.pipe; g_sw.pipe = on; return old; }
extern "C" int gaot_debug_set_attention_dh8(int on) { const int old = g_sw.dh8; g_sw.dh8 = on; return old; }
extern "C" int gaot_debug_set_attention_h16(int nw) { const int old = g_sw.h16; g_sw.h16 = nw; return old; }
extern "C" int gaot_debug_set_attention_split(int on) { const int old = (int)g_sw.split; g_sw.split = (AttnSplit)on; return old; }
extern "C" int gaot_debug_set_attention_keysplit(int on) { const int old = (int)g_sw.keysplit; g_sw.keysplit = (AttnKeySplit)on; return old; }

extern "C" int64_t gaot_attention_fwd_workspace(int32_t B, int32_t S, int32_t H, int32_t head_dim) { return attn_fwd_workspace_floats(B, S, H, head_dim, g_sw); }
extern "C" int64_t gaot_attention_bwd_workspace(int32_t B, int32_t S, int32_t H, int32_t head_dim) { return attn_bwd_workspace_floats(B, S, H, head_dim); }

// the four entry points: what each checks of its sizes, in its own words
enum AttnEntry { ENTRY_FWD = 0, ENTRY_FWD_DROPOUT = 1, ENTRY_BWD = 2, ENTRY_BWD_DROPOUT = 3 };
static const char* const ENTRY_NAME[4] = {"attention_fwd", "attention_fwd_dropout", "attention_bwd", "attention_bwd_dropout"};
static int validate(AttnEntry e, bool pointers, int pieces, int B, int S, int H, int Hkv, int head_dim) {
    const char* name = ENTRY_NAME[e];
    GAOT_REQUIRE(pointers, "%s: null pointer", name);
    if (e == ENTRY_FWD || e == ENTRY_BWD) GAOT_REQUIRE(pieces == 0 || (pieces >= 2 && pieces <= 4), "%s: pieces %d not in {0, 2, 3, 4}", name, pieces);
    const bool sizes = B > 0 && S > 0 && H > 0 && Hkv > 0 && H % Hkv == 0;
    if (e == ENTRY_FWD || e == ENTRY_FWD_DROPOUT) GAOT_REQUIRE(sizes, "%s: bad sizes B=%d S=%d H=%d Hkv=%d", name, B, S, H, Hkv);
    else GAOT_REQUIRE(sizes, "%s: bad sizes", name);
    GAOT_REQUIRE(head_dim > 0 && head_dim <= 256, "%s: head_dim %d not in 1..256", name, head_dim);
    return GAOT_OK;
}

static void fill_common(AttnArgs& a, const float* q, const float* k, const float* v, int64_t ldq, int64_t ldk, int64_t ldv,
                        int B, int S, int H, int Hkv, int D) {
    a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
    a.B = B; a.S = S; a.H = H; a.Hkv = Hkv; a.D = D;
    a.scale = 1.0f / sqrtf((float)D);
    a.vec = (D % 4 == 0) && (ldq % 4 == 0) && (ldk % 4 == 0) && (ldv % 4 == 0) && aligned16(q) && aligned16(k) && aligned16(v);
}
static void fill_backward(AttnArgs& a, const float* o, const float* dout, int64_t ldo, const float* lse, float* dq, float* dk, float* dv,
                          int64_t lddq, int64_t lddk, int64_t lddv) {
    a.vec = a.vec && (ldo % 4 == 0) && aligned16(dout);
    a.oin = o; a.dout = dout; a.ldo = ldo; a.lse = const_cast<float*>(lse);
    a.dq = dq; a.dk = dk; a.dv = dv; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
}
static int fill_dropout(AttnArgs& a, float p_drop, const uint64_t* seed) {
    GAOT_REQUIRE(p_drop > 0.f && p_drop < 1.f && seed, "attention dropout: need 0 < p < 1 and a device seed word");
    a.drop_seed = reinterpret_cast<const unsigned long long*>(seed);
    const double keep = 1.0 - (double)p_drop;
    a.drop_thresh = (unsigned)(keep * 4294967296.0 >= 4294967295.0 ? 4294967295.0 : keep * 4294967296.0);
    a.drop_scale = (float)(1.0 / keep);
    return GAOT_OK;
}

// the facts of a filled argument block (the one place where pointers become booleans)
static AttnFacts gather_facts(const AttnArgs& a, AttnDir dir, bool dropout, int pieces, const float* workspace) {
    AttnFacts f = {};
    f.B = a.B; f.S = a.S; f.H = a.H; f.Hkv = a.Hkv; f.D = a.D;
    f.dir = dir; f.dropout = dropout; f.pieces = pieces;
    f.has_qkv_absmax = a.qkv_amax != nullptr; f.has_dout_absmax = a.dout_amax != nullptr; f.has_dqkv_absmax = a.dqkv_amax != nullptr;
    f.vec = a.vec;
    f.ldo4 = a.ldo % 4 == 0;
    f.has_workspace = workspace != nullptr; f.ws_aligned = aligned16(workspace);
    if (dir == AttnDir::Forward) { f.o_aligned = aligned16(a.o); return f; }
    f.o_aligned = aligned16(a.oin);
    f.dq_aligned = aligned16(a.dq); f.dk_aligned = aligned16(a.dk); f.dv_aligned = aligned16(a.dv);
    f.lddq4 = a.lddq % 4 == 0; f.lddk4 = a.lddk % 4 == 0; f.lddv4 = a.lddv % 4 == 0;
    f.dq_part_aligned = aligned16(workspace + attn_bwd_layout(a.B, a.S, a.H, a.D).dq_part);
    return f;
}

static thread_local AttnPlan t_last_plan[2];       // what this thread's last forward / backward launch executed
static thread_local bool t_has_plan[2];

// a kernel whose dynamic LDS exceeds the default limit: raise the limit once per kernel
template <int DP, bool DROP> static void allow_bwd_lds() {
    static bool attr_set = false;
    if (!attr_set) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_kernel<DP, DROP>), hipFuncAttributeMaxDynamicSharedMemorySize, attn_bwd_lds_bytes(DP));
        attr_set = true;
    }
}

// template arguments of a plan as one switch label
static constexpr long tkey(int a, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0) { return (((((long)a * 256 + b) * 256 + c) * 256 + d) * 256 + e) * 256 + f; }
#define MAIN(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(p.grid), dim3(p.block), p.lds_bytes, ST(stream), a)
#define ON(key, ...) case key: MAIN(__VA_ARGS__); break

static int attention_forward(AttnArgs& a, const AttnFacts& f, float* workspace, const char* name, gaot_stream_t stream) {
    const AttnPlan p = plan_attention(f, g_sw);
    t_last_plan[0] = p; t_has_plan[0] = true;
    if (p.ks == 2) { a.o_part = workspace + p.o_part; a.lse_part = workspace + p.lse_part; }
    bool found = true;
    switch (p.family) {
        case AttnFamily::OneKey: MAIN(attn_fwd_one_key_kernel); break;
        case AttnFamily::Wide: attn_wide_fwd_launch(a, p.drop, ST(stream)); break;
        case AttnFamily::Split:
            switch (tkey(p.nw, p.dh, p.pp, p.op, p.f16, p.ks)) {
                ON(tkey(8, 32, 2, 2, 1, 2), attn_fwd_split_kernel<8, 32, 2, 2, true, 2>);
                ON(tkey(8, 64, 2, 2, 1, 2), attn_fwd_split_kernel<8, 64, 2, 2, true, 2>);
                ON(tkey(8, 32, 2, 2, 1, 1), attn_fwd_split_kernel<8, 32, 2, 2, true>);
                ON(tkey(8, 32, 3, 3, 0, 1), attn_fwd_split_kernel<8, 32, 3>);
                ON(tkey(8, 32, 2, 3, 0, 1), attn_fwd_split_kernel<8, 32, 2>);
                ON(tkey(8, 32, 2, 2, 0, 1), attn_fwd_split_kernel<8, 32, 2, 2>);
                ON(tkey(4, 32, 2, 2, 1, 1), attn_fwd_split_kernel<4, 32, 2, 2, true>);
                ON(tkey(4, 32, 3, 3, 0, 1), attn_fwd_split_kernel<4, 32, 3>);
                ON(tkey(4, 32, 2, 3, 0, 1), attn_fwd_split_kernel<4, 32, 2>);
                ON(tkey(4, 32, 2, 2, 0, 1), attn_fwd_split_kernel<4, 32, 2, 2>);
                ON(tkey(8, 64, 2, 2, 1, 1), attn_fwd_split_kernel<8, 64, 2, 2, true>);
                ON(tkey(4, 64, 2, 2, 1, 1), attn_fwd_split_kernel<4, 64, 2, 2, true>);
                ON(tkey(8, 64, 2, 2, 0, 1), attn_fwd_split_kernel<8, 64, 2, 2>);
                ON(tkey(8, 64, 3, 3, 0, 1), attn_fwd_split_kernel<8, 64>);
                ON(tkey(4, 64, 2, 2, 0, 1), attn_fwd_split_kernel<4, 64, 2, 2>);
                ON(tkey(4, 64, 3, 3, 0, 1), attn_fwd_split_kernel<4, 64>);
                default: found = false;
            }
            break;
        case AttnFamily::Pipe: MAIN(attn_fwd_split_pipe_kernel<0>); break;
        case AttnFamily::Glds: MAIN(attn_fwd_glds_kernel); break;
        case AttnFamily::Fp32:
            switch (tkey(p.dh, p.drop)) {
                ON(tkey(32, 0), attn_fwd_kernel<32>);
                ON(tkey(64, 0), attn_fwd_kernel<64>);
                ON(tkey(128, 0), attn_fwd_kernel<128>);
                ON(tkey(32, 1), attn_fwd_kernel<32, true>);
                ON(tkey(64, 1), attn_fwd_kernel<64, true>);
                ON(tkey(128, 1), attn_fwd_kernel<128, true>);
                default: found = false;
            }
            break;
        default: found = false;
    }
    GAOT_REQUIRE(found, "%s: no kernel for the plan (family %d)", name, (int)p.family);
    if (p.combine_grid) hipLaunchKernelGGL(attn_fwd_combine_kernel, dim3(p.combine_grid), dim3(256), 0, ST(stream), a);
    GAOT_CHECK_LAUNCH(p.ks == 2 ? "gaot_attention_fwd_ws" : name);
    return GAOT_OK;
}

static int attention_backward(AttnArgs& a, const AttnFacts& f, float* workspace, const char* name, gaot_stream_t stream) {
    const AttnPlan p = plan_attention(f, g_sw);
    t_last_plan[1] = p; t_has_plan[1] = true;
    a.delta = workspace + p.delta_off;
    a.dq_part = workspace + p.dq_part;
    a.n_kblocks = p.n_kblocks;
    if (p.qs == 2) { a.dk2 = workspace + p.dk2; a.dv2 = workspace + p.dv2; }
    if (p.delta == AttnDelta::Vector) hipLaunchKernelGGL(attn_delta_vec_kernel, dim3(p.delta_grid), dim3(256), 0, ST(stream), a, 8);
    else if (p.delta == AttnDelta::Scalar) hipLaunchKernelGGL(attn_delta_kernel, dim3(p.delta_grid), dim3(256), 0, ST(stream), a);
    bool found = true;
    switch (p.family) {
        case AttnFamily::Wide: attn_wide_bwd_launch(a, p.drop, ST(stream)); break;
        case AttnFamily::BwdSplit8:
            switch (tkey(p.pp, p.op, p.tr, p.f16, p.qs)) {
                ON(tkey(2, 2, 1, 1, 2), attn_bwd_split8_kernel<2, 2, true, true, 2>);
                ON(tkey(2, 2, 1, 1, 1), attn_bwd_split8_kernel<2, 2, true, true>);
                ON(tkey(3, 3, 0, 0, 1), attn_bwd_split8_kernel<3>);
                ON(tkey(2, 3, 0, 0, 1), attn_bwd_split8_kernel<2>);
                ON(tkey(2, 2, 1, 0, 1), attn_bwd_split8_kernel<2, 2, true>);
                ON(tkey(2, 2, 0, 0, 1), attn_bwd_split8_kernel<2, 2>);
                default: found = false;
            }
            break;
        case AttnFamily::BwdH16:
            switch (tkey(p.nw, p.qs, p.var)) {
                ON(tkey(4, 1, 0), attn_bwd_h16_kernel<4>);
                ON(tkey(8, 1, 1), attn_bwd_h16_kernel<8, 1, 1>);
                ON(tkey(8, 1, 2), attn_bwd_h16_kernel<8, 1, 2>);
                ON(tkey(8, 1, 3), attn_bwd_h16_kernel<8, 1, 3>);
                ON(tkey(8, 1, 0), attn_bwd_h16_kernel<8>);
                default: found = false;
            }
            break;
        case AttnFamily::BwdSplit4: MAIN(attn_bwd_split_kernel); break;
        case AttnFamily::BwdSplit8Dh:
            switch (tkey(p.f16, p.qs)) {
                ON(tkey(1, 1), attn_bwd_split8_dh_kernel<true, 1>);
                ON(tkey(1, 2), attn_bwd_split8_dh_kernel<true, 2>);
                ON(tkey(0, 1), attn_bwd_split8_dh_kernel<false, 1>);
                default: found = false;
            }
            break;
        case AttnFamily::BwdSplitDh:
            switch (tkey(p.dh, p.pp, p.op, p.f16)) {
                ON(tkey(64, 2, 2, 1), attn_bwd_split_dh_kernel<64, 2, 2, true>);
                ON(tkey(64, 2, 2, 0), attn_bwd_split_dh_kernel<64, 2, 2>);
                ON(tkey(64, 3, 3, 0), attn_bwd_split_dh_kernel<64>);
                default: found = false;
            }
            break;
        case AttnFamily::Fp32:
            switch (tkey(p.dh, p.drop)) {
                ON(tkey(32, 0), attn_bwd_kernel<32>);
                case tkey(64, 0): allow_bwd_lds<64, false>(); MAIN(attn_bwd_kernel<64>); break;
                case tkey(128, 0): allow_bwd_lds<128, false>(); MAIN(attn_bwd_kernel<128>); break;
                ON(tkey(32, 1), attn_bwd_kernel<32, true>);
                case tkey(128, 1): allow_bwd_lds<128, true>(); MAIN(attn_bwd_kernel<128, true>); break;
                case tkey(64, 1): allow_bwd_lds<64, true>(); MAIN(attn_bwd_kernel<64, true>); break;
                default: found = false;
            }
            break;
        default: found = false;
    }
    GAOT_REQUIRE(found, "%s: no kernel for the plan (family %d)", name, (int)p.family);
    if (p.add_cols_grid) {
        const int c4 = a.H * a.D / 4;
        hipLaunchKernelGGL(attn_add_cols_kernel, dim3(p.add_cols_grid), dim3(256), 0, ST(stream), a.dk, (long)a.lddk, a.dk2, a.dv, (long)a.lddv, a.dv2, (long)a.B * a.S, c4);
    }
    if (p.reduce == AttnReduce::Vector) {
        const dim3 g(p.reduce_grid);
        switch (p.reduce_dp4) {
            case 8: hipLaunchKernelGGL(attn_dq_reduce_vec_kernel<8>, g, dim3(256), 0, ST(stream), a); break;
            case 16: hipLaunchKernelGGL(attn_dq_reduce_vec_kernel<16>, g, dim3(256), 0, ST(stream), a); break;
            default: hipLaunchKernelGGL(attn_dq_reduce_vec_kernel<32>, g, dim3(256), 0, ST(stream), a); break;
        }
    } else if (p.reduce == AttnReduce::Scalar) {
        hipLaunchKernelGGL(attn_dq_reduce_kernel, dim3(p.reduce_grid), dim3(256), 0, ST(stream), a, attn_padded_dim(a.D));
    }
    GAOT_CHECK_LAUNCH(name);
    if (p.absmax_tensors) {        // dK and dV, with dQ in front where the plan says three
        const gaot_absmax_item it[3] = {{a.dq, a.lddq, a.B * a.S, a.H * a.D, a.dqkv_amax}, {a.dk, a.lddk, a.B * a.S, a.H * a.D, a.dqkv_amax},
                                        {a.dv, a.lddv, a.B * a.S, a.H * a.D, a.dqkv_amax}};
        if (int rc = gaot_absmax_grouped(it + 3 - p.absmax_tensors, p.absmax_tensors, stream)) return rc;
    }
    return GAOT_OK;
}
#undef ON
#undef MAIN

extern "C" int gaot_attention_fwd_ws(const float* q, const float* k, const float* v, int64_t ldq, int64_t ldk, int64_t ldv,
                                     int32_t B, int32_t S, int32_t H, int32_t Hkv, int32_t head_dim, float* o, int64_t ldo,
                                     float* lse, int32_t pieces, const float* qkv_absmax, float* workspace, gaot_stream_t stream) {
    if (int rc = validate(ENTRY_FWD, q && k && v && o && lse, pieces, B, S, H, Hkv, head_dim)) return rc;
    AttnArgs a = {};
    fill_common(a, q, k, v, ldq, ldk, ldv, B, S, H, Hkv, head_dim);
    a.o = o; a.ldo = ldo; a.lse = lse; a.qkv_amax = qkv_absmax;
    return attention_forward(a, gather_facts(a, AttnDir::Forward, false, pieces, workspace), workspace, "gaot_attention_fwd", stream);
}
extern "C" int gaot_attention_fwd(const float* q, const float* k, const float* v, int64_t ldq, int64_t ldk, int64_t ldv,
                                  int32_t B, int32_t S, int32_t H, int32_t Hkv, int32_t head_dim, float* o, int64_t ldo,
                                  float* lse, int32_t pieces, const float* qkv_absmax, gaot_stream_t stream) {
    return gaot_attention_fwd_ws(q, k, v, ldq, ldk, ldv, B, S, H, Hkv, head_dim, o, ldo, lse, pieces, qkv_absmax, nullptr, stream);
}

// ---- attention dropout: seed bookkeeping on the device (graph-replay safe: nothing about the seed is a launch argument)
// state = (seed, counter).  used[0] = seed mixed with counter and salt; counter += 1.
__global__ void attn_seed_next_kernel(unsigned long long* state, unsigned long long salt, unsigned long long* used) {
    unsigned long long x = state[0] + 0x9e3779b97f4a7c15ull * (state[1] + 1) + salt;
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    used[0] = x;
    state[1] += 1;
}

extern "C" int gaot_attention_seed_next(uint64_t* state, uint64_t salt, uint64_t* used, gaot_stream_t stream) {
    GAOT_REQUIRE(state && used, "attention_seed_next: null pointer");
    hipLaunchKernelGGL(attn_seed_next_kernel, dim3(1), dim3(1), 0, ST(stream), reinterpret_cast<unsigned long long*>(state),
                       (unsigned long long)salt, reinterpret_cast<unsigned long long*>(used));
    GAOT_CHECK_LAUNCH("gaot_attention_seed_next");
    return GAOT_OK;
}

extern "C" int gaot_attention_fwd_dropout(const float* q, const float* k, const float* v, int64_t ldq, int64_t ldk, int64_t ldv,
                                          int32_t B, int32_t S, int32_t H, int32_t Hkv, int32_t head_dim, float* o, int64_t ldo,
                                          float* lse, float p_drop, const uint64_t* seed, gaot_stream_t stream) {
    if (int rc = validate(ENTRY_FWD_DROPOUT, q && k && v && o && lse, 0, B, S, H, Hkv, head_dim)) return rc;
    AttnArgs a = {};
    fill_common(a, q, k, v, ldq, ldk, ldv, B, S, H, Hkv, head_dim);
    a.o = o; a.ldo = ldo; a.lse = lse;
    if (int rc = fill_dropout(a, p_drop, seed)) return rc;
    return attention_forward(a, gather_facts(a, AttnDir::Forward, true, 0, nullptr), nullptr, "gaot_attention_fwd_dropout", stream);
}

extern "C" int gaot_attention_bwd_dropout(const float* q, const float* k, const float* v, int64_t ldq, int64_t ldk, int64_t ldv,
                                          const float* o, const float* dout, int64_t ldo, const float* lse, int32_t B, int32_t S,
                                          int32_t H, int32_t Hkv, int32_t head_dim, float* dq, float* dk, float* dv, int64_t lddq,
                                          int64_t lddk, int64_t lddv, float* workspace, float p_drop, const uint64_t* seed,
                                          gaot_stream_t stream) {
    if (int rc = validate(ENTRY_BWD_DROPOUT, q && k && v && o && dout && lse && dq && dk && dv && workspace, 0, B, S, H, Hkv, head_dim)) return rc;
    AttnArgs a = {};
    fill_common(a, q, k, v, ldq, ldk, ldv, B, S, H, Hkv, head_dim);
    fill_backward(a, o, dout, ldo, lse, dq, dk, dv, lddq, lddk, lddv);
    if (int rc = fill_dropout(a, p_drop, seed)) return rc;
    return attention_backward(a, gather_facts(a, AttnDir::Backward, true, 0, workspace), workspace, "gaot_attention_bwd_dropout", stream);
}

extern "C" int gaot_attention_bwd(const float* q, const float* k, const float* v, int64_t ldq, int64_t ldk, int64_t ldv,
                                  const float* o, const float* dout, int64_t ldo, const float* lse, int32_t B, int32_t S,
                                  int32_t H, int32_t Hkv, int32_t head_dim, float* dq, float* dk, float* dv, int64_t lddq,
                                  int64_t lddk, int64_t lddv, float* workspace, int32_t pieces, const float* qkv_absmax,
                                  const float* dout_absmax, float* dqkv_absmax, gaot_stream_t stream) {
    if (int rc = validate(ENTRY_BWD, q && k && v && o && dout && lse && dq && dk && dv && workspace, pieces, B, S, H, Hkv, head_dim)) return rc;
    AttnArgs a = {};
    fill_common(a, q, k, v, ldq, ldk, ldv, B, S, H, Hkv, head_dim);
    fill_backward(a, o, dout, ldo, lse, dq, dk, dv, lddq, lddk, lddv);
    a.qkv_amax = qkv_absmax; a.dout_amax = dout_absmax; a.dqkv_amax = dqkv_absmax;
    return attention_backward(a, gather_facts(a, AttnDir::Backward, false, pieces, workspace), workspace, "gaot_attention_bwd", stream);
}

// ---- the plan as numbers (include/gaot_hip_debug.h lists the columns)
static void plan_columns(const AttnPlan& p, int64_t out[GAOT_ATTENTION_PLAN_COLUMNS]) {
    const int64_t cols[GAOT_ATTENTION_PLAN_COLUMNS] = {
        (int)p.delta, p.delta_grid, (int)p.family, p.nw, p.dh, p.pp, p.op, p.f16, p.ks, p.tr, p.qs, p.var, p.drop, p.grid, p.block, p.lds_bytes,
        p.keys_per_wg, p.n_kblocks, p.combine_grid, p.add_cols_grid, (int)p.reduce, p.reduce_dp4, p.reduce_grid, p.absmax_tensors,
        p.o_part, p.lse_part, p.delta_off, p.dq_part, p.dk2, p.dv2, p.workspace_floats};
    for (int i = 0; i < GAOT_ATTENTION_PLAN_COLUMNS; ++i) out[i] = cols[i];
}

extern "C" int gaot_debug_attention_plan(const gaot_debug_attention_query* c, int64_t out[GAOT_ATTENTION_PLAN_COLUMNS]) {
    GAOT_REQUIRE(c != nullptr && out != nullptr, "attention_plan: null pointer");
    GAOT_REQUIRE((c->direction == 0 || c->direction == 1) && (c->dropout == 0 || c->dropout == 1), "attention_plan: direction %d, dropout %d not 0 / 1", c->direction, c->dropout);
    const bool fwd = c->direction == 0, dropout = c->dropout != 0;
    if (int rc = validate((AttnEntry)(2 * c->direction + c->dropout), true, c->pieces, c->B, c->S, c->H, c->Hkv, c->head_dim)) return rc;
    auto bit = [&](uint32_t b) { return (c->facts & b) != 0; };
    AttnFacts f = {};
    f.B = c->B; f.S = c->S; f.H = c->H; f.Hkv = c->Hkv; f.D = c->head_dim;
    f.dir = fwd ? AttnDir::Forward : AttnDir::Backward; f.dropout = dropout; f.pieces = dropout ? 0 : c->pieces;
    f.has_qkv_absmax = !dropout && bit(GAOT_ATTN_FACT_QKV_ABSMAX);
    f.has_dout_absmax = !dropout && !fwd && bit(GAOT_ATTN_FACT_DOUT_ABSMAX);
    f.has_dqkv_absmax = !dropout && !fwd && bit(GAOT_ATTN_FACT_DQKV_ABSMAX);
    f.vec = c->head_dim % 4 == 0 && bit(GAOT_ATTN_FACT_VEC);
    f.o_aligned = bit(GAOT_ATTN_FACT_O_ALIGNED); f.ldo4 = bit(GAOT_ATTN_FACT_LDO4);
    f.has_workspace = (!fwd || !dropout) && bit(GAOT_ATTN_FACT_WORKSPACE); f.ws_aligned = bit(GAOT_ATTN_FACT_WS_ALIGNED);
    f.dq_aligned = bit(GAOT_ATTN_FACT_DQ_ALIGNED); f.dk_aligned = bit(GAOT_ATTN_FACT_DK_ALIGNED); f.dv_aligned = bit(GAOT_ATTN_FACT_DV_ALIGNED);
    f.lddq4 = bit(GAOT_ATTN_FACT_LDDQ4); f.lddk4 = bit(GAOT_ATTN_FACT_LDDK4); f.lddv4 = bit(GAOT_ATTN_FACT_LDDV4);
    f.dq_part_aligned = bit(GAOT_ATTN_FACT_DQ_PART_ALIGNED);
    plan_columns(plan_attention(f, g_sw), out);
    return GAOT_OK;
}

extern "C" int gaot_debug_last_attention_plan(int direction, int64_t out[GAOT_ATTENTION_PLAN_COLUMNS]) {
    GAOT_REQUIRE(out != nullptr && (direction == 0 || direction == 1), "last_attention_plan: null output or direction %d not 0 / 1", direction);
    if (t_has_plan[direction]) plan_columns(t_last_plan[direction], out);
    else for (int i = 0; i < GAOT_ATTENTION_PLAN_COLUMNS; ++i) out[i] = -1;      // no launch on this thread yet
    return GAOT_OK;
}
