// Softmax attention for 128 < head_dim <= 256: forward and backward in exact fp32 on v_mfma_f32_32x32x2_f32, as the
// fp32-MFMA kernels of attention.hip, with the HEAD DIMENSION split over the four waves of a workgroup: wave w owns the
// d columns [64 w, 64 w + 64) of the padded head (WIDE_DP = 256; columns past head_dim are zero-filled on load and never stored).
//
//   forward : a workgroup owns 64 queries (two 32-query tiles).  Per 32-key tile every wave forms its partial S^T over its 64 columns
//             (32 MFMAs per query tile, its Q slice in 2 x 32 registers); the four partials are exchanged through LDS and summed in
//             the fixed order ((w0 + w1) + w2) + w3 by every wave, so all four hold bit-identical scores, run the online softmax
//             redundantly (and draw the identical dropout mask), and accumulate O^T[their 64 d][q] with no further exchange.
//   backward: two passes with the same d split and the same fixed-order LDS sum of the partial S and dP.
//             dK / dV (key-stationary): a workgroup owns WIDE_KB keys and walks the 32-query tiles; each wave holds the full P and
//             dS and keeps only its d slice of K, V (operands) and dK, dV (accumulators).
//             dQ (query-stationary): a workgroup owns 64 queries and walks the key tiles as the forward does; S^T and dP^T have
//             the query on the lane, so dS^T feeds dQ^T += K^T dS^T from registers and dQ is written once: no partial sums in
//             memory, no workspace beyond delta.
//             (A single pass that also keeps the K slice as the dQ operand and the dQ accumulators needs 320 persistent registers
//             per lane next to the staging and score registers: as compiled it spilled 540 bytes per lane, so it is not built.)
// No atomics anywhere and every reduction order is fixed: results are bit-reproducible run to run.
#include "attention_common.h"

namespace gaot {

namespace {

constexpr int WLDT = WIDE_DP + 4;      // LDS row stride of a staged [32][256] tile (floats): 16-byte rows, ds_read_b128 conflict-free

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------
// forward: workgroup = 4 waves (d slices) x 64 queries; key/value tiles of 32 rows staged through LDS
// ---------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256) void attn_wide_fwd_kernel(const AttnArgs p) {
    constexpr int QT = 2;                              // 32-query tiles per workgroup
    constexpr int KT = 32;                             // keys per staged tile
    constexpr int NF4 = KT * WIDE_DP / 4 / 256;        // float4 per thread per operand tile (8)
    __shared__ __attribute__((aligned(16))) float smem[2 * KT * WLDT + 4 * QT * 16 * 64];
    float* Ks = smem;
    float* Vs = smem + KT * WLDT;
    float* Xs = smem + 2 * KT * WLDT;                  // partial scores [wave][query tile][16 r][64 lanes]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int dw = 64 * wave;                          // first d column of this wave
    int bh, blk;
    xcd_group_decode(blockIdx.x, p.B * p.H, (p.S + 32 * QT - 1) / (32 * QT), bh, blk);      // query blocks of one (b, h) share K / V: same XCD
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int q0 = blk * 32 * QT;
    const int D = p.D;
    const bool vec = p.vec != 0;
    const float c = p.scale * LOG2E;

    // Q^T operand slice: lane (q = li, half lh) keeps Q[q][dw + 8g + 4lh + s]
    float qreg[QT][32];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int qi = q0 + 32 * t + li;
        const float* qrow = p.q + ((long)b * p.S + qi) * p.ldq + (long)h * D;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 v = load4(qrow, dw + 8 * g + 4 * lh, D, qi < p.S, vec);
            qreg[t][4 * g + 0] = v[0]; qreg[t][4 * g + 1] = v[1]; qreg[t][4 * g + 2] = v[2]; qreg[t][4 * g + 3] = v[3];
        }
    }
    f32x16 oacc[QT][2];
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        m_run[t] = -INFINITY; l_run[t] = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[t][u][r] = 0.f;
    }

    const float* kbase = p.k + (long)b * p.S * p.ldk + (long)hk * D;
    const float* vbase = p.v + (long)b * p.S * p.ldv + (long)hk * D;
    f32x4 rk[NF4], rv[NF4];
    auto fetch = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            const int row = t / (WIDE_DP / 4), d = (t % (WIDE_DP / 4)) * 4;
            const bool ok = kv0 + row < p.S;
            rk[i] = load4(kbase + (long)(kv0 + row) * p.ldk, d, D, ok, vec);
            rv[i] = load4(vbase + (long)(kv0 + row) * p.ldv, d, D, ok, vec);
        }
    };
    const int ntiles = (p.S + KT - 1) / KT;
    fetch(0);
    for (int kt = 0; kt < ntiles; ++kt) {
        const int kvs = kt * KT;
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            const int row = t / (WIDE_DP / 4), d = (t % (WIDE_DP / 4)) * 4;
            *reinterpret_cast<f32x4*>(Ks + row * WLDT + d) = rk[i];
            *reinterpret_cast<f32x4*>(Vs + row * WLDT + d) = rv[i];
        }
        __syncthreads();                                    // barrier A: the tile is staged
        if (kt + 1 < ntiles) fetch(kvs + KT);
        // ---- partial S^T[kv][q] = sum over this wave's 64 columns of K[kv][d] Q[q][d]
        f32x16 s[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
        {
            const float* krow = Ks + li * WLDT + dw + 4 * lh;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(krow + 8 * g);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int t = 0; t < QT; ++t)
                        s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[u], qreg[t][4 * g + u], s[t], 0, 0, 0);
            }
        }
        // ---- exchange: every wave sums the four partials in wave order (identical bits in all four)
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[((wave * QT + t) * 16 + r) * 64 + lane] = s[t][r];
        __syncthreads();                                    // barrier B
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* x = Xs + (t * 16 + r) * 64 + lane;
                s[t][r] = ((x[0] + x[QT * 1024]) + x[2 * QT * 1024]) + x[3 * QT * 1024];
            }
        // ---- online softmax per query tile over the key rows this lane holds (16) + the other half-wave (16)
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kvs + crow(r, lh) >= p.S) s[t][r] = -INFINITY;
                mx = fmaxf(mx, s[t][r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run[t], mx);
            const float alpha = exp2f((m_run[t] - m_new) * c);
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[t][r] = exp2f((s[t][r] - m_new) * c); ps += s[t][r]; }
            ps += __shfl_xor(ps, 32, 64);
            l_run[t] = l_run[t] * alpha + ps;
            m_run[t] = m_new;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[t][u][r] *= alpha;
            if (DROP) {      // the row sum above is of the undropped probabilities (softmax first, dropout on its output)
                const unsigned long long seed = *p.drop_seed;
                const long base = (((long)b * p.H + h) * p.S + (q0 + 32 * t + li)) * p.S + kvs;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[t][r] *= attn_drop_factor(seed, base + crow(r, lh), p.drop_thresh, p.drop_scale);
            }
        }
        // ---- O^T[d][q] += sum_kv V[kv][d] P^T[kv][q] over this wave's columns (P^T registers are the B operand as they are)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vrow = Vs + crow(r, lh) * WLDT + dw + li;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float a = vrow[32 * u];
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    oacc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s[t][r], oacc[t][u], 0, 0, 0);
            }
        }
        __syncthreads();                                    // barrier C: K / V / Xs may be overwritten
    }
    // ---- epilogue: normalise, transpose O^T through LDS (wave-private [32][65] per query tile, over the K / V tiles), row stores
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const float inv_l = 1.0f / l_run[t];
        float* Os = smem + (wave * QT + t) * 32 * 65;       // 4 * QT * 32 * 65 floats == 2 * KT * WLDT
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) Os[li * 65 + 32 * u + crow(r, lh)] = oacc[t][u][r] * inv_l;
        wave_lds_fence();
        for (int rr = lh; rr < 32; rr += 2) {
            const int qi = q0 + 32 * t + rr;
            if (qi < p.S) {
                float* orow = p.o + ((long)b * p.S + qi) * p.ldo + (long)h * D + dw;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int d = 32 * u + li;
                    if (dw + d < D) orow[d] = Os[rr * 65 + d];
                }
            }
        }
        if (wave == 0 && lh == 0 && q0 + 32 * t + li < p.S)
            p.lse[((long)b * p.H + h) * p.S + q0 + 32 * t + li] = m_run[t] * p.scale + logf(l_run[t]);
    }
}

// ---------------------------------------------------------------------------------------------
// backward, key-stationary pass (dK, dV): workgroup = 4 waves (d slices) x WIDE_KB keys (NJ sub-blocks of 32 per wave; NJ = 1: at
// two, K, V, dK and dV of 64 keys are 256 registers per lane and the kernel spills); loops over query tiles of 32
// ---------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256) void attn_wide_bwd_dkdv_kernel(const AttnArgs p) {
    constexpr int NJ = WIDE_KB / 32;                   // key sub-blocks per wave
    constexpr int NF4 = 32 * WIDE_DP / 4 / 256;        // float4 per thread per 32-row tile (8)
    __shared__ __attribute__((aligned(16))) float smem[2 * 32 * WLDT + 64 + NJ * 4 * 2 * 1024 + 4 * 32 * 33];
    float* Qs = smem;                                  // [32][WLDT]
    float* Gs = Qs + 32 * WLDT;                        // dO tile [32][WLDT]
    float* lse_s = Gs + 32 * WLDT;                     // [32]
    float* del_s = lse_s + 32;                         // [32]
    float* Xs = del_s + 32;                            // partial S | dP: [sub-block][wave][2][16 r][64 lanes]
    float* Sw = Xs + NJ * 4 * 2 * 1024;                // per wave transpose staging of the epilogue [32][33]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int dw = 64 * wave;
    int bh, kblk;
    xcd_group_decode(blockIdx.x, p.B * p.H, p.n_kblocks, bh, kblk);     // key blocks of one (b,h) share Q / dO: same XCD
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int kv0 = kblk * WIDE_KB;
    const int D = p.D;
    const bool vec = p.vec != 0;
    const float c = p.scale * LOG2E;
    float* Smine = Sw + wave * 32 * 33;
    const int nj = kv0 + 32 < p.S ? NJ : 1;            // a ragged last block may hold one sub-block only (workgroup-uniform)

    // K^T / V^T operand slices of this lane's key (column li): K[kv][dw + 8g + 4lh + s]
    float kreg[NJ][32], vreg[NJ][32];
    bool kv_ok[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int key = kv0 + 32 * j + li;
        kv_ok[j] = key < p.S;
        const float* krow = p.k + ((long)b * p.S + key) * p.ldk + (long)hk * D;
        const float* vrow = p.v + ((long)b * p.S + key) * p.ldv + (long)hk * D;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 a = load4(krow, dw + 8 * g + 4 * lh, D, kv_ok[j], vec);
            const f32x4 w = load4(vrow, dw + 8 * g + 4 * lh, D, kv_ok[j], vec);
#pragma unroll
            for (int u = 0; u < 4; ++u) { kreg[j][4 * g + u] = a[u]; vreg[j][4 * g + u] = w[u]; }
        }
    }
    f32x16 dvacc[NJ][2], dkacc[NJ][2];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dvacc[j][u][r] = 0.f; dkacc[j][u][r] = 0.f; }

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
            const int row = t / (WIDE_DP / 4), d = (t % (WIDE_DP / 4)) * 4;
            const bool ok = q0 + row < p.S;
            rq[i] = load4(qbase + (long)(q0 + row) * p.ldq, d, D, ok, vec);
            rg[i] = load4(gbase + (long)(q0 + row) * p.ldo, d, D, ok, vec);
        }
        if (tid < 32) {
            const bool ok = q0 + tid < p.S;
            rl = ok ? lse_b[q0 + tid] * LOG2E : INFINITY;   // +inf -> P = 0 for padded queries
            rd = ok ? del_b[q0 + tid] : 0.f;
        }
    };
    const int nq = (p.S + 31) / 32;

    fetch(0);
    for (int qt = 0; qt < nq; ++qt) {
        const int q0 = qt * 32;
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            const int row = t / (WIDE_DP / 4), d = (t % (WIDE_DP / 4)) * 4;
            *reinterpret_cast<f32x4*>(Qs + row * WLDT + d) = rq[i];
            *reinterpret_cast<f32x4*>(Gs + row * WLDT + d) = rg[i];
        }
        if (tid < 32) { lse_s[tid] = rl; del_s[tid] = rd; }
        __syncthreads();                                    // barrier A: the tile is staged
        if (qt + 1 < nq) fetch(q0 + 32);

        // ---- partial S[q][kv] and dP[q][kv] over this wave's 64 columns, per key sub-block
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j < nj) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
                const float* qrow = Qs + li * WLDT + dw + 4 * lh;
                const float* grow = Gs + li * WLDT + dw + 4 * lh;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const f32x4 qa = *reinterpret_cast<const f32x4*>(qrow + 8 * g);
                    const f32x4 ga = *reinterpret_cast<const f32x4*>(grow + 8 * g);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        s = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[u], kreg[j][4 * g + u], s, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[u], vreg[j][4 * g + u], dp, 0, 0, 0);
                    }
                }
                float* x = Xs + ((j * 4 + wave) * 2) * 1024 + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) { x[r * 64] = s[r]; x[1024 + r * 64] = dp[r]; }
            }
        }
        __syncthreads();                                    // barrier B: the partials are exchanged

#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j < nj) {
                // ---- the full S and dP: the four partials added in wave order (identical bits in all four waves)
                f32x16 s, dp;
                const float* x = Xs + (j * 4 * 2) * 1024 + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = x[r * 64]; dp[r] = x[1024 + r * 64]; }
#pragma unroll
                for (int w = 1; w < 4; ++w)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { s[r] += x[w * 2048 + r * 64]; dp[r] += x[w * 2048 + 1024 + r * 64]; }
                // ---- P = exp(S*scale - lse), dS = P * (dP - delta)   (rows q = crow(r,lh), column kv = li)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qr = crow(r, lh);
                    float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse_s[qr]));
                    if (!kv_ok[j]) pv = 0.f;
                    if (DROP) {      // O = (P o M) V: dV takes P o M, dS = P o (M o dP - delta); delta = rowsum(dO o O) as without dropout
                        const float m = attn_drop_factor(*p.drop_seed, (((long)b * p.H + h) * p.S + (q0 + qr)) * p.S + kv0 + 32 * j + li,
                                                         p.drop_thresh, p.drop_scale);
                        s[r] = pv * m;
                        dp[r] = pv * (dp[r] * m - del_s[qr]);
                    } else {
                        s[r] = pv;
                        dp[r] = pv * (dp[r] - del_s[qr]);
                    }
                }
                // ---- dV^T[d][kv] += dO^T[d][q] P[q][kv] ; dK^T[d][kv] += Q^T[d][q] dS[q][kv]   (this wave's d columns)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* grow = Gs + crow(r, lh) * WLDT + dw + li;
                    const float* qrow = Qs + crow(r, lh) * WLDT + dw + li;
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        dvacc[j][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[32 * u], s[r], dvacc[j][u], 0, 0, 0);
                        dkacc[j][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[32 * u], dp[r], dkacc[j][u], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                                    // barrier C: Q / dO / Xs may be overwritten
    }
    // ---- epilogue: dK^T, dV^T -> [kv][d] through wave-private LDS, row stores (per QUERY head h)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int r = 0; r < 16; ++r) Smine[li * 33 + crow(r, lh)] = (pass == 0 ? dkacc[j][u][r] * p.scale : dvacc[j][u][r]);
                wave_lds_fence();
                for (int rr = lh; rr < 32; rr += 2) {
                    const int kv = kv0 + 32 * j + rr;
                    const int d = dw + 32 * u + li;
                    if (kv < p.S && d < D) {
                        if (pass == 0) p.dk[((long)b * p.S + kv) * p.lddk + (long)h * D + d] = Smine[rr * 33 + li];
                        else           p.dv[((long)b * p.S + kv) * p.lddv + (long)h * D + d] = Smine[rr * 33 + li];
                    }
                }
                wave_lds_fence();
            }
}

// ---------------------------------------------------------------------------------------------
// backward, query-stationary pass (dQ): workgroup = 4 waves (d slices) x 64 queries, key/value tiles of 32 rows through LDS as in
// the forward.  S^T and dP^T have the query on the lane, so dS^T is the B operand of dQ^T[d][q] += K^T[d][kv] dS^T[kv][q] as it
// stands: no transposition, no partial sums in memory, dQ is written once.
// ---------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256) void attn_wide_bwd_dq_kernel(const AttnArgs p) {
    constexpr int QT = 2;
    constexpr int KT = 32;
    constexpr int NF4 = KT * WIDE_DP / 4 / 256;
    __shared__ __attribute__((aligned(16))) float smem[2 * KT * WLDT + 4 * QT * 2 * 1024];
    float* Ks = smem;
    float* Vs = smem + KT * WLDT;
    float* Xs = smem + 2 * KT * WLDT;                  // partial S^T | dP^T: [wave][query tile][2][16 r][64 lanes]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int dw = 64 * wave;
    int bh, blk;
    xcd_group_decode(blockIdx.x, p.B * p.H, (p.S + 32 * QT - 1) / (32 * QT), bh, blk);
    const int b = bh / p.H, h = bh % p.H, hk = h / (p.H / p.Hkv);
    const int q0 = blk * 32 * QT;
    const int D = p.D;
    const bool vec = p.vec != 0;
    const float c = p.scale * LOG2E;

    // Q^T and dO^T operand slices: lane (q = li, half lh) keeps Q[q][dw + 8g + 4lh + s]; its query's lse (in log2 units) and delta
    float qreg[QT][32], greg[QT][32], lse2[QT], del[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int qi = q0 + 32 * t + li;
        const bool ok = qi < p.S;
        const float* qrow = p.q + ((long)b * p.S + qi) * p.ldq + (long)h * D;
        const float* grow = p.dout + ((long)b * p.S + qi) * p.ldo + (long)h * D;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 v = load4(qrow, dw + 8 * g + 4 * lh, D, ok, vec);
            const f32x4 w = load4(grow, dw + 8 * g + 4 * lh, D, ok, vec);
#pragma unroll
            for (int u = 0; u < 4; ++u) { qreg[t][4 * g + u] = v[u]; greg[t][4 * g + u] = w[u]; }
        }
        lse2[t] = ok ? p.lse[((long)b * p.H + h) * p.S + qi] * LOG2E : INFINITY;       // +inf -> P = 0 for padded queries
        del[t] = ok ? p.delta[((long)b * p.H + h) * p.S + qi] : 0.f;
    }
    f32x16 dqacc[QT][2];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) dqacc[t][u][r] = 0.f;

    const float* kbase = p.k + (long)b * p.S * p.ldk + (long)hk * D;
    const float* vbase = p.v + (long)b * p.S * p.ldv + (long)hk * D;
    f32x4 rk[NF4], rv[NF4];
    auto fetch = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            const int row = t / (WIDE_DP / 4), d = (t % (WIDE_DP / 4)) * 4;
            const bool ok = kv0 + row < p.S;
            rk[i] = load4(kbase + (long)(kv0 + row) * p.ldk, d, D, ok, vec);
            rv[i] = load4(vbase + (long)(kv0 + row) * p.ldv, d, D, ok, vec);
        }
    };
    const int ntiles = (p.S + KT - 1) / KT;
    fetch(0);
    for (int kt = 0; kt < ntiles; ++kt) {
        const int kvs = kt * KT;
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int t = tid + i * 256;
            const int row = t / (WIDE_DP / 4), d = (t % (WIDE_DP / 4)) * 4;
            *reinterpret_cast<f32x4*>(Ks + row * WLDT + d) = rk[i];
            *reinterpret_cast<f32x4*>(Vs + row * WLDT + d) = rv[i];
        }
        __syncthreads();                                    // barrier A: the tile is staged
        if (kt + 1 < ntiles) fetch(kvs + KT);
        // ---- partial S^T[kv][q] = K Q^T and dP^T[kv][q] = V dO^T over this wave's 64 columns
        f32x16 s[QT], dp[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[t][r] = 0.f; dp[t][r] = 0.f; }
        {
            const float* krow = Ks + li * WLDT + dw + 4 * lh;
            const float* vrow = Vs + li * WLDT + dw + 4 * lh;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 ka = *reinterpret_cast<const f32x4*>(krow + 8 * g);
                const f32x4 va = *reinterpret_cast<const f32x4*>(vrow + 8 * g);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[u], qreg[t][4 * g + u], s[t], 0, 0, 0);
                        dp[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[u], greg[t][4 * g + u], dp[t], 0, 0, 0);
                    }
            }
        }
        // ---- exchange: every wave adds the four partials in wave order (identical bits in all four)
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            float* x = Xs + ((wave * QT + t) * 2) * 1024 + lane;
#pragma unroll
            for (int r = 0; r < 16; ++r) { x[r * 64] = s[t][r]; x[1024 + r * 64] = dp[t][r]; }
        }
        __syncthreads();                                    // barrier B
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const float* x = Xs + (t * 2) * 1024 + lane;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[t][r] = x[r * 64]; dp[t][r] = x[1024 + r * 64]; }
#pragma unroll
            for (int w = 1; w < 4; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[t][r] += x[w * QT * 2048 + r * 64]; dp[t][r] += x[w * QT * 2048 + 1024 + r * 64]; }
            // ---- P^T = exp(S^T*scale - lse), dS^T = P^T * (dP^T - delta)   (rows kv = crow(r,lh), column q = li)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float pv = __builtin_amdgcn_exp2f(fmaf(s[t][r], c, -lse2[t]));
                if (kvs + crow(r, lh) >= p.S) pv = 0.f;
                if (DROP) {
                    const float m = attn_drop_factor(*p.drop_seed, (((long)b * p.H + h) * p.S + (q0 + 32 * t + li)) * p.S + kvs + crow(r, lh),
                                                     p.drop_thresh, p.drop_scale);
                    dp[t][r] = pv * (dp[t][r] * m - del[t]);
                } else {
                    dp[t][r] = pv * (dp[t][r] - del[t]);
                }
            }
        }
        // ---- dQ^T[d][q] += sum_kv K[kv][d] dS^T[kv][q] over this wave's columns
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* krow = Ks + crow(r, lh) * WLDT + dw + li;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float a = krow[32 * u];
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    dqacc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dp[t][r], dqacc[t][u], 0, 0, 0);
            }
        }
        __syncthreads();                                    // barrier C: K / V / Xs may be overwritten
    }
    // ---- epilogue: scale, transpose dQ^T through LDS (wave-private [32][65] per query tile, over the K / V tiles), row stores
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float* Os = smem + (wave * QT + t) * 32 * 65;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) Os[li * 65 + 32 * u + crow(r, lh)] = dqacc[t][u][r] * p.scale;
        wave_lds_fence();
        for (int rr = lh; rr < 32; rr += 2) {
            const int qi = q0 + 32 * t + rr;
            if (qi < p.S) {
                float* drow = p.dq + ((long)b * p.S + qi) * p.lddq + (long)h * D + dw;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int d = 32 * u + li;
                    if (dw + d < D) drow[d] = Os[rr * 65 + d];
                }
            }
        }
    }
}

}  // namespace

void attn_wide_fwd_launch(const AttnArgs& a, bool dropout, hipStream_t stream) {
    const dim3 grid(cdiv(a.S, 64) * a.B * a.H), block(256);
    if (dropout) hipLaunchKernelGGL(attn_wide_fwd_kernel<true>, grid, block, 0, stream, a);
    else         hipLaunchKernelGGL(attn_wide_fwd_kernel<false>, grid, block, 0, stream, a);
}

void attn_wide_bwd_launch(const AttnArgs& a, bool dropout, hipStream_t stream) {
    AttnArgs w = a;
    w.n_kblocks = cdiv(a.S, WIDE_KB);
    const dim3 gk(w.n_kblocks * a.B * a.H), gq(cdiv(a.S, 64) * a.B * a.H), block(256);
    if (dropout) {
        hipLaunchKernelGGL(attn_wide_bwd_dkdv_kernel<true>, gk, block, 0, stream, w);
        hipLaunchKernelGGL(attn_wide_bwd_dq_kernel<true>, gq, block, 0, stream, w);
    } else {
        hipLaunchKernelGGL(attn_wide_bwd_dkdv_kernel<false>, gk, block, 0, stream, w);
        hipLaunchKernelGGL(attn_wide_bwd_dq_kernel<false>, gq, block, 0, stream, w);
    }
}

}  // namespace gaot
