// Which kernels serve a call of gaot_attention_fwd_ws / gaot_attention_bwd and their dropout twins: the whole launch sequence and the
// workspace layout as one pure function of the call's facts and the debug switches.  Plain C++17: no HIP header, no pointer, no global --
// the launch (attention.hip), the two workspace queries, the dry answer (gaot_debug_attention_plan) and the CPU test that enumerates the
// table (tests/test_attention_plan_cpu.py) all read this one function.
#pragma once
#include <stdint.h>

namespace gaot {

enum class AttnDir { Forward = 0, Backward = 1 };

// ---- what the decision reads of a (validated) call; pointers have become booleans
struct AttnFacts {
    int B, S, H, Hkv, D;
    AttnDir dir;
    bool dropout;
    int pieces;                        // as passed (0 with dropout: those entries have no such argument)
    bool has_qkv_absmax, has_dout_absmax, has_dqkv_absmax;
    bool vec;                          // head_dim % 4 == 0, q / k / v 16-byte aligned with pitches % 4 == 0; backward: ldo % 4 == 0 and dout aligned too
    bool o_aligned;                    // forward: the output; backward: the forward's output handed back
    // forward
    bool ldo4;                         // ldo % 4 == 0
    bool has_workspace, ws_aligned;
    // backward
    bool dq_aligned, dk_aligned, dv_aligned;
    bool lddq4, lddk4, lddv4;          // pitches % 4 == 0
    bool dq_part_aligned;              // workspace + B H S floats (attn_bwd_layout) is 16-byte aligned
};

// ---- the debug switches (include/gaot_hip_debug.h); the setters store their argument, normalised where they always did
enum class AttnSplit : int {           // head_dim <= 64 with 16-byte operands (gaot_debug_set_attention_split)
    Fp32 = 0,                          // fp32-MFMA kernels
    Heuristic = 1,                     // DEFAULT: split-bf16 kernels, 8-wave workgroups when they fill the chip
    EightWave = 2,                     // split with the 8-wave workgroup always
    FourWave = 3,                      // split with the 4-wave workgroup always
};                                     // (any other value: split kernels, 8 waves by the fill rule, none of the shapes reserved for Heuristic)
enum class AttnKeySplit : int { Off = 0, On = 1, Dh32Too = 2 };      // [r6] key-split forward (128 .. 255 blocks of 256 queries x batch x heads, with a workspace); 2 = head_dim 32 too (tests)
// [r6] the fp16-piece backward (256-key blocks, one workgroup per key block), gaot_debug_set_attention_h16: 8 + 16 VAR =
// attn_bwd_h16_kernel<8, 1, VAR> (default VAR 1), 4 = <4>, 0 = attn_bwd_split8_kernel
constexpr int H16_SPLIT8 = 0, H16_FOUR_WAVE = 4, H16_EIGHT_WAVE = 8, H16_DEFAULT = 0x18;
constexpr int FOLLOW_CALL = -1;        // p_pieces / operand_pieces: follow the call's `pieces` argument

struct AttnSwitches {
    AttnSplit split = AttnSplit::Heuristic;
    AttnKeySplit keysplit = AttnKeySplit::On;
    int dh8 = 1;                       // [r6] 32 < head_dim <= 64, fp16 pieces: the 8-wave 256-key backward (query-split at 128 .. 255 blocks); 0 = the 4-wave kernel
    int h16 = H16_DEFAULT;
    // pieces of P (forward) and of P / dS (backward) in the head_dim-32 split kernels, as 10 * forward + backward: 22 = two ROUNDED
    // pieces everywhere (five piece products per P V / dS K product instead of six).  Measured at the bench configuration against the
    // oracle evaluated in float64 (tools/grad_errors.py): output 1.25e-7 with either forward, worst gradient tensor 7.6e-7 (q_proj of the
    // middle layer) with either; the kernel alone is 2.2e-6 off float64 instead of 2.4e-7 on random data -- a rounding error of the
    // probabilities, which sum to one and average out over the keys.  33 / 32 / 23: A/B and tests.
    // -1 (default): follow the call's `pieces` argument (3 -> 33, 2 -> 22); anything else overrides every call (A/B runs, tools)
    int p_pieces = FOLLOW_CALL;
    // pieces of the Q / K / V / dO operands in the same kernels (with two-piece P / dS only): 2 = two rounded pieces, three piece
    // products per k-step in every product of the kernel (forward 11 -> 6 MFMAs per k-step pair, backward 27 -> 15); 3 = exact three-way splits
    int operand_pieces = FOLLOW_CALL;  // -1 (default): follow the call's `pieces` argument
    bool tr = true;                    // the two-piece 8-wave backward takes its transposed operands through transposing LDS reads
    bool qsplit = true;                // the 8-wave fp16-piece backward shares a key block's query tiles between two workgroups when that fills the chip (A/B switch)
    int pipe = 0;                      // 1 = the software-pipelined 8-wave forward for S % 64 == 0 (same speed as the plain one since both keep the
                                       // tile product off the running accumulator: 57.6 vs 58.0 us; kept for tools/attn_ablate.hip and as a tested variant)
};

// ---- the answer
enum class AttnFamily {                // the main kernel; its template parameters in AttnPlan, the rest 0
    OneKey = 0,                        // attn_fwd_one_key_kernel
    Wide = 1,                          // attention_wide.hip, 128 < head_dim <= 256 (drop)
    Fp32 = 2,                          // attn_fwd_kernel / attn_bwd_kernel<dh, drop>
    Glds = 3,                          // attn_fwd_glds_kernel
    Split = 4,                         // attn_fwd_split_kernel<nw, dh, pp, op, f16, ks>
    Pipe = 5,                          // attn_fwd_split_pipe_kernel<0>
    BwdSplit4 = 6,                     // attn_bwd_split_kernel
    BwdSplitDh = 7,                    // attn_bwd_split_dh_kernel<64, pp, op, f16>
    BwdSplit8 = 8,                     // attn_bwd_split8_kernel<pp, op, tr, f16, qs>
    BwdH16 = 9,                        // attn_bwd_h16_kernel<nw, qs, var>
    BwdSplit8Dh = 10,                  // attn_bwd_split8_dh_kernel<f16, qs>
};
enum class AttnDelta { None = 0, Vector = 1, Scalar = 2 };       // None: the forward, or a backward kernel that forms delta itself
enum class AttnReduce { None = 0, Vector = 1, Scalar = 2 };

struct AttnPlan {
    AttnDelta delta; int delta_grid;
    AttnFamily family;
    int nw, dh, pp, op, f16, ks, tr, qs, var, drop;      // template parameters of the family (dh: DP of Fp32, DH of Split / BwdSplitDh)
    int grid, block, lds_bytes;        // of the main kernel (Wide backward: of its dK / dV pass)
    int keys_per_wg;                   // forward: queries per workgroup
    int n_kblocks;                     // AttnArgs::n_kblocks: dQ slabs written (backward)
    int combine_grid;                  // key-split forward: attn_fwd_combine_kernel; 0 = none
    int add_cols_grid;                 // query-split backward: attn_add_cols_kernel; 0 = none
    AttnReduce reduce; int reduce_dp4, reduce_grid;      // dQ slabs -> dQ; the vector kernel's DP4 8 / 16 / 32
    int absmax_tensors;                // the trailing grouped absmax: 0 none, 2 dK dV, 3 dQ dK dV
    // workspace layout in floats from the workspace base; -1 = not used by this plan
    int64_t o_part, lse_part;          // forward
    int64_t delta_off, dq_part, dk2, dv2;      // backward
    int64_t workspace_floats;          // what the caller must provide
};

inline int attn_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
inline int attn_cap_blocks(long n, int per, int cap) { long b = (n + per - 1) / per; return (int)(b > cap ? cap : (b < 1 ? 1 : b)); }
inline int attn_padded_dim(int D) { return D <= 32 ? 32 : (D <= 64 ? 64 : 128); }
// dynamic LDS of attn_bwd_kernel<DP>
inline int attn_bwd_lds_bytes(int DP) { return (int)sizeof(float) * (2 * 32 * (DP + 4) + 64 + 4 * 32 * DP + 4 * 32 * 33 + 4 * 32 * (DP < 64 ? DP : 64)); }

// ---- workspace layouts
// key-split forward: per key half the normalised output [B S][H D] (dense), then its log-sum-exp [B H S]
struct AttnFwdLayout { int64_t o_part, lse_part, total; };
inline AttnFwdLayout attn_fwd_layout(int B, int S, int H, int D) {
    return {0, 2 * (int64_t)B * S * H * D, 2 * ((int64_t)B * S * H * D + (int64_t)B * H * S)};
}
// backward: delta [B H S], then one dQ slab [B H S][DP] per block of 128 keys.  Sized for 128-key blocks even when 256-key kernels run
// (they write half the slabs).  128 < head_dim <= 256: delta only (the dQ pass writes dQ itself)
struct AttnBwdLayout { int64_t delta, dq_part, slab, total; };
inline AttnBwdLayout attn_bwd_layout(int B, int S, int H, int D) {
    const int64_t bhs = (int64_t)B * H * S;
    if (D > 128) return {0, bhs, 0, bhs};
    const int64_t slab = bhs * attn_padded_dim(D);
    return {0, bhs, slab, bhs + (int64_t)attn_cdiv(S, 128) * slab};
}
// the query-split backward puts the second half's dK / dV partials (dense [B S][H DP], one slab each) into the first two slabs the
// 256-key blocks leave unused: there must be two
inline bool attn_two_spare_slabs(int S) { return attn_cdiv(S, 128) - attn_cdiv(S, 256) >= 2; }

// key-split forward (attn_fwd_split_kernel<8, 64, .., KS = 2>): shapes it is for -- 128 .. 255 blocks of 256 queries x batch x heads, at least eight
// key tiles, head_dim 36 .. 64 in steps of 4.  (head_dim 32 stays on the 4-wave kernel, which already runs two workgroups per CU there:
// 4 x 1 024 x 8 x 32 measured 28.7 us against 30.2 with the split; keysplit = 2 forces it on for the tests.)
inline bool attn_fwd_key_split_shape(int B, int S, int H, int D, const AttnSwitches& sw) {
    const long wg8 = (long)attn_cdiv(S, 256) * B * H;
    return sw.keysplit != AttnKeySplit::Off && sw.split == AttnSplit::Heuristic && wg8 >= 128 && wg8 < 256 && attn_cdiv(S, 64) >= 8 &&
           D >= (sw.keysplit == AttnKeySplit::Dh32Too ? 32 : 36) && D <= 64 && D % 4 == 0;
}

// gaot_attention_fwd_workspace: an upper bound -- it answers without knowing whether the call will have fp16 pieces or aligned operands
inline int64_t attn_fwd_workspace_floats(int B, int S, int H, int D, const AttnSwitches& sw) {
    if (B <= 0 || S <= 0 || H <= 0 || D <= 0) return -1;
    return attn_fwd_key_split_shape(B, S, H, D, sw) ? attn_fwd_layout(B, S, H, D).total : 0;
}
// gaot_attention_bwd_workspace
inline int64_t attn_bwd_workspace_floats(int B, int S, int H, int D) { return attn_bwd_layout(B, S, H, D).total; }

inline AttnPlan plan_attention(const AttnFacts& f, const AttnSwitches& sw) {
    const int B = f.B, S = f.S, H = f.H, D = f.D;
    const bool fwd = f.dir == AttnDir::Forward;
    AttnPlan p{};
    p.o_part = p.lse_part = p.delta_off = p.dq_part = p.dk2 = p.dv2 = -1;
    p.block = 256;
    auto on = [&](AttnFamily fam, int grid, int block, int keys) { p.family = fam; p.grid = grid; p.block = block; p.keys_per_wg = keys; };
    const int grid64 = attn_cdiv(S, 64) * B * H, grid128 = attn_cdiv(S, 128) * B * H, grid256 = attn_cdiv(S, 256) * B * H;
    const int DP = attn_padded_dim(D);
    // fp16 pieces where a kernel takes them; else exact
    const bool f16 = !f.dropout && f.pieces == 4 && f.has_qkv_absmax && (fwd || f.has_dout_absmax) && sw.p_pieces < 0 && sw.operand_pieces < 0;
    const int pp = sw.p_pieces >= 0 ? sw.p_pieces : (f.pieces == 2 ? 22 : 33);
    const int op = sw.operand_pieces >= 0 ? sw.operand_pieces : (f.pieces == 2 ? 2 : 3);
    const bool split_on = sw.split != AttnSplit::Fp32;
    const long wg8 = (long)attn_cdiv(S, 256) * B * H;
    // 256-query / 256-key workgroups once they still fill the chip (one per CU): half the K / V tile splits per head
    const bool fill8 = sw.split != AttnSplit::FourWave && (sw.split == AttnSplit::EightWave || wg8 >= 256);

    if (fwd) {
        if (f.dropout) {               // no one-key shortcut, fp32 MFMA only
            if (D > 128) { on(AttnFamily::Wide, grid64, 256, 64); p.drop = 1; }
            else { on(AttnFamily::Fp32, grid128, 256, 128); p.dh = DP; p.drop = 1; }
            return p;
        }
        if (S == 1) {                  // a single key: out = v exactly, every head_dim, every `pieces`
            on(AttnFamily::OneKey, B * H, 64, 1);
            return p;
        }
        if (D > 128) {                 // 128 < head_dim <= 256: fp32 MFMA with the head dimension split over the waves (attention_wide.hip)
            on(AttnFamily::Wide, grid64, 256, 64);
            return p;
        }
        auto split = [&](int nw, int dh, int ppf, int opf, bool h) {
            on(AttnFamily::Split, nw == 8 ? grid256 : grid128, nw == 8 ? 512 : 256, nw == 8 ? 256 : 128);
            p.nw = nw; p.dh = dh; p.pp = ppf; p.op = opf; p.f16 = h; p.ks = 1;
        };
        if (f.has_workspace && f16 && f.vec && f.ws_aligned && f.o_aligned && f.ldo4 && attn_fwd_key_split_shape(B, S, H, D, sw)) {
            const AttnFwdLayout w = attn_fwd_layout(B, S, H, D);
            split(8, D == 32 ? 32 : 64, 2, 2, true);
            p.ks = 2; p.grid = grid256 * 2;
            p.combine_grid = attn_cap_blocks((long)B * S * H * (D / 4), 256, 2048);
            p.o_part = w.o_part; p.lse_part = w.lse_part; p.workspace_floats = w.total;
        }
        else if (D == 32 && f.vec && split_on) {
            const int nw = fill8 ? 8 : 4;
            if (f16) split(nw, 32, 2, 2, true);
            else if (fill8 && S % 64 == 0 && sw.pipe) on(AttnFamily::Pipe, grid256, 512, 256);
            else if (pp / 10 == 3) split(nw, 32, 3, 3, false);
            else if (op == 3) split(nw, 32, 2, 3, false);
            else split(nw, 32, 2, 2, false);
        }
        else if (D > 32 && D <= 64 && f.vec && split_on) {       // (vec: head_dim % 4 == 0): split-bf16 with four d steps
            const bool two64 = pp / 10 == 2 && op == 2;          // two rounded pieces of everything, or exact splits
            const int nw = fill8 ? 8 : 4;
            if (f16) split(nw, 64, 2, 2, true);
            else if (two64) split(nw, 64, 2, 2, false);
            else split(nw, 64, 3, 3, false);
        }
        else if (D == 32 && f.vec) on(AttnFamily::Glds, grid128, 256, 128);
        else { on(AttnFamily::Fp32, grid128, 256, 128); p.dh = DP; }      // 64 < head_dim <= 128: fp32 MFMA, one wave per SIMD
        return p;
    }

    // ---- backward
    const AttnBwdLayout w = attn_bwd_layout(B, S, H, D);
    p.delta_off = w.delta; p.dq_part = w.dq_part; p.workspace_floats = w.total;
    p.n_kblocks = attn_cdiv(S, 128);
    const int delta_vec_grid = attn_cdiv((long)B * S * H * 8, 256), delta_grid = attn_cdiv((long)B * S * H, 256);      // the vector kernel: 8 lanes per row
    const bool delta_vec = !f.dropout && f.vec && f.o_aligned;       // (dropout backward never takes the vector delta or the vector reduce)
    if (D > 128) {                     // 128 < head_dim <= 256 (attention_wide.hip): delta, the dK / dV pass, the dQ pass: no dQ partials, no reduce
        p.delta = delta_vec ? AttnDelta::Vector : AttnDelta::Scalar;
        p.delta_grid = delta_vec ? delta_vec_grid : delta_grid;
        on(AttnFamily::Wide, attn_cdiv(S, 32) * B * H, 256, 32);
        p.drop = f.dropout;
        p.absmax_tensors = !f.dropout && f.has_dqkv_absmax ? 3 : 0;      // these kernels publish nothing: one grouped-absmax launch over dQ, dK and dV
        return p;
    }
    bool dkdv_published = false;
    auto blocks256 = [&](AttnFamily fam, int qs) {                   // 256 keys per workgroup: half the dQ slabs (the workspace is sized for 128)
        p.n_kblocks = attn_cdiv(S, 256);
        on(fam, p.n_kblocks * B * H * qs, 512, 256);
        p.qs = qs;
        if (qs == 2) {                 // the second half's dK / dV: the first two slabs the 256-key blocks leave unused
            p.dk2 = w.dq_part + (int64_t)p.n_kblocks * w.slab;
            p.dv2 = p.dk2 + w.slab;
            p.add_cols_grid = attn_cap_blocks((long)B * S * (H * D / 4), 256, 2048);
        }
    };
    const bool out_aligned = f.dq_aligned && f.dk_aligned && f.dv_aligned;
    const bool split_ok = !f.dropout && D == 32 && f.vec && split_on && out_aligned;
    // 128 .. 255 workgroups of 256 keys: the query tiles of a key block go to two workgroups (QS = 2)
    const bool qs_shape = f.lddk4 && f.lddv4 && f.dq_part_aligned && wg8 >= 128 && wg8 < 256 && attn_cdiv(S, 32) >= 8 && attn_two_spare_slabs(S);
    const bool qsplit = f16 && split_ok && f.o_aligned && qs_shape && sw.split == AttnSplit::Heuristic && sw.qsplit;
    const bool fused_delta = f16 && split_ok && f.o_aligned && sw.split != AttnSplit::FourWave && (sw.split == AttnSplit::EightWave || wg8 >= 256 || qsplit);   // the fp16 8-wave kernel forms delta itself
    if (fused_delta) p.delta = AttnDelta::None;
    else if (delta_vec) { p.delta = AttnDelta::Vector; p.delta_grid = delta_vec_grid; }
    else { p.delta = AttnDelta::Scalar; p.delta_grid = delta_grid; }

    if (qsplit) {
        // (attn_bwd_h16_kernel<8, 2> measured equal here -- 76.5 against 77.2 us at 4 x 1 024 tokens: sixteen query tiles per workgroup -- so this
        // shape stays on the kernel its tests were written against)
        blocks256(AttnFamily::BwdSplit8, 2);
        p.pp = 2; p.op = 2; p.tr = 1; p.f16 = 1;
        dkdv_published = true;
    } else if (split_ok && fill8) {
        blocks256(AttnFamily::BwdSplit8, 1);
        const bool h16_shape = f16 && fused_delta && (long)B * H * S >= 1024;
        if (h16_shape && sw.h16 == H16_FOUR_WAVE) {          // back to 128-key blocks
            p.n_kblocks = attn_cdiv(S, 128);
            on(AttnFamily::BwdH16, p.n_kblocks * B * H, 256, 128);
            p.nw = 4; p.qs = 1; p.var = 0;
            dkdv_published = true;
        } else if (h16_shape && (sw.h16 & 15) == H16_EIGHT_WAVE) {
            p.family = AttnFamily::BwdH16;
            p.nw = 8; p.qs = 1; p.var = (sw.h16 >> 4) >= 1 && (sw.h16 >> 4) <= 3 ? (sw.h16 >> 4) : 0;
            dkdv_published = true;
        } else if (f16 && fused_delta) { p.pp = 2; p.op = 2; p.tr = 1; p.f16 = 1; dkdv_published = true; }
        else if (pp % 10 == 3) { p.pp = 3; p.op = 3; }
        else if (op == 3) { p.pp = 2; p.op = 3; }
        else { p.pp = 2; p.op = 2; p.tr = sw.tr; }
    } else if (split_ok) {
        on(AttnFamily::BwdSplit4, p.n_kblocks * B * H, 256, 128);
    } else if (!f.dropout && D > 32 && D <= 64 && f.vec && split_on && out_aligned) {
        const bool two64 = pp % 10 == 2 && op == 2;
        // [r6] fp16 pieces on eight waves: 256-key blocks when they fill the chip, shared between two workgroups (QS = 2) at 128 .. 255 blocks
        const bool f16_8 = f16 && sw.dh8 && sw.split != AttnSplit::FourWave;
        if (f16_8 && wg8 >= 256) {     // (EightWave does not force this one)
            blocks256(AttnFamily::BwdSplit8Dh, 1);
            p.f16 = 1;
            dkdv_published = true;
        } else if (f16_8 && qs_shape) {
            blocks256(AttnFamily::BwdSplit8Dh, 2);
            p.f16 = 1;
            dkdv_published = true;
        } else if (two64 && sw.tr && fill8) {                // (C5: 128 such workgroups: stays on the 4-wave kernel, 800 vs 822 us)
            blocks256(AttnFamily::BwdSplit8Dh, 1);
        } else {
            on(AttnFamily::BwdSplitDh, p.n_kblocks * B * H, 256, 128);
            p.dh = 64;
            if (f16) { p.pp = 2; p.op = 2; p.f16 = 1; }
            else if (two64) { p.pp = 2; p.op = 2; }
            else { p.pp = 3; p.op = 3; }
        }
    } else {
        on(AttnFamily::Fp32, p.n_kblocks * B * H, 256, 128);
        p.dh = DP; p.drop = f.dropout; p.lds_bytes = attn_bwd_lds_bytes(DP);
    }
    const long total = (long)B * H * S * DP;
    const bool vec_ok = !f.dropout && D % 4 == 0 && f.dq_aligned && f.lddq4 && f.dq_part_aligned && total < (1L << 31);
    if (vec_ok && (DP != 32 || D == 32)) {
        p.reduce = AttnReduce::Vector;
        p.reduce_dp4 = DP / 4;
        p.reduce_grid = attn_cap_blocks(total / 4, 256, DP == 32 ? 1024 : 2048);
    } else {
        p.reduce = AttnReduce::Scalar;
        int nb = attn_cdiv(total, 256); if (nb > 4096) nb = 4096;
        p.reduce_grid = nb;
    }
    // main kernels that do not publish: one grouped-absmax launch over dK and dV
    p.absmax_tensors = !f.dropout && f.has_dqkv_absmax && !dkdv_published ? 2 : 0;
    return p;
}

}  // namespace gaot
