// Which kernel serves a product of gaot_gemm_f32: the whole selection as one pure function of the descriptor's facts and the debug
// switches.  Plain C++17: no HIP header, no pointer, no global -- the launch (gemm.hip), the dry answer (gaot_gemm_path) and the
// CPU test that enumerates the table (tests/test_gemm_plan_cpu.py through gaot_debug_gemm_plan) all read this one function.
#pragma once
#include <stdint.h>

namespace gaot {

constexpr int GEMM_BK = 32;          // k-tile of every tile kernel
constexpr int GEMM_ACT_SWIGLU = 6;   // = GAOT_ACT_SWIGLU (include/gaot_hip.h; both checked in gemm.hip)

// ---- what the decision reads of a (validated) descriptor; pointers have become booleans
struct GemmFacts {
    int M, N, K;
    bool a_kmajor, b_kmajor;
    int act;
    int split_k;               // as requested
    bool has_workspace;
    bool raw_slabs;
    bool has_colsum;
    bool has_a2; int k_split;
    bool vec;                  // operands allow 16-byte loads
    bool vec_epi;              // N, C and every epilogue operand allow 16-byte accesses
    bool plain_epi;            // the split-K reduce has nothing to do but sum (+ an aligned residual) on 16-byte vectors
    int pieces;                // effective: after the forced override and the "no absmax words -> 3" demotion
    bool planes_offered;       // gaot_gemm_desc.b_planes given
    bool planes_usable;        // ... and fp16 pieces, the planes switch on, layout and alignment as the kernels need
};

// ---- the debug switches (include/gaot_hip_debug.h), decoded once by their setters
enum class SplitTiles {        // split-bf16 / fp16-piece tiles (gemm_split.hip); +3 = the argument of gaot_debug_set_gemm_glds
    Off = 0,
    Heuristic = 1,             // DEFAULT: +5 % on the GAOT step, same-box A/B on two boxes, DESIGN.md section 6
    Everywhere = 2,            // 128-row tiles wherever eligible
    SwigluOnly = 3,            // for the SwiGLU-gate product only
    Rows64Everywhere = 4,      // 64-row tiles wherever eligible
    NoRows64 = 5,              // as Heuristic without the 64-row tiles
    Rows64NN = 6,              // 64-row tiles for NN products without planes too
};
enum class Tall256 { Off = 0, WhileFull = 1, Everywhere = 2 };      // 256x128 (8-wave) split tiles: while they still fill the chip / wherever M allows (tuning)
enum class AdTiles { Off = 0, Heuristic = 1, Rows64Everywhere = 2, Rows128Everywhere = 3 };      // all-DMA fp16-piece tiles (gemm_ad.hip)
// 64 x 64 all-DMA tiles (gaot_debug_set_gemm_ad_narrow, bits)
constexpr int NARROW_HALF_FILLED = 1;      // half-filled launches of outputs two tiles wide (default)
constexpr int NARROW_SHORT_K = 2;          // also N <= 256, K <= 256 at full launches
constexpr int NARROW_THREE_WIDE = 4;       // also outputs THREE tiles wide (4 096 tokens x 384: the 3-D configuration's o_proj-shaped products, which fell to the fp32-MFMA tiles; default)
constexpr int NARROW_K_SLABS = 8;          // K slabs of such products too (4 096 x 384 x 1 152 in two slabs: C5 5.20 -> 5.27 ms same-box, tools/c45_ab.py 5 13: off)
constexpr int NARROW_A2 = 16;              // the concatenated-input (A2) product of the skip block too (C4 1.498 -> 1.500, C5 5.12 -> 5.09: nothing: off)
// gaot_debug_set_gemm_tile: 0 = heuristic, else the register-staged configuration below (1 .. 3 also name the LDS-direct tiles)
constexpr int TILE_AUTO = 0, TILE_GLDS_LAST = 3, TILE_CFG_LAST = 6;

struct GemmSwitches {
    bool glds = true;                               // eligible products run on the LDS-direct kernels (gemm_glds.hip); false = register-staged only
    SplitTiles split = SplitTiles::Heuristic;
    Tall256 tall256 = Tall256::Off;
    int forced_pieces = 0;                          // 0 = every call's own gaot_gemm_desc.pieces; 1 = operands rounded to bf16, one piece product (bench `--dtype bf16` only); 2 / 3 = forced for A/B runs
    AdTiles ad = AdTiles::Heuristic;
    bool ad_flush = true;                           // [r6] unsplit reductions of 1 025 .. 2 048 on the 64 x 64 all-DMA tiles with the in-kernel flush (gemm_ad.hip FL); false = K slabs as before
    int ad_narrow = NARROW_HALF_FILLED | NARROW_THREE_WIDE;
    bool planes = true;                             // false: ignore gaot_gemm_desc.b_planes (A/B switch; read when the facts are gathered)
    int tile = TILE_AUTO;
};

// ---- the answer
enum class GemmFamily { SkinnyTN = 0, SkinnyK = 1, SkinnyN = 2, Cfg = 3, Glds = 4, Split = 5, Ad = 6 };
enum class GemmReduce { None = 0, Vector = 1, Scalar = 2 };
struct CfgTile { int bm, bn, waves_m, waves; };
// register-staged configurations by the number of gaot_debug_set_gemm_tile (= GemmPlan::variant of the family)
constexpr CfgTile CFG_TILES[TILE_CFG_LAST + 1] = {{0, 0, 0, 0}, {128, 128, 2, 4}, {128, 64, 2, 4}, {64, 64, 2, 4}, {128, 32, 4, 4}, {128, 128, 2, 8}, {128, 64, 4, 8}};

struct GemmPlan {
    GemmFamily family;
    int tile_rows, tile_cols;          // 0 x 0 on the skinny kernels
    int variant;                       // Glds: tile id 1 .. 3; Cfg: index into CFG_TILES; Split: tile height 64 / 128 / 256; else 0
    int split_k, ktiles_per_split;     // effective: no empty slab
    GemmReduce reduce;
    bool publish_after;                // the kernel does not publish C's magnitude word itself: one absmax launch over C as stored (if the caller wants the word)
    bool vec_epi;                      // as the launch sees it (raw slabs of an uncut reduction and the SwiGLU gate always take the vector epilogue)
    int path;                          // 1 = fp32-MFMA tiles, 2 = skinny, 3 = split tiles: gaot_gemm_path / gaot_debug_last_gemm_path
};

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// K slabs of a reduction of K asked to be cut into split_k: 32-wide k-tiles, no empty slab
inline int gemm_slab_count(int K, int split_k, int* ktiles_per_split = nullptr) {
    const int nkt = ceil_div(K, GEMM_BK);
    int split = split_k > 1 ? split_k : 1;
    if (split > nkt) split = nkt;
    const int per = ceil_div(nkt, split);
    if (ktiles_per_split) *ktiles_per_split = per;
    return ceil_div(nkt, per);
}

inline GemmPlan plan_gemm(const GemmFacts& f, const GemmSwitches& sw) {
    const int M = f.M, N = f.N, K = f.K, pieces = f.pieces;
    const bool ak = f.a_kmajor, bk = f.b_kmajor, raw = f.raw_slabs;
    GemmPlan p{};
    p.split_k = gemm_slab_count(K, f.split_k, &p.ktiles_per_split);
    p.vec_epi = f.vec_epi || (raw && p.split_k <= 1);      // a reduction too short to cut: the product itself is slab 0
    const int split_k = p.split_k;
    const bool vec_epi = p.vec_epi;
    auto tiles = [&](int bm, int bn) { return (long)ceil_div(M, bm) * ceil_div(N, bn); };
    auto blocks = [&](int bm, int bn) { return tiles(bm, bn) * split_k; };
    auto on = [&](GemmFamily fam, int rows, int cols, int variant) { p.family = fam; p.tile_rows = rows; p.tile_cols = cols; p.variant = variant; };
    auto on_glds = [&](int tile) { on(GemmFamily::Glds, tile == 3 ? 64 : 128, tile == 1 ? 128 : 64, tile); };
    auto on_cfg = [&](int cfg) { on(GemmFamily::Cfg, CFG_TILES[cfg].bm, CFG_TILES[cfg].bn, cfg); };
    const bool split_on = sw.split != SplitTiles::Off;

    if (f.act == GEMM_ACT_SWIGLU) {          // only the LDS-staged kernels lay the gate's bands out
        const long nb128 = tiles(128, 128);
        p.vec_epi = true;
        if (sw.split == SplitTiles::Everywhere || (split_on && nb128 >= 256)) {
            const bool big = M >= 256 && (sw.tall256 == Tall256::Everywhere || (sw.tall256 == Tall256::WhileFull && nb128 >= 500));
            const int bm = big && pieces != 1 ? 256 : 128;
            on(GemmFamily::Split, bm, 128, bm);
            p.path = 3;
        } else {
            on_glds(nb128 >= 512 ? 1 : (tiles(128, 64) >= 512 ? 2 : 3));
            p.path = 1;
        }
        return p;
    }
    // skinny VALU kernels (skinny.hip)
    if (sw.tile == TILE_AUTO && !raw && !f.has_a2) {
        // transposed-A weight gradient with a tiny side and a long reduction (needs the split-K workspace)
        const bool tn = !ak && !bk && split_k > 1 && f.has_workspace && (N <= 16 || M <= 16) && (long)M * N <= 4096 && K >= 1024;
        const bool row = ak && split_k <= 1 && !f.has_colsum;
        if (tn || (row && (K <= 16 || N <= 4))) {
            on(tn ? GemmFamily::SkinnyTN : (K <= 16 ? GemmFamily::SkinnyK : GemmFamily::SkinnyN), 0, 0, 0);
            p.path = 2;
            p.publish_after = true;
            return p;
        }
    }
    const bool glds_ok = sw.glds && f.vec && vec_epi && K % 32 == 0 && M >= 4 && N >= 4;
    // the bf16 MFMA does not round its fp32 accumulator to nearest: same-signed increments drift (4096^3 with positive
    // operands: 1.1e-5 relative against 8e-7 on the fp32 MFMA, tools/acc_bias.py), so one workgroup accumulates at most 1 024
    // values of k on that pipe; longer reductions either arrive split (the slabs are summed on the vector pipe) or stay on the
    // fp32-MFMA tiles
    const long k_per_wg = split_k > 1 ? (long)p.ktiles_per_split * 32 : K;
    // [r6] unsplit reductions of 1 025 .. 2 048 on the 64 x 64 all-DMA tiles, which flush their accumulators every 1 024 values of k in the
    // kernel (gemm_ad.hip FL): the narrow outputs whose K slabs would not fill the split tiles and fell to the fp32-MFMA tiles (4 096 x 384 x
    // 1 152, the 3-D configuration's q|k|v input gradient: two slabs of 39 us + a reduce)
    const bool long_k = sw.ad_flush && pieces == 4 && split_k <= 1 && K > 1024 && K <= 2048 && !raw;
    const bool split_ok = split_on && sw.split != SplitTiles::SwigluOnly && glds_ok && (!f.has_a2 || (ak && f.k_split % 16 == 0)) && sw.tile == TILE_AUTO &&
                          (k_per_wg <= 1024 || pieces == 1 || sw.split != SplitTiles::Heuristic || long_k);      // forced tuning modes bypass the cap
    // measured (round 2, tools/gemm_bench.py sweeps): the 128x128 split-bf16 tiles win once they fill the chip (>= 256 workgroups
    // counting split-K slabs) on outputs at least one tile wide; narrower / smaller products stay on the fp32 MFMA tiles
    // two-piece products, outputs at most six 128-wide tiles across (N <= 768): the 64-row tiles win although the 128-row ones would
    // fill the chip (8192 x 768 x 256 NT: 21.7 vs 24.2 us, NN x 512 x 256: 18.6 vs 19.5; N >= 1 024: the other way round)
    const bool two_pl = pieces == 2 || pieces >= 4;       // two planes per operand in LDS
    const bool fills64 = blocks(64, 128) >= 250 && M >= 64 && N >= 128 && split_k <= 1;
    const bool prefer64 = split_ok && !long_k && sw.split == SplitTiles::Heuristic && two_pl && ak && ceil_div(N, 128) <= 6 && fills64;
    const bool split128 = split_ok && !long_k && sw.split != SplitTiles::Rows64Everywhere && !prefer64 &&
                          (sw.split == SplitTiles::Everywhere || (blocks(128, 128) >= 250 && M >= 128 && N >= 128 && tiles(128, 128) >= 8));
    // outputs only a few 128-wide tiles across (N = 256): 64-row tiles double the workgroup count
    // (with pre-split B planes an NN product stages B exactly like an NT one; with two-piece products the 64-row split tiles beat the
    // fp32-MFMA tiles on the NN products too: 8192 x 256 x 768 37.4 -> 25.6 us, x 512 26.5 -> 19.0, x 256 15.5 -> 12.8, tools/gemm_modes_2p.py)
    const bool split64 = split_ok && !long_k && !split128 && sw.split != SplitTiles::NoRows64 && sw.split != SplitTiles::Everywhere &&
                         (sw.split == SplitTiles::Rows64Everywhere || prefer64 ||
                          ((ak && (bk || f.planes_usable || sw.split == SplitTiles::Rows64NN || two_pl)) && fills64));   // measured: NT +6-14 %, NN +-0
    // 64 x 64 all-DMA tiles (gaot_debug_set_gemm_ad_narrow, bits): (1, default) half-filled launches of outputs two tiles wide (4 096 tokens x
    // 256: 128 workgroups of 64 rows, which fall to the fp32-MFMA tiles) get 256 workgroups -- tools/ad_bench.hip: 4096 x 256 x 256 in 8.3 us
    // against ~15; same-box step A/B at the 4 096-token batch (tools/step_ab.py --c4, twice): 1.6486 -> 1.6249, 1.6481 -> 1.6234 ms, C2
    // untouched (its launches are full).  (2, off) N <= 256 with K <= 256 at 8 192 rows: 11.9 -> 11.2 us alone, but C2 2.1499 -> 2.1663,
    // 2.1399 -> 2.1705 ms per step.  Bit-identical to the other fp16-piece tiles in every test (tests/test_ops_gpu.py, tools/ad_stress.py);
    // a product that (1) moves off the fp32-MFMA tiles is rounded as the fp16-piece family rounds (same error class, other last bits).
    // (An earlier series of A/B runs looked inconsistent and twice ended at an unexplained loss: that was the host-side slot bookkeeping,
    // DESIGN 7, not these tiles.)
    const bool narrow_shape = sw.ad == AdTiles::Heuristic && (sw.ad_narrow & NARROW_HALF_FILLED) && split_ok && !split128 && !split64 && pieces == 4 && ak && K % 32 == 0 && vec_epi &&
                              (split_k <= 1 || ((sw.ad_narrow & NARROW_K_SLABS) && !raw)) && (!f.has_a2 || ((sw.ad_narrow & NARROW_A2) && f.k_split % 32 == 0)) &&
                              (ceil_div(N, 128) == 2 || ((sw.ad_narrow & NARROW_THREE_WIDE) && ceil_div(N, 128) == 3)) && blocks(64, 64) >= 128 && tiles(64, 128) < 250 &&
                              k_per_wg <= (long_k ? 2048 : 1024);          // (K slabs of such a product too -- 4 096 x 384 x 1 152 in two slabs)
    const bool ad_narrow = narrow_shape && f.planes_usable;
    // planes handed in but switched off (gaot_debug_set_gemm_planes(0)): the same tile family on the staged 64-row kernel, so that the
    // switch changes where B's pieces come from and nothing else (products WITHOUT planes -- B an activation -- stay where they were)
    const bool narrow_staged = narrow_shape && !long_k && !f.planes_usable && f.planes_offered;
    if (split128 || split64 || ad_narrow || narrow_staged) {
        // 256x128 (8-wave) tiles: measured +3-7 % on the NT / TN products that still give ~200 workgroups, -2 % on NN
        const bool big = split128 && M >= 512 && (sw.tall256 == Tall256::Everywhere || (sw.tall256 == Tall256::WhileFull && ak == bk && blocks(256, 128) >= 190));
        // all-DMA tiles (gemm_ad.hip; tools/ad_bench.hip, same box, us staged -> all-DMA): outputs two tiles wide (N <= 256) on 64-row
        // tiles: 8192 x 256 x 256 13.5 -> 11.8, x 768 26.7 -> 22.1, x 1024 32.8 -> 26.8; wider outputs on 64-row tiles while those fit
        // one round of two workgroups per CU (the 4 096-token batches), else on 128-row ones while THOSE fit one round; what needs more
        // rounds (8192 x 2048 x 256: 49 -> 51-54 us; x 768: 23.2 -> 26.8 on 64-row tiles) and the K-slab products (8192 x 256 x 2048 in
        // two slabs: 42.9 -> 42.6) stay on the staged kernel -- there the output stores / the slab count decide.  Step level
        // (tools/step_ab.py, same box): C2 2.3225 -> 2.2666 ms, C4-shaped 1.8169 -> 1.7888
        // Re-checked with the epilogue's aux prefetch in (tools/bin/ad_bench swiglu, u from HBM): the SwiGLU-gradient product 8192 x 1024 x 256
        // 39.8-43.0 us on the 128-row tiles (one round) against 42.3-42.6 on the 64-row ones (two rounds): the rule stays
        const bool ad_ok = sw.ad != AdTiles::Off && pieces == 4 && f.planes_usable && ak && K % 32 == 0 && vec_epi && (!f.has_a2 || f.k_split % 32 == 0);
        const bool ad64 = ad_ok && (sw.ad == AdTiles::Rows64Everywhere || (split_k <= 1 && (ceil_div(N, 128) <= 2 || blocks(64, 128) <= 512) && blocks(64, 128) >= 128));
        const bool ad128 = ad_ok && !ad64 && !big && (sw.ad == AdTiles::Rows128Everywhere || (split_k <= 1 && split128 && blocks(128, 128) <= 512));
        if (ad_narrow) on(GemmFamily::Ad, 64, 64, 0);
        else if (ad64) on(GemmFamily::Ad, 64, ((sw.ad_narrow & NARROW_SHORT_K) && K <= 256 && ceil_div(N, 128) <= 2) ? 64 : 128, 0);      // (8192 x 256 x 256: 11.9 -> 11.2 us on 64 x 64 tiles)
        else if (ad128) on(GemmFamily::Ad, 128, 128, 0);
        else {
            const int bm = (split64 || narrow_staged) ? 64 : (big && pieces != 1 ? 256 : 128);
            on(GemmFamily::Split, bm, 128, bm);
        }
    }
    // tile choice: the largest tile that still gives every CU (256) a workgroup; skinny N gets a 128x32 tile
    else if (glds_ok && sw.tile >= TILE_AUTO && sw.tile <= TILE_GLDS_LAST) {
        int tile = sw.tile;
        if (tile == TILE_AUTO) {      // from the on-box sweep (round 2, tools/gemm_bench.py; 2-stage ring)
            if (!ak && !bk) tile = blocks(128, 128) >= 256 ? 1 : (blocks(128, 64) >= 256 && M >= 128 ? 2 : 3);
            else if (blocks(128, 128) >= 512) tile = 1;
            else if (blocks(128, 64) >= 512) tile = 2;
            else tile = 3;
        }
        on_glds(tile);
    }
    else if (sw.tile > TILE_AUTO && sw.tile <= TILE_CFG_LAST) on_cfg(sw.tile);
    else if (N <= 32)                 on_cfg(4);
    // measured on MI355X (tools/gemm_bench.py): short reductions want SEVERAL block-waves in flight so that the
    // load / MFMA / store phases of different workgroups overlap; big tiles only pay off on large outputs.
    // transposed-A weight gradients (long reduction, split-K): 128x64 measured 10-17 % ahead of 64x64 once it fills the chip
    else if (!ak && !bk && blocks(128, 64) >= 256 && M >= 128) on_cfg(2);
    else if (blocks(64, 64) <= 1536)  on_cfg(3);
    else if (blocks(128, 64) <= 3072) on_cfg(2);
    else                              on_cfg(1);
    // the answer gaot_gemm_path has always given -- planes offered but unusable count as planes, so a long-K narrow product without usable planes reports 3 and runs on the fp32-MFMA tiles: kept as it is, ops.gemm keys on it
    p.path = (split128 || split64 || (narrow_shape && f.planes_offered)) ? 3 : 1;
    if (split_k > 1 && !raw) p.reduce = f.plain_epi ? GemmReduce::Vector : GemmReduce::Scalar;
    else p.publish_after = !vec_epi && !raw;
    return p;
}

}  // namespace gaot
