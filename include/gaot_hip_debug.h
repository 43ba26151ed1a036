/*
 * gaot_hip_debug.h -- tuning / ablation hooks of libgaot_hip.so.  NOT part of the data path and NOT part of the drop-in
 * boundary (include/gaot_hip.h): these setters change process-global kernel-selection state, so they are neither thread-safe
 * nor re-entrant across streams.  Only tools/, bench.py's separately reported `--dtype bf16` variant and A/B tests call them;
 * gaot_amd's modules never do.  Every setter returns the previous value.
 */
#ifndef GAOT_HIP_DEBUG_H
#define GAOT_HIP_DEBUG_H

#include "gaot_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tuning hook (not part of the data path): force the GEMM tile; 0 = heuristic. Returns the previous value. */
int gaot_debug_set_gemm_tile(int cfg);
/* tuning hook: ablate parts of the GEMM kernel (results become WRONG): 1 no in-loop loads, 2 no LDS staging, 4 no stores */
int gaot_debug_set_gemm_ablate(int bits);
/* which kernel family served the calling thread's last gaot_gemm_f32: 1 = fp32 MFMA tiles, 2 = skinny VALU path,
 * 3 = split-bf16 MFMA tiles (fp32 operands split exactly into three bf16 pieces, six bf16 MFMAs per product, fp32-level error) */
int gaot_debug_last_gemm_path(void);
/* which kernel gaot_gemm_f32 WOULD run this product on, under the switches as they stand (csrc/gemm_plan.h; launches nothing and reads
 * no memory through the descriptor's pointers): out = {path (as gaot_gemm_path), family (0 / 1 / 2 skinny TN / K / N kernels, 3 register-
 * staged fp32 tiles, 4 LDS-direct fp32 tiles, 5 staged split tiles, 6 all-DMA fp16-piece tiles), tile rows, tile columns, variant (family 3:
 * the configuration as gaot_debug_set_gemm_tile numbers them, 4: tile id 1 .. 3, 5: tile height), K slabs, the reduce that follows (0 none,
 * 1 vector, 2 scalar), whether an absmax launch over C follows when c_absmax is given}; GAOT_OK, or the descriptor's error */
int gaot_debug_gemm_plan(const gaot_gemm_desc* d, int32_t out[8]);
/* tuning hook: 0 = register-staged fp32 tiles only, 1 = + LDS-direct fp32 tiles (2-stage ring), 3 = same with a 3-stage
 * ring, 4 = + split-bf16 tiles where the heuristic picks them (DEFAULT), 5 = split-bf16 wherever eligible, 6 = split-bf16
 * for the SwiGLU-gate product only */
int gaot_debug_set_gemm_glds(int on);
/* 3 (default): fp32-level products from three bf16 pieces per operand; 1: operands rounded to bf16, one piece product, fp32
 * accumulation -- the separately reported `bench.py --dtype bf16` variant only (BASELINE configs[1]); returns the old value. */
int gaot_debug_set_gemm_pieces(int pieces);
/* 0: ignore gaot_gemm_desc.b_planes (same-box A/B of the pre-split weight planes; bit-identical results); returns the old value */
int gaot_debug_set_gemm_planes(int on);
/* all-DMA fp16-piece tiles (gemm_ad.hip): 0 off, 1 per the heuristic (default), 2 / 3: 64- / 128-row tiles wherever eligible; returns the old value */
int gaot_debug_set_gemm_ad(int on);
/* GEMM vector epilogues of the acts that read aux_in (GELU_BWD / RELU_BWD / SWIGLU_BWD): 1 (default) = the aux vectors of a wave's whole
 * 32-row band are issued together, ahead of the band's LDS transpose; 0 = one pass's worth in front of every pass's arithmetic (same-box
 * A/B; bit-identical results); returns the old value */
int gaot_debug_set_gemm_aux_prefetch(int on);
/* 64 x 64 all-DMA tiles for narrow outputs (N <= 256), bits: 1 (default) launches that 64 x 128 tiles leave half filled (4 096-token
 * batches), 2 also K <= 256 at full launches (off: slower at step level); 0 none (same-box A/B; see csrc/gemm_plan.h);
 * returns the old value */
int gaot_debug_set_gemm_ad_narrow(int on);
/* attention backward, head_dim 32, fp16 pieces: 1 (default) lets two workgroups share the query tiles of a 256-key block when the launch
 * would otherwise hold 128 .. 255 workgroups (4 x 1 024 tokens x 8 heads); 0: the 4-wave kernel as before (same-box A/B); returns the old value */
int gaot_debug_set_attention_qsplit(int on);
/* fp16-piece products: output tiles (of the split tile kernels and the grouped weight-gradient launch) that took the per-row second pass
 * since the counter was last reset -- a tile whose operand rows span more than 2^13 in magnitude is recomputed with one power-of-two
 * scale per row (gemm_split.hip).  Synchronises the device.  reset != 0: zero the counter after reading it. */
unsigned gaot_debug_split_redo_count(int reset);
/* grouped weight gradients: values of k per workgroup (K slab length; multiple of 32, default 4096) */
/* (k > 0: a fixed K slab for every product of the grouped launch; 0: automatic; -c: the cap of longer products' slabs (default 4 096);
 * -(100000 + c): the same for node-level products, K > 16 384) */
int gaot_debug_set_wgrad_kslab(int k);
/* [r6] grouped weight gradients on fp16 pieces: 256 = 256 x 128 tiles on eight waves (one workgroup per CU) when every product's M is a
 * multiple of 256; 128 = 128 x 128 tiles, two workgroups per CU */
int gaot_debug_set_gemm_ad_flush(int on);        /* [r6] narrow outputs with a reduction of 1 025 .. 2 048: 1 (default) = unsplit on the 64 x 64 all-DMA tiles, which flush their accumulators every 1 024 values of k; 0 = K slabs as before; negative = query; returns the old value */
int gaot_debug_set_wgrad_tile_rows(int bm);
/* [r6] grouped weight gradients, automatic K slabs: 0 (default) = the rule of rounds 3-5, 1 = a cost model (rounds x longest K loop + a per-slab term: measured slower, gemm_split.hip) */
int gaot_debug_set_wgrad_slab_rule(int r);
/* tuning hook: head_dim 32 attention, 1 = split-bf16 MFMA kernels (default), 0 = fp32-MFMA kernels, 2 / 3 = split with the
 * 8-wave / 4-wave forward workgroup forced.  Returns the previous value. */
int gaot_debug_set_attention_split(int on);
int gaot_debug_set_attention_keysplit(int on);  /* [r6] the key-split forward of gaot_attention_fwd_ws: 1 (default) = on for the shapes it is for (head_dim 36 .. 64), 2 = head_dim 32 too (tests), 0 = off (the workspace query then answers 0); returns the old value */
int gaot_debug_set_attention_dh8(int on);       /* [r6] 32 < head_dim <= 64 on fp16 pieces: 1 (default) = the 8-wave 256-key backward (attn_bwd_split8_dh_kernel<true, QS>: query-split at 128 .. 255 key blocks x batch x heads), 0 = the 4-wave 128-key kernel; returns the old value */
int gaot_debug_set_attention_h16(int mode);     /* [r6] the fp16-piece backward at >= 256 key blocks: 8 + 16 VAR = attn_bwd_h16_kernel<8, 1, VAR> (default 0x18), 4 = <4> (two workgroups per CU), 0 = attn_bwd_split8_kernel; returns the old mode */
/* head_dim-32 split attention: pieces of P in the forward and of P / dS in the backward products, as 10 * forward + backward:
 * 22 (default) = two rounded pieces (five piece products instead of six) in both; 33 = exact three-way splits; 32, 23 for A/B runs.
 * Returns the previous value. */
int gaot_debug_set_attention_p_pieces(int n);
/* head_dim-32 split attention: pieces of the Q / K / V / dO operands: 2 (default) = two rounded pieces (with two-piece P / dS: three
 * piece products everywhere), 3 = exact three-way splits.  Returns the previous value. */
int gaot_debug_set_attention_operand_pieces(int n);
/* A/B hook: 1 (default) = the two-piece head_dim-32 backward reads dO^T / Q^T / dS through transposing LDS reads, 0 = separately staged
 * transposed planes.  Same results.  Returns the previous value. */
int gaot_debug_set_attention_tr(int on);
/* tuning hook: 1 = the software-pipelined 8-wave split forward where it applies (S % 64 == 0), 0 (default) = the plain one.
 * Returns the previous value. */
int gaot_debug_set_attention_pipe(int on);
/* which kernels an attention call WOULD run, under the switches as they stand (csrc/attention_plan.h; launches nothing and touches no
 * memory).  The call is described by its sizes, `pieces`, direction (0 forward: gaot_attention_fwd_ws, 1 backward: gaot_attention_bwd),
 * dropout (1: the _dropout entry of that direction; pieces and the absmax bits are then ignored) and the facts the entry point reads off
 * its pointers and pitches, as bits:
 *   QKV_ABSMAX, DOUT_ABSMAX, DQKV_ABSMAX  that pointer given
 *   VEC              q, k, v 16-byte aligned, their pitches % 4 == 0; backward: dout and ldo too (head_dim % 4 is read off head_dim)
 *   O_ALIGNED        o 16-byte aligned                       LDO4  ldo % 4 == 0 (forward)
 *   WORKSPACE        forward: a workspace given              WS_ALIGNED  ... and 16-byte aligned
 *   DQ_ / DK_ / DV_ALIGNED, LDDQ4 / LDDK4 / LDDV4            the backward's outputs and their pitches % 4 == 0
 *   DQ_PART_ALIGNED  workspace + B H S floats 16-byte aligned (backward)
 * out = {0 delta step (0 none: forward or fused, 1 vector, 2 scalar), 1 its grid,
 *        2 family of the main kernel (0 one key, 1 wide (attention_wide.hip), 2 fp32 MFMA attn_fwd_kernel / attn_bwd_kernel<dh, drop>, 3
 *          attn_fwd_glds_kernel, 4 attn_fwd_split_kernel<nw, dh, pp, op, f16, ks>, 5 attn_fwd_split_pipe_kernel, 6 attn_bwd_split_kernel,
 *          7 attn_bwd_split_dh_kernel<dh, pp, op, f16>, 8 attn_bwd_split8_kernel<pp, op, tr, f16, qs>, 9 attn_bwd_h16_kernel<nw, qs, var>,
 *          10 attn_bwd_split8_dh_kernel<f16, qs>),
 *        3 nw, 4 dh, 5 pp, 6 op, 7 f16, 8 ks, 9 tr, 10 qs, 11 var, 12 drop  (template arguments of that family; the others 0),
 *        13 grid, 14 block, 15 dynamic LDS bytes, 16 keys (forward: queries) per workgroup, 17 n_kblocks (dQ slabs written),
 *        18 grid of the key-split combine (0 none), 19 grid of the query-split add_cols launch (0 none),
 *        20 dQ reduce (0 none, 1 vector, 2 scalar), 21 its DP4 (8 / 16 / 32), 22 its grid,
 *        23 tensors under the trailing grouped absmax (0, 2: dK dV, 3: dQ dK dV),
 *        24 o_part, 25 lse_part, 26 delta, 27 dq_part, 28 dk2, 29 dv2  (floats from the workspace base; -1 unused),
 *        30 workspace floats the caller must provide};  GAOT_OK, or the error the entry point gives for those sizes */
typedef struct gaot_debug_attention_query {
    int32_t B, S, H, Hkv, head_dim, pieces, direction, dropout;
    uint32_t facts;
} gaot_debug_attention_query;
enum {
    GAOT_ATTN_FACT_QKV_ABSMAX = 1 << 0, GAOT_ATTN_FACT_DOUT_ABSMAX = 1 << 1, GAOT_ATTN_FACT_DQKV_ABSMAX = 1 << 2, GAOT_ATTN_FACT_VEC = 1 << 3,
    GAOT_ATTN_FACT_O_ALIGNED = 1 << 4, GAOT_ATTN_FACT_LDO4 = 1 << 5, GAOT_ATTN_FACT_WORKSPACE = 1 << 6, GAOT_ATTN_FACT_WS_ALIGNED = 1 << 7,
    GAOT_ATTN_FACT_DQ_ALIGNED = 1 << 8, GAOT_ATTN_FACT_DK_ALIGNED = 1 << 9, GAOT_ATTN_FACT_DV_ALIGNED = 1 << 10,
    GAOT_ATTN_FACT_LDDQ4 = 1 << 11, GAOT_ATTN_FACT_LDDK4 = 1 << 12, GAOT_ATTN_FACT_LDDV4 = 1 << 13, GAOT_ATTN_FACT_DQ_PART_ALIGNED = 1 << 14
};
#define GAOT_ATTENTION_PLAN_COLUMNS 31
int gaot_debug_attention_plan(const gaot_debug_attention_query* call, int64_t out[GAOT_ATTENTION_PLAN_COLUMNS]);
/* the plan the calling thread's last forward (direction 0) or backward (1) attention launch executed, dropout entries included: the same
 * columns; all -1 before the first such launch.  A call that fails its checks leaves it as it was. */
int gaot_debug_last_attention_plan(int direction, int64_t out[GAOT_ATTENTION_PLAN_COLUMNS]);
/* tuning hook (results become WRONG): forward kernel 1 = no stores, 2 = no GELU, 4 = no MFMA layers, 8 = no weight staging */
int gaot_debug_set_kernel_mlp_ablate(int bits);
/* A/B hook: 1 (default) = the bf16-split kernel-MLP kernels (fp32-level products on v_mfma_f32_32x32x16_bf16), 0 = the fp32-MFMA
 * kernels.  Same results to fp32 rounding either way.  Returns the previous value. */
int gaot_debug_set_kernel_mlp_split(int on);
int gaot_debug_set_ep_chunk(int edges_per_chunk);      /* tuning only: 0 = default (32) */
/* A/B hook: the grouped helper launches (gaot_absmax_grouped, gaot_split_f16_planes_grouped, gaot_colsum_grouped), one bit per kernel:
 * 1 = absmax, 2 = fp16 planes, 4 = column sums; 7 (default) = the present kernels, a cleared bit = the kernel as it was before them.
 * Same bits in every output either way (the absmax word: the same maximum over its slots).  Returns the previous value. */
int gaot_debug_set_grouped_helpers(int bits);
/* A/B hook: gaot_proj_fold_bwd, 1 (default) = dwa and the stretch sums of g_weff Wr_a^T computed in slices by every workgroup ahead of the
 * ticket, the last workgroup only adds the partial rows and joins dhw; 0 = all of it by the last workgroup, as before.  Same bits either
 * way.  Returns the previous value. */
int gaot_debug_set_proj_fold_split(int on);
/* A/B hook: gaot_gno_proj_backward with a row-bias gradient, 1 (default) = computed by workgroups appended to the edge-gradient launch,
 * 0 = by a gaot_batchsum launch behind it, as before.  Same bits either way.  Returns the previous value. */
int gaot_debug_set_proj_bwd_rowbias(int on);

#ifdef __cplusplus
}
#endif
#endif
