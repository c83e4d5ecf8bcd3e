// Who owns a scratch size: the module whose gate it mirrors.  A launcher that is handed scratch lowers its split until the slices
// fit (launch_small_splitk, tail_split_256, ...), so the size of a scratch region selects a kernel split and with it the bits of
// the result.  Each limit below is therefore stated once, here, beside the name of the module that applies it; the module's own
// *_fits / clamp code and the workspace layouts (layout.h, fused_forward.hip, entity_cache.hip) both read it from here.
// Part of internal.h, kept host-only (no HIP include) so that the layouts compile with a plain host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/drin_hip.h"
#include "arena.h"

namespace drin {

// The y (and z) extent a launch grid may have.  Every launcher whose grid.y counts mentions, groups, rows or row tiles slices at
// it (internal.h: for_grid_slices), strides past it or refuses past it; it stands here because the row limit below derives from it.
constexpr int kMaxGridY = 65535;

// ---- exact-fp32 products (gemm_f32.hip) ------------------------------------------------------------------------------
// mention-sized: at most this many rows (NT / NN) or reduction rows (TN) run on 64 x 64 tiles
constexpr int64_t kMentionSizedMaxRows = 2048;
// past that limit an NT / NN product runs on 128 x 128 tiles, one row tile per grid.y: the rows one product may have
// (launch_gemm_nt / launch_gemm_nn refuse more; api.hip's layers_call_fits asks before a call's first launch)
constexpr int64_t kF32MaxRows = (int64_t)kMaxGridY * 128;
inline bool gemm_f32_rows_fit(int64_t rows) { return rows <= kF32MaxRows; }
// small split-K (small_splitk_fits, launch_small_splitk, the NT group): products of a few hundred rows with a long reduction
// split K over workgroups into scratch, at most kSmallSplitkMaxSlices slices of [rows][n_out]
constexpr int64_t kSmallSplitkMaxRows = 512;
constexpr int kSmallSplitkMinK = 512;
constexpr int kSmallSplitkMaxSlices = 8;
inline bool small_splitk_shape(int64_t rows, int K) { return rows <= kSmallSplitkMaxRows && K >= kSmallSplitkMinK; }
inline int small_splitk_slices(int K) {   // >= 4 stages of 32 per slice
  const int s = K / 128;
  return s > kSmallSplitkMaxSlices ? kSmallSplitkMaxSlices : (s < 1 ? 1 : s);
}
inline size_t small_splitk_floats(size_t rows, size_t n_out) { return (size_t)kSmallSplitkMaxSlices * rows * n_out; }
// two such products in one grouped launch (launch_gemm_nt_pair): + the 16-byte alignment slack between their slices
inline size_t small_splitk_pair_floats(size_t rows_a, size_t n_a, size_t rows_b, size_t n_b) {
  return 8 + small_splitk_floats(rows_a, n_a) + small_splitk_floats(rows_b, n_b);
}
// slices of a mention-sized weight-gradient product (launch_gemm_tn_f32_group, launch_gemm_tn)
inline int small_tn_slices(int64_t reduction_rows) {
  const int64_t s = (reduction_rows + 127) / 128;
  return (int)(s > 4 ? 4 : (s < 1 ? 1 : s));
}
// ... that it stores: a product past the mention-sized limit leaves the group
inline size_t small_tn_stored_slices(size_t reduction_rows) {
  return reduction_rows > (size_t)kMentionSizedMaxRows ? 0 : (size_t)small_tn_slices((int64_t)reduction_rows);
}

// ---- split-bf16 NT products (gemm_f32.hip: launch_gemm_nt; gemm_bf16x3.hip, gemm_x3_planes.hip) ----------------------------
// from a tile row of pairs up DRIN_PREC_BF16X3 leaves the exact kernel; DRIN_PREC_BF16X3_ALL always does
constexpr int64_t kBf16x3MinRows = 256;
inline bool split_bf16(int precision) { return precision == DRIN_PREC_BF16X3 || precision == DRIN_PREC_BF16X3_ALL; }
inline bool nt_takes_bf16x3(int precision, int64_t rows) {
  return (precision == DRIN_PREC_BF16X3 && rows >= kBf16x3MinRows) || precision == DRIN_PREC_BF16X3_ALL;
}
// pre-split (hi, lo) weight planes stream by LDS-DMA in K-blocks of 32
inline bool nt_planes_width(int K) { return (K % 32) == 0; }
// an NT product whose row-side operand is STORED as bf16 (NtProduct::x_bf16; row stride ldx elements, reduction K): it runs on the
// stored rows as the hi plane of the plane kernel, else on a widened copy.  The layouts that carve the planes of the other operand
// or the widened chunk (table_topk.hip) ask here, as launch_gemm_nt does.
inline bool nt_bf16_rows_as_planes(int precision, int K, int64_t ldx) { return split_bf16(precision) && nt_planes_width(K) && (ldx % 8) == 0; }
// "this call's NT weights run as planes": the pair-sized products (pair_rows rows, reductions D and R) of a split-bf16 call
inline bool nt_weights_as_planes(int precision, int64_t pair_rows, int D, int R) {
  return split_bf16(precision) && pair_rows >= kBf16x3MinRows && nt_planes_width(D) && nt_planes_width(R);
}
// 256 x 256 tiles, one workgroup per CU: a round of tiles
constexpr int kTileRound = 256;
constexpr size_t kTile256Floats = 65536;
// tail split (tail_split_256): a partly filled last round splits K kTailSplitMax .. 2 ways while slices x tiles fit a round
constexpr int kTailSplitMax = 4;
constexpr int64_t kTailSplitMaxRounds = 16;
// the scratch with which every tail split is open: a quarter round of tail tiles, kTailSplitMax - 1 partial tiles each
inline size_t tail_split_floor_floats() { return (size_t)(kTileRound / kTailSplitMax) * (kTailSplitMax - 1) * kTile256Floats; }
// split-K of a whole product of less than half a round of tiles (launch_gemm_x3_planes): the first rung that fits a round
constexpr int64_t kPairSplitkMaxTiles = 128;
constexpr int kPairSplitkLadder[] = {16, 8, 6, 4, 3, 2};
inline size_t pair_splitk_floats(size_t rows, size_t n_out) {
  const size_t row_tiles = (rows + 255) / 256, tiles = row_tiles * ((n_out + 255) / 256);
  if (tiles > (size_t)kPairSplitkMaxTiles) return 0;
  for (int s : kPairSplitkLadder)
    if (tiles * s <= (size_t)kTileRound) return (size_t)s * (row_tiles * 256) * n_out;
  return 0;
}

// ---- split-bf16 weight-gradient group (gemm_tn_bf16x3.hip: launch_gemm_tn_group) -------------------------------------------
constexpr int kTnGroupMax = 8;   // products per launch
// one workgroup per CU over the whole group: at most a round of partial 256 x 256 tiles - or, where one product alone has more
// tiles than that, one slice of each product - + per product a row of column sums [n_out] per workgroup
inline size_t tn_group_floats(size_t one_slice_of_each, size_t n_out) {
  const size_t round = (size_t)kTileRound * kTile256Floats;
  return (round > one_slice_of_each ? round : one_slice_of_each) + (size_t)kTnGroupMax * kTileRound * n_out;
}

// ---- backward row kernels (backward_kernels.hip) ---------------------------------------------------------------------------
// LayerNorm backward: [kLnBwdMaxBlocks][3][D] per-block column sums, then [kLnBwdLevel1Rows][3][D] for their first reduction
// level (one row per kLnBwdGroup blocks); a pass that defers the second level keeps one more level-1 area per layer behind them
constexpr int kLnBwdMaxBlocks = 1024;
constexpr int kLnBwdGroup = 64;
constexpr int kLnBwdLevel1Rows = kLnBwdMaxBlocks / kLnBwdGroup;
inline size_t ln_bwd_block_floats(size_t D) { return (size_t)kLnBwdMaxBlocks * 3 * D; }
inline size_t ln_bwd_partial_floats(size_t D) { return ln_bwd_block_floats(D) + (size_t)kLnBwdLevel1Rows * 3 * D; }
inline size_t ln_bwd_level1(size_t D, int layer) { return ln_bwd_partial_floats(D) + (size_t)kLnBwdLevel1Rows * layer * 3 * D; }
// column sums: up to kColsumBatchMax of them per launch (ColsumBatch), each dealt over up to kColsumMaxSlices workgroups per
// 256 columns whose partial rows [slices][C] go to scratch
constexpr int kColsumMaxSlices = 64;
constexpr int kColsumBatchMax = 8;
inline size_t colsum_batch_floats(size_t C) { return (size_t)kColsumBatchMax * kColsumMaxSlices * C; }

}  // namespace drin
