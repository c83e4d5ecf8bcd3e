// Which 256 x 256 tile a work item of the LDS-DMA GEMMs (gemm_x3_planes.hip) computes.  Plain index arithmetic, shared by the
// kernels and by a host program that walks it (tests/host/tile_walk_main.cpp): no HIP header is needed to include this file.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRIN_TILE_WALK_FN __host__ __device__ __forceinline__
#else
#define DRIN_TILE_WALK_FN inline
#endif

namespace drin {
namespace x3p {

// XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (id % 8), each with its own L2.
// The column tiles of one row tile all stream the same A rows, so they should run on ONE XCD at the same
// time: XCD x takes a contiguous range of the tile sequence (column index fastest).  Without this the
// A operand is fetched from HBM once per column tile (3x for N = 768).  Placement only affects speed.
// Work item `id` of `count` whole tiles -> its position in the sequence (a bijection of [0, count)).
DRIN_TILE_WALK_FN unsigned xcd_tile_of_item(unsigned id, unsigned count) {
  const unsigned xcd = id & 7, k = id >> 3;
  const unsigned q = count >> 3, rem = count & 7;
  return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + k;
}

// A persistent grid of `wgs` workgroups over `count` tiles: workgroup g takes the work items g, g + wgs, g + 2 wgs, ... below
// `count`.  With wgs a multiple of 8 a workgroup keeps its XCD (g & 7) for every item, and the workgroups of one XCD walk that
// XCD's contiguous range side by side, so the column tiles of a row tile still meet in one L2; any other wgs is still exact.
// `tile0`: position of the range's first tile in the product's tile sequence (row_tile_begin * column tiles).
DRIN_TILE_WALK_FN unsigned persistent_items(unsigned g, unsigned wgs, unsigned count) { return g < count ? (count - g + wgs - 1) / wgs : 0u; }
DRIN_TILE_WALK_FN unsigned persistent_tile(unsigned g, unsigned wgs, unsigned i, unsigned count, unsigned tile0) {
  return tile0 + xcd_tile_of_item(g + i * wgs, count);
}

}  // namespace x3p
}  // namespace drin
