// The workspace of the cosine top-k against the whole table (table_topk.hip), in its two forms: ONE description.
//   summed = true   drin_table_topk_sum: S live terms, each with its padded mentions, its per-mention
//                   factors and its own block of dot products (block 0 takes the combined scores), and the S x [batch, kp]
//                   re-scored cosines
//   summed = false  drin_table_topk (section 24): that layout at S = 1 without the factors and the cosines - `scale` and `cos`
//                   are taken with 0 floats, which adds nothing to the arena
// bf16-stored rows (section 34) add per term on the plane route the hi / lo bf16 planes of its padded mentions, split once per
// call, and ONE widen region - a chunk of the widest term on the widen route as fp32; the terms' products run one after the other.
// Host only, no HIP include (tests/host/topk_layout_main.cpp walks it with a plain host compiler): arena.h, scratch_sizes.h and the
// public header are all it needs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/drin_hip.h"
#include "arena.h"
#include "scratch_sizes.h"

namespace drin {

constexpr int kTopkSlice = DRIN_TOPK_SLICE;                     // columns per partial workgroup
constexpr int kTopkMaxKp = 256;
constexpr int64_t kTopkBlockBudgetBytes = (int64_t)256 << 20;   // the default chunk bounds the score blocks to this
constexpr int64_t kTopkMaxChunk = (int64_t)1 << 30;

struct TopkLayout {
  size_t xpad[DRIN_TOPK_MAX_TERMS], scale[DRIN_TOPK_MAX_TERMS], block[DRIN_TOPK_MAX_TERMS];   // offsets in floats
  size_t planes[DRIN_TOPK_MAX_TERMS], planes_floats[DRIN_TOPK_MAX_TERMS];
  size_t cos, keys, rows, slices, scores, widen, widen_floats, total_floats;
  int64_t chunk, num_slices;
  int kp, Bp, S;

  static bool bf16_row(const int* dtypes, int s) { return dtypes != nullptr && dtypes[s] == DRIN_FEAT_BF16; }
  static bool plane_route(const int* widths, const int* dtypes, int s, int precision) {
    return bf16_row(dtypes, s) && nt_bf16_rows_as_planes(precision, widths[s], widths[s]);
  }
  // the widest term that takes the widen route (0: none does)
  static int widen_width(const int* widths, const int* dtypes, int terms, int precision) {
    int w = 0;
    for (int s = 0; s < terms; ++s)
      if (bf16_row(dtypes, s) && !plane_route(widths, dtypes, s, precision) && widths[s] > w) w = widths[s];
    return w;
  }

  // dtypes: how term s stores its rows (NULL: all fp32).  false: a region does not fit in size_t / the chunk is out of range
  bool build(const int* widths, const int* dtypes, int terms, bool summed, int batch, int64_t E, int k, int64_t chunk_entities, int precision) {
    kp = DRIN_TOPK_KP(k), Bp = (batch + 3) & ~3, S = terms;
    const int wide = widen_width(widths, dtypes, S, precision);
    if (chunk_entities > 0) {
      chunk = chunk_entities;
    } else {   // a multiple of 256 rows whose S blocks together - and the widened copy - stay inside the budget (at least 256)
      const int64_t row_bytes = (int64_t)4 * (wide > (int64_t)S * Bp ? wide : (int64_t)S * Bp);
      chunk = kTopkBlockBudgetBytes / row_bytes / 256 * 256;
      chunk = chunk < 256 ? 256 : chunk;
    }
    chunk = chunk < E ? chunk : E;
    if (chunk > kTopkMaxChunk) return false;
    num_slices = (chunk + kTopkSlice - 1) / kTopkSlice;
    // of floats: the blocks, the slice lists and the widened chunk are what can grow past size_t; beside them the regions sum to
    // less than 2^50 floats (Bp <= 2^16, widths < 2^31, kp <= 2^8), so the total and its byte count stay representable
    const size_t limit = SIZE_MAX / 64;
    auto fits = [&](size_t a, size_t b) { return a == 0 || b <= limit / a; };
    if (!fits((size_t)chunk * S, (size_t)Bp) || !fits((size_t)num_slices * 2, (size_t)batch * kp) || !fits((size_t)chunk, (size_t)wide)) return false;
    Arena A;
    for (int s = 0; s < S; ++s) {
      xpad[s] = A.take((size_t)Bp * widths[s]);
      scale[s] = A.take(summed ? (size_t)Bp : 0);
      block[s] = A.take((size_t)chunk * Bp);
    }
    cos = A.take(summed ? (size_t)S * batch * kp : 0);
    keys = A.take((size_t)batch * kp);
    rows = A.take((size_t)batch * kp * 2);
    slices = A.take((size_t)num_slices * batch * kp * 2);
    scores = A.take((size_t)batch * kp);
    for (int s = 0; s < S; ++s) {   // (fp32 terms: empty regions behind the old ones - the old offsets and the old total)
      planes_floats[s] = plane_route(widths, dtypes, s, precision) ? (size_t)Bp * widths[s] : 0;
      planes[s] = A.take(planes_floats[s]);
    }
    widen_floats = (size_t)chunk * wide;
    widen = A.take(widen_floats);
    total_floats = A.total;
    return true;
  }
};

// The self-check of one case: the rules of kp, chunk and slice count, and every region with the floats its launches index - stated
// here, not read from build() - aligned, disjoint and inside the total.  nullptr when all hold; else "build", "rules" or the region.
inline const char* topk_layout_fault(const int* widths, const int* dtypes, int S, bool summed, int batch, int64_t E, int k,
                                     int64_t chunk_entities, int precision, TopkLayout* out = nullptr) {
  TopkLayout W;
  if (!W.build(widths, dtypes, S, summed, batch, E, k, chunk_entities, precision)) return "build";
  if (out != nullptr) *out = W;
  const size_t B = batch, kp = W.kp;
  if (W.kp < k || W.kp > kTopkMaxKp || (W.kp & (W.kp - 1)) || W.Bp < batch || W.Bp % 4 || W.Bp > batch + 3 || W.chunk < 1 || W.chunk > E ||
      W.num_slices * kTopkSlice < W.chunk ||
      (chunk_entities == 0 && W.chunk != E &&
       (W.chunk % 256 ||
        (W.chunk > 256 && (W.chunk * W.Bp * 4 * S > kTopkBlockBudgetBytes || (int64_t)W.widen_floats * 4 > kTopkBlockBudgetBytes)))))
    return "rules";
  Region ws[4 * DRIN_TOPK_MAX_TERMS + 6];
  int n = 0, widest = 0;
  for (int s = 0; s < S; ++s) {
    // the padded mentions, their factors 1 / max(|x|, eps) (the summed form alone), one block of dot products
    ws[n++] = {"xpad", W.xpad[s], (size_t)W.Bp * widths[s]};
    ws[n++] = {"scale", W.scale[s], summed ? (size_t)W.Bp : 0};
    ws[n++] = {"block", W.block[s], (size_t)W.chunk * W.Bp};
    // what the routes index: hi + lo planes of xpad (2 bf16 = 1 float per element), or a widened chunk of the widest such term
    const bool bf16 = dtypes != nullptr && dtypes[s] == DRIN_FEAT_BF16;
    const bool as_planes = bf16 && nt_bf16_rows_as_planes(precision, widths[s], widths[s]);
    ws[n++] = {"planes", W.planes[s], as_planes ? (size_t)W.Bp * widths[s] : 0};
    if (bf16 && !as_planes && widths[s] > widest) widest = widths[s];
  }
  // the widened chunk, the re-scored cosines per term (summed), the running list, every slice's list, the final scores
  ws[n++] = {"widen", W.widen, (size_t)W.chunk * widest};
  ws[n++] = {"cos", W.cos, summed ? (size_t)S * B * kp : 0};
  ws[n++] = {"keys", W.keys, B * kp};
  ws[n++] = {"rows", W.rows, B * kp * 2};
  ws[n++] = {"slices", W.slices, (size_t)((W.chunk + kTopkSlice - 1) / kTopkSlice) * B * kp * 2};
  ws[n++] = {"scores", W.scores, B * kp};
  return first_bad_region(ws, n, W.total_floats);
}

}  // namespace drin
