// Host program over drin_amd/csrc/topk_layout.h: the one workspace description of the cosine top-k in its two forms, the
// single-table one (drin_table_topk: S = 1, summed = false) and the summed one (drin_table_topk_sum).  Over a grid of batches,
// table sizes, widths (776 takes the widen route in either precision), storages, precisions, k and chunks it checks that the layout
// builds, keeps the rules of kp, chunk and slice count, that every region is aligned, disjoint, inside the total and holds what
// its launches index (topk_layout_fault states those sizes itself), that the total is the sum of the regions - restated here, each
// rounded up to 64 floats - and that the single form is the summed form at S = 1 less exactly the rounded `scale` and `cos`
// regions, with every other region the same size and the chunk rule unchanged.
// Built and run by tests/test_topk_layout_host.py (no GPU, no HIP runtime).  Exit status 0 = all cases hold.
#include <cstdio>
#include <initializer_list>

#include "topk_layout.h"

using namespace drin;

static size_t r64(size_t floats) { return (floats + 63) / 64 * 64; }

static int fail(const char* what, const char* detail, bool summed, int S, int B, long long E, int k, long long chunk, int prec) {
  std::printf("%s: %s (%s, S %d B %d E %lld k %d chunk %lld precision %d)\n", what, detail, summed ? "summed" : "single", S, B, E, k, chunk, prec);
  return 1;
}

// the total as the sum of what the launches index, region by region
static size_t restated_total(const TopkLayout& W, const int* widths, const int* dtypes, int S, bool summed, int B, int prec) {
  const size_t kp = W.kp, Bp = (size_t)(B + 3) / 4 * 4, slices = (size_t)(W.chunk + DRIN_TOPK_SLICE - 1) / DRIN_TOPK_SLICE;
  size_t total = 0, widest = 0;
  for (int s = 0; s < S; ++s) {
    const bool bf16 = dtypes[s] == DRIN_FEAT_BF16, planes = bf16 && prec == DRIN_PREC_BF16X3 && widths[s] % 32 == 0;
    total += r64(Bp * widths[s]) + (summed ? r64(Bp) : 0) + r64((size_t)W.chunk * Bp) + (planes ? r64(Bp * widths[s]) : 0);
    if (bf16 && !planes && (size_t)widths[s] > widest) widest = widths[s];
  }
  total += summed ? r64((size_t)S * B * kp) : 0;
  total += r64(B * kp) + r64(B * kp * 2) + r64(slices * B * kp * 2) + r64(B * kp) + r64((size_t)W.chunk * widest);
  return total;
}

static int check(const int* widths, const int* dtypes, int S, bool summed, int B, int64_t E, int k, int64_t chunk, int prec, TopkLayout* W) {
  if (const char* bad = topk_layout_fault(widths, dtypes, S, summed, B, E, k, chunk, prec, W))
    return fail("layout", bad, summed, S, B, (long long)E, k, (long long)chunk, prec);
  if (W->total_floats != restated_total(*W, widths, dtypes, S, summed, B, prec))
    return fail("layout", "the total is not the sum of the rounded regions", summed, S, B, (long long)E, k, (long long)chunk, prec);
  return 0;
}

int main() {
  const int F = DRIN_FEAT_F32, H = DRIN_FEAT_BF16;
  int cases = 0;
  const int64_t tables[] = {300, 1500, 70000, 1000000};
  const int term_widths[][4] = {{16, 32, 768, 776}, {776, 16, 32, 768}, {768, 776, 16, 32}, {32, 768, 776, 16}};
  const int term_dtypes[][4] = {{F, F, F, F}, {H, H, H, H}, {H, F, H, F}, {F, H, F, H}};
  for (int B : {1, 3, 4, 5, 4096, 65535})
    for (int64_t E : tables)
      for (int k : {1, 64, 65, 256})
        for (int64_t chunk : {(int64_t)0, (int64_t)1, (int64_t)64, (int64_t)512})
          for (int prec : {(int)DRIN_PREC_F32, (int)DRIN_PREC_BF16X3}) {
            // the single form against the summed form at S = 1, per width and storage
            for (int D : {16, 32, 768, 776})
              for (int dt : {F, H}) {
                TopkLayout one, sum;
                if (check(&D, &dt, 1, false, B, E, k, chunk, prec, &one) || check(&D, &dt, 1, true, B, E, k, chunk, prec, &sum)) return 1;
                const size_t Bp = (size_t)(B + 3) / 4 * 4;
                if (one.scale[0] != one.block[0] || one.cos != one.keys)   // empty regions: the next one starts where they do
                  return fail("single form", "scale / cos take room", false, 1, B, (long long)E, k, (long long)chunk, prec);
                if (one.chunk != sum.chunk || one.num_slices != sum.num_slices || one.kp != sum.kp || one.Bp != sum.Bp ||
                    one.planes_floats[0] != sum.planes_floats[0] || one.widen_floats != sum.widen_floats)
                  return fail("single form", "chunk, slices, kp or the bf16 regions differ from the summed form at S = 1", false, 1, B, (long long)E, k,
                              (long long)chunk, prec);
                if (sum.total_floats - one.total_floats != r64(Bp) + r64((size_t)B * one.kp))
                  return fail("single form", "does not differ from the summed form at S = 1 by scale + cos", false, 1, B, (long long)E, k,
                              (long long)chunk, prec);
                cases += 2;
              }
            // the summed form, S = 2 .. 4 of mixed widths and storages
            for (int S = 2; S <= 4; ++S)
              for (const auto& w : term_widths)
                for (const auto& d : term_dtypes) {
                  TopkLayout W;
                  if (check(w, d, S, true, B, E, k, chunk, prec, &W)) return 1;
                  ++cases;
                }
          }
  // what does not build: a chunk past 2^30 rows, in either form
  {
    const int D = 16, dt = F;
    TopkLayout W;
    if (W.build(&D, &dt, 1, false, 3, (int64_t)1 << 40, 20, ((int64_t)1 << 30) + 1, DRIN_PREC_F32) ||
        W.build(&D, &dt, 1, true, 3, (int64_t)1 << 40, 20, (int64_t)1 << 31, DRIN_PREC_F32) ||
        !W.build(&D, &dt, 1, false, 3, (int64_t)1 << 40, 20, (int64_t)1 << 30, DRIN_PREC_F32))
      return std::printf("the chunk bound of 2^30 rows does not hold\n"), 1;
  }
  std::printf("topk layout: %d cases hold\n", cases);
  return 0;
}
