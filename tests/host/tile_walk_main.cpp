// Host program over drin_amd/csrc/tile_walk.h: the persistent grid's walk over a range of 256 x 256 tiles visits every tile of the
// range exactly once and none outside it; with a grid that is a multiple of 8 every workgroup stays on its XCD's contiguous share.
// Built and run by tests/test_tile_walk_host.py (no GPU, no HIP runtime).  Exit status 0 = all cases hold.
#include <cstdio>
#include <vector>

#include "tile_walk.h"

using namespace drin::x3p;

static int check(unsigned count, unsigned nx, unsigned wgs, unsigned row_tile_begin) {
  const unsigned tile0 = row_tile_begin * nx;
  std::vector<int> seen(tile0 + count + 64, 0);
  unsigned visits = 0;
  for (unsigned g = 0; g < wgs; ++g) {
    // what the kernel runs: for (id = g; id < count; id += wgs)
    unsigned items = 0;
    for (unsigned id = g; id < count; id += wgs, ++items) {
      const unsigned t = tile0 + xcd_tile_of_item(id, count);
      if (t != persistent_tile(g, wgs, items, count, tile0)) return std::printf("count %u wgs %u: item %u of workgroup %u disagrees\n", count, wgs, items, g), 1;
      if (t < tile0 || t >= tile0 + count) return std::printf("count %u wgs %u: tile %u outside [%u, %u)\n", count, wgs, t, tile0, tile0 + count), 1;
      ++seen[t];
      ++visits;
      if (wgs % 8 == 0) {   // XCD g & 7 owns the contiguous share [start, start + share)
        const unsigned x = g & 7, q = count >> 3, rem = count & 7;
        const unsigned start = x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q, share = q + (x < rem ? 1u : 0u);
        if (t - tile0 < start || t - tile0 >= start + share) return std::printf("count %u wgs %u: workgroup %u left its XCD's share\n", count, wgs, g), 1;
      }
    }
    if (items != persistent_items(g, wgs, count)) return std::printf("count %u wgs %u: workgroup %u item count\n", count, wgs, g), 1;
  }
  if (visits != count) return std::printf("count %u wgs %u: %u visits\n", count, wgs, visits), 1;
  for (unsigned t = 0; t < seen.size(); ++t)
    if (seen[t] != ((t >= tile0 && t < tile0 + count) ? 1 : 0)) return std::printf("count %u wgs %u: tile %u seen %d times\n", count, wgs, t, seen[t]), 1;
  return 0;
}

int main() {
  const unsigned nx = 3;
  int cases = 0;
  for (unsigned tiles : {1u, 7u, 8u, 9u, 153u, 4848u})
    for (unsigned wgs : {1u, 8u, 64u})
      for (unsigned begin : {0u, 5u}) {
        if (check(tiles, nx, wgs, begin)) return 1;
        ++cases;
      }
  std::printf("tile walk: %d cases hold\n", cases);
  return 0;
}
