// The one bump allocator of every caller-owned workspace.  A layout struct describes its regions by take()-ing them from an
// Arena in a build(config); the entry point that sizes the workspace reads the total, the one that runs in it adds the same
// offsets to the caller's base.  Offsets and sizes are in floats; every region starts on a 256-byte boundary of the base.
// Host only, no HIP include (tests/host/workspace_main.cpp walks the layouts with a plain host compiler).
#pragma once
#include <stddef.h>

namespace drin {

struct Arena {
  static constexpr size_t kAlignFloats = 64;
  static constexpr size_t rounded(size_t floats) { return (floats + kAlignFloats - 1) & ~(kAlignFloats - 1); }
  size_t total = 0;   // floats taken so far
  size_t take(size_t floats) {
    const size_t at = total;
    total += rounded(floats);
    return at;
  }
  // the region at `offset` of the workspace that starts at `base`
  template <class T>
  static T* at(T* base, size_t offset) { return base + offset; }
};

// What a self-check states about a layout: regions that are live together, each with the floats its kernels index.
struct Region {
  const char* name;
  size_t offset, floats;
};
// The first region that does not start on a 256-byte boundary, ends past `total` or overlaps another one (empty regions hold
// nothing and overlap nothing); nullptr when all hold.
inline const char* first_bad_region(const Region* r, int n, size_t total) {
  for (int i = 0; i < n; ++i) {
    if (r[i].offset % Arena::kAlignFloats != 0 || r[i].offset + r[i].floats > total) return r[i].name;
    for (int j = 0; j < i; ++j)
      if (r[i].floats != 0 && r[j].floats != 0 && r[i].offset < r[j].offset + r[j].floats && r[j].offset < r[i].offset + r[i].floats)
        return r[i].name;
  }
  return nullptr;
}

}  // namespace drin
