// The keep mask of the attention dropout (drin_attention_dropout_*): a pure function of (seed, call, element index),
// the same on the host and on the device.  This file is the contract; tests regenerate masks through
// drin_attention_dropout_keep, which calls dropout_keep below for every element.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), key = the 64-bit seed
// (low word, high word), counter = (low word of e >> 2, high word of e >> 2, low word of call, high word of call) with
//   e = ((b * H + h) * Lq + i) * Lk + j
// the flat index of attention weight (mention b, head h, query i, key j) in a [B, H, Lq, Lk] array.  One evaluation
// yields the four uniform 32-bit words of the elements 4 (e >> 2) .. 4 (e >> 2) + 3; element e takes word e & 3.
// Element e is KEPT iff its word >= dropout_threshold(p) = (uint32_t)llrint((double)p * 2^32), p in [0, 1): the kept
// share is 1 - p to within 2^-32, and p = 0 keeps everything.  A kept weight is multiplied by 1 / (1 - p).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRIN_HD __host__ __device__
#else
#define DRIN_HD
#endif

namespace drin {

struct Philox4 {
  uint32_t w[4];
};

DRIN_HD inline Philox4 philox4x32_10(uint64_t seed, uint64_t call, uint64_t quad) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = (uint32_t)quad, c1 = (uint32_t)(quad >> 32), c2 = (uint32_t)call, c3 = (uint32_t)(call >> 32);
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the uniform 32-bit word of element e
DRIN_HD inline uint32_t dropout_word(uint64_t seed, uint64_t call, uint64_t e) {
  const Philox4 r = philox4x32_10(seed, call, e >> 2);
  const uint32_t lane = (uint32_t)e & 3u;
  return lane == 0 ? r.w[0] : lane == 1 ? r.w[1] : lane == 2 ? r.w[2] : r.w[3];
}

// host side: the threshold of a rate p in [0, 1)
inline uint32_t dropout_threshold(float p) { return (uint32_t)llrint((double)p * 4294967296.0); }

DRIN_HD inline bool dropout_keep(uint64_t seed, uint64_t call, uint64_t e, uint32_t threshold) {
  return dropout_word(seed, call, e) >= threshold;
}

}  // namespace drin
