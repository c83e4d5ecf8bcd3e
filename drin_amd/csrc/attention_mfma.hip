// The softmax-attention core on the matrix pipes: the forward and the backward of attention_fma.hip's
// FMA core with every product as the library's split-bf16 form - each fp32 operand x is hi = bf16(x), lo = bf16(x - hi),
// and hi hi + hi lo + lo hi accumulate in fp32 through v_mfma_f32_16x16x32_bf16.  Softmax, the running max and sum, lse,
// delta and ds = p (dp - delta) stay fp32; the exponentials are exp2 on scores in log2 units.  An opt-in
// (drin_attention_mfma_fwd / drin_attention_mfma_bwd): the FMA core keeps its entry points and its bits.
//
// One workgroup = 4 waves owns 64 rows, 16 per wave (32 rows at head dims above 128: struct Shape), and walks the other side
// in tiles of 32 (one MFMA K step):
//   k_attention_mfma          owns query rows, walks key tiles:    S^T = K Q^T,  O^T += V^T P^T
//   k_attention_mfma_bwd_dq   owns query rows, walks key tiles:    S^T = K Q^T,  dP^T = V dO^T,  dQ^T += K^T dS^T
//   k_attention_mfma_bwd_dkv  owns keys,       walks query tiles:  S = Q K^T,    dP = dO V^T,    dV^T += dO^T P,  dK^T += Q^T dS
// No atomics, no scratch: a workgroup alone writes the rows it owns, the same bits every run.
//
// Operands.  The rows a wave owns (Q; Q and dO; K and V) are its B fragments, loaded from global memory straight into the
// fragment layout (lane l: row l & 15, columns 32 s + 8 (l >> 4) .. + 7 of K step s), split in registers and kept for the
// whole kernel (the wide backward kernels read them from planes in LDS instead).  The walked tile (K and V; Q and dO) is staged once per tile through registers - split there - into two
// bf16 planes [32][dp + 8] per operand, dp = head dim rounded up to 32; rows past the tile's end and columns past the head
// dim are written as zeros, never left stale (NaN x 0 is NaN in an MFMA).  That ONE row-major image serves both reads: as
// the A operand of the first products one ds_read_b128 per lane (row stride 2 dp + 16 bytes: the 16 rows of a read meet 16
// different bank quads), and as the A operand of the second products - summed over the tile's ROWS - by the transposing
// read ds_read_b64_tr_b16 (4 rows x 16 columns per 16-lane group, delivered column-major).
// The first products are oriented so that the tile's row index lands in the accumulator's registers (element r of lane l:
// tile row 16 mt + 4 (l >> 4) + r, owned row l & 15): p and ds are computed and split right there and ARE the B fragments
// of the second products, in the K order (element j of lane group g: tile row 16 (j >> 2) + 4 g + (j & 3)) that the two
// transposing reads of rows 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3 deliver.  A lane holds one owned row: its softmax
// statistics, lse and delta are per-lane scalars, and a row's max and sum cross the four 16-lane groups by two exchanges.
// Masked keys, keys past k_len, rows past q_len and rows without a kept key take p = ds = 0 by a select before the split.
#include "attention_common.h"
#include "device_utils.h"

namespace drin {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 32;   // rows of a staged tile: one K step of the second products
// Head dims <= 128 (DPMAX = 128): a workgroup owns 64 rows, 16 per wave, and a wave accumulates all output columns.
// Wider (DPMAX = 256): 32 rows, and the two waves that share 16 rows take one half of the output columns each (both form
// the same p / ds); the backward kernels then keep the owned rows' planes in LDS instead of registers.  Either way a
// kernel stays under 256 registers per lane (two waves per SIMD).
template <int DPMAX>
struct Shape {
  static constexpr int KS = DPMAX / 32;          // K steps of the first products
  static constexpr int DS = DPMAX > 128 ? 2 : 1; // waves that share 16 owned rows
  static constexpr int NTW = DPMAX / 16 / DS;    // 16-column output tiles per wave
  static constexpr int OWN = 64 / DS;            // rows a workgroup owns
  static constexpr bool OWN_LDS = DPMAX > 128;   // backward: owned rows' fragments are read from LDS
};
constexpr float kLog2e = 1.44269504088896340736f, kLn2 = 0.69314718055994530942f;

struct Frag {
  bf16x8 hi, lo;
};

// c += a b in split-bf16: the two cross terms first, then hi hi
__device__ __forceinline__ f32x4 mfma3(const Frag& a, const Frag& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.lo, b.hi, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.hi, c, 0, 0, 0);
}

// columns c .. c + 3 of a global row of dh floats; zeros past dh and for a row that is not there.  vec: dh % 4 == 0 and
// the rows are 16-byte aligned.
__device__ __forceinline__ float4 load4(const float* row, int c, bool ok, int dh, bool vec) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok && c < dh) {
    if (vec) {
      x = ld4(row + c);
    } else {
      x.x = row[c];
      if (c + 1 < dh) x.y = row[c + 1];
      if (c + 2 < dh) x.z = row[c + 2];
      if (c + 3 < dh) x.w = row[c + 3];
    }
  }
  return x;
}

__device__ __forceinline__ Frag split8(float4 a, float4 b) {
  uint4 h, l;
  split_bf16_pair(a.x, a.y, h.x, l.x);
  split_bf16_pair(a.z, a.w, h.y, l.y);
  split_bf16_pair(b.x, b.y, h.z, l.z);
  split_bf16_pair(b.z, b.w, h.w, l.w);
  return Frag{__builtin_bit_cast(bf16x8, h), __builtin_bit_cast(bf16x8, l)};
}

// the fragment of an owned row: columns c .. c + 7 times mul
__device__ __forceinline__ Frag global_frag(const float* row, bool ok, int c, int dh, bool vec, float mul) {
  return split8(load4(row, c, ok, dh, vec) * mul, load4(row, c + 4, ok, dh, vec) * mul);
}

// `valid` rows x dh columns of a row-major global block -> the hi and lo planes [kTile][sd] of a tile; rows valid ..
// kTile - 1 and columns dh .. dp - 1 are zeros
__device__ __forceinline__ void stage_planes(unsigned short* hi, unsigned short* lo, int sd, const float* src, int64_t ld, int valid,
                                             int dh, int dp, bool vec) {
  const int n4 = dp >> 2;
  for (int i = threadIdx.x; i < kTile * n4; i += 256) {
    const int r = i / n4, c = (i - r * n4) * 4;
    const float4 x = load4(src + r * ld, c, r < valid, dh, vec);
    uint2 h, l;
    split_bf16_pair(x.x, x.y, h.x, l.x);
    split_bf16_pair(x.z, x.w, h.y, l.y);
    *reinterpret_cast<uint2*>(hi + r * sd + c) = h;
    *reinterpret_cast<uint2*>(lo + r * sd + c) = l;
  }
}

// A fragment of tile rows 16 mt .. + 15, K step s (columns): off = (16 mt + (lane & 15)) sd + 32 s + 8 (lane >> 4)
__device__ __forceinline__ Frag row_frag(const unsigned short* hi, const unsigned short* lo, int off) {
  return Frag{*reinterpret_cast<const bf16x8*>(hi + off), *reinterpret_cast<const bf16x8*>(lo + off)};
}

// A fragment of the TRANSPOSED tile: fragment row = tile column 16 nt + (lane & 15), K = the tile's rows in the order of
// the file comment.  Every lane supplies the address of 4 columns of one row of its group's 4 x 16 block (all 64 lanes
// active: callers branch on workgroup-uniform conditions only): off = (4 g + ((lane & 15) >> 2)) sd + 16 nt + 4 (lane & 3).
__device__ __forceinline__ bf16x8 tr_plane(const unsigned short* img, int off, int sd) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off + 16 * sd));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ Frag tr_frag(const unsigned short* hi, const unsigned short* lo, int off, int sd) {
  return Frag{tr_plane(hi, off, sd), tr_plane(lo, off, sd)};
}

__device__ __forceinline__ float4 as4(f32x4 v) { return make_float4(v[0], v[1], v[2], v[3]); }

// a value of every lane's owned row combined over the four 16-lane groups that share it
__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// 4 consecutive columns of an owned output row; ovec: the destination rows are 16-byte aligned and dh % 4 == 0
__device__ __forceinline__ void store4(float* row, int d, f32x4 v, float mul, int dh, bool ovec) {
  if (ovec) {
    if (d < dh) st4(row + d, as4(v) * mul);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (d + r < dh) row[d + r] = v[r] * mul;
  }
}

// the LDS of one workgroup: four planes [kTile][sd], 64 words of per-row values and, where the owned rows live in LDS,
// four more planes [kTile][sd] (words + 64)
struct Tile {
  unsigned short *ah, *al, *bh, *bl;
  void* words;
};
__device__ __forceinline__ Tile carve_tile(void* base, int sd) {
  unsigned short* p = reinterpret_cast<unsigned short*>(base);
  const int n = kTile * sd;
  return Tile{p, p + n, p + 2 * n, p + 3 * n, p + 4 * n};
}

template <int DPMAX, bool DROP>
__global__ void __launch_bounds__(256, 2) k_attention_mfma(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                        const float* __restrict__ v, int64_t ldv, const int64_t* __restrict__ mask,
                                                        float* __restrict__ out, int64_t ldo, float* __restrict__ lse, int Lq, int Lk,
                                                        int dh, float q_scale, int vec, int ovec, DropArgs drop) {
  typedef Shape<DPMAX> SH;
  constexpr int KS = SH::KS, NT = SH::NTW;
  extern __shared__ uint4 smem[];
  const int dp = (dh + 31) & ~31, sd = dp + 8, nks = dp >> 5, nnt = (dh + 15) >> 4;
  const Tile t = carve_tile(smem, sd);   // a: K, b: V
  int* keep = reinterpret_cast<int*>(t.words);
  const int b = blockIdx.z, h = blockIdx.y, H = gridDim.y;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
  const int nt0 = (w % SH::DS) * NT;   // this wave's first output tile
  const int qi = blockIdx.x * SH::OWN + (w / SH::DS) * 16 + c16;
  const bool q_ok = qi < Lq;
  const float ninf = -__builtin_inff();
  const float* qrow = q + ((int64_t)b * Lq + qi) * ldq + (int64_t)h * dh;
  Frag qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = global_frag(qrow, q_ok, 32 * s + 8 * g, dh, vec != 0, q_scale);
  k += (int64_t)b * Lk * ldk + (int64_t)h * dh;
  v += (int64_t)b * Lk * ldv + (int64_t)h * dh;
  if (mask != nullptr) mask += (int64_t)b * Lk;

  f32x4 o[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) o[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = ninf, l = 0.f;   // l: this lane's share of the row sum
  const int row_off = c16 * sd + 8 * g, tr_off = (4 * g + (c16 >> 2)) * sd + 4 * (lane & 3);

  for (int j0 = 0; j0 < Lk; j0 += kTile) {
    const int jn = Lk - j0 < kTile ? Lk - j0 : kTile;
    __syncthreads();   // the previous tile has been read (first tile: nothing)
    stage_planes(t.ah, t.al, sd, k + j0 * ldk, ldk, jn, dh, dp, vec != 0);
    stage_planes(t.bh, t.bl, sd, v + j0 * ldv, ldv, jn, dh, dp, vec != 0);
    if (threadIdx.x < kTile) keep[threadIdx.x] = (int)threadIdx.x < jn && (mask == nullptr || mask[j0 + threadIdx.x] != 0);
    __syncthreads();
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      if (ks < nks) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) s[mt] = mfma3(row_frag(t.ah, t.al, row_off + mt * 16 * sd + 32 * ks), qf[ks], s[mt]);
      }
    float sr[8];
    float tmax = ninf;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int4 kp = *reinterpret_cast<const int4*>(keep + 16 * mt + 4 * g);
      sr[4 * mt + 0] = kp.x ? s[mt][0] : ninf;
      sr[4 * mt + 1] = kp.y ? s[mt][1] : ninf;
      sr[4 * mt + 2] = kp.z ? s[mt][2] : ninf;
      sr[4 * mt + 3] = kp.w ? s[mt][3] : ninf;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) tmax = fmaxf(tmax, sr[e]);
    const float mn = fmaxf(m, group_max(tmax));
    const bool none = mn == ninf;   // no kept key so far
    const float alpha = none ? 1.0f : exp2f(m - mn);
    float p[8], psum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p[e] = none ? 0.f : exp2f(sr[e] - mn);
      psum += p[e];
    }
    l = fmaf(l, alpha, psum);
    m = mn;
    if constexpr (DROP) {
      const uint64_t e0 = (((uint64_t)b * H + h) * Lq + qi) * Lk + j0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        p[e] = dropout_keep(drop.seed, drop.call, e0 + 16 * (e >> 2) + 4 * g + (e & 3), drop.threshold) ? p[e] * drop.scale : 0.f;
    }
    const Frag pf = split8(make_float4(p[0], p[1], p[2], p[3]), make_float4(p[4], p[5], p[6], p[7]));
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (nt0 + nt < nnt) o[nt] = mfma3(tr_frag(t.bh, t.bl, tr_off + 16 * (nt0 + nt), sd), pf, o[nt] * alpha);
  }
  l = group_sum(l);
  if (!q_ok) return;
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  if (lse != nullptr && g == 0 && nt0 == 0)   // natural log of the row's sum of exp(score); m is in log2 units (q_scale)
    lse[((int64_t)b * H + h) * Lq + qi] = l > 0.f ? (m + log2f(l)) * kLn2 : ninf;
  float* orow = out + ((int64_t)b * Lq + qi) * ldo + (int64_t)h * dh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    if (nt0 + nt < nnt) store4(orow, 16 * (nt0 + nt) + 4 * g, o[nt], inv, dh, ovec != 0);
}

// p and ds of the 8 (tile row, owned row) pairs of a lane from the two accumulators; e0: the dropout index of (tile row 0
// of the pair's orientation, this lane), e_step: its step per tile row
template <bool DROP>
__device__ __forceinline__ void probs8(const f32x4* s, const f32x4* dp, const bool* on, const float* l2, const float* dl, float q_scale,
                                       const DropArgs& drop, uint64_t e0, uint64_t e_step, int g, float* p, float* ds) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float pe = on[e] ? exp2f(fmaf(s[e >> 2][e & 3], q_scale, -l2[e])) : 0.f;
    if constexpr (DROP) {
      const float mm = dropout_keep(drop.seed, drop.call, e0 + e_step * (16 * (e >> 2) + 4 * g + (e & 3)), drop.threshold) ? drop.scale : 0.f;
      p[e] = pe * mm;
      ds[e] = on[e] ? pe * (dp[e >> 2][e & 3] * mm - dl[e]) : 0.f;
    } else {
      p[e] = pe;
      ds[e] = on[e] ? pe * (dp[e >> 2][e & 3] - dl[e]) : 0.f;
    }
  }
}

template <int DPMAX, bool DROP>
__global__ void __launch_bounds__(256, 2) k_attention_mfma_bwd_dq(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                               int64_t ldk, const float* __restrict__ v, int64_t ldv,
                                                               const int64_t* __restrict__ mask, const float* __restrict__ lse,
                                                               const float* __restrict__ dout, int64_t lddo,
                                                               const float* __restrict__ delta, float* __restrict__ dq, int64_t lddq,
                                                               int Lq, int Lk, int dh, float q_scale, float out_scale, int vec, int ovec,
                                                               DropArgs drop) {
  typedef Shape<DPMAX> SH;
  constexpr int KS = SH::KS, NT = SH::NTW;
  extern __shared__ uint4 smem[];
  const int dp = (dh + 31) & ~31, sd = dp + 8, nks = dp >> 5, nnt = (dh + 15) >> 4;
  const Tile t = carve_tile(smem, sd);   // a: K, b: V
  int* keep = reinterpret_cast<int*>(t.words);
  const Tile own = carve_tile(keep + 64, sd);   // a: Q, b: dO of the owned rows (OWN_LDS)
  const int b = blockIdx.z, h = blockIdx.y, H = gridDim.y;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
  const int nt0 = (w % SH::DS) * NT;
  const int own0 = blockIdx.x * SH::OWN, qi = own0 + (w / SH::DS) * 16 + c16;
  const bool q_ok = qi < Lq;
  const float ninf = -__builtin_inff();
  const int own_off = ((w / SH::DS) * 16 + c16) * sd + 8 * g;
  Frag qf[SH::OWN_LDS ? 1 : KS], gf[SH::OWN_LDS ? 1 : KS];
  if constexpr (SH::OWN_LDS) {   // (the tile loop's first barrier comes before these planes are read)
    const int n = Lq - own0 < kTile ? Lq - own0 : kTile;
    stage_planes(own.ah, own.al, sd, q + ((int64_t)b * Lq + own0) * ldq + (int64_t)h * dh, ldq, n, dh, dp, vec != 0);
    stage_planes(own.bh, own.bl, sd, dout + ((int64_t)b * Lq + own0) * lddo + (int64_t)h * dh, lddo, n, dh, dp, vec != 0);
  } else {
    const float* qrow = q + ((int64_t)b * Lq + qi) * ldq + (int64_t)h * dh;
    const float* grow = dout + ((int64_t)b * Lq + qi) * lddo + (int64_t)h * dh;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[s] = global_frag(qrow, q_ok, 32 * s + 8 * g, dh, vec != 0, 1.0f);
      gf[s] = global_frag(grow, q_ok, 32 * s + 8 * g, dh, vec != 0, 1.0f);
    }
  }
  const int64_t stat = ((int64_t)b * H + h) * Lq + qi;
  const float lse2 = q_ok ? lse[stat] * kLog2e : ninf, dl1 = q_ok ? delta[stat] : 0.f;
  k += (int64_t)b * Lk * ldk + (int64_t)h * dh;
  v += (int64_t)b * Lk * ldv + (int64_t)h * dh;
  if (mask != nullptr) mask += (int64_t)b * Lk;

  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int row_off = c16 * sd + 8 * g, tr_off = (4 * g + (c16 >> 2)) * sd + 4 * (lane & 3);
  float l2[8], dl[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) l2[e] = lse2, dl[e] = dl1;

  for (int j0 = 0; j0 < Lk; j0 += kTile) {
    const int jn = Lk - j0 < kTile ? Lk - j0 : kTile;
    __syncthreads();   // the previous tile has been read (first tile: nothing)
    stage_planes(t.ah, t.al, sd, k + j0 * ldk, ldk, jn, dh, dp, vec != 0);
    stage_planes(t.bh, t.bl, sd, v + j0 * ldv, ldv, jn, dh, dp, vec != 0);
    if (threadIdx.x < kTile) keep[threadIdx.x] = (int)threadIdx.x < jn && (mask == nullptr || mask[j0 + threadIdx.x] != 0);
    __syncthreads();
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 dpv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      if (ks < nks) {
        const Frag qb = SH::OWN_LDS ? row_frag(own.ah, own.al, own_off + 32 * ks) : qf[SH::OWN_LDS ? 0 : ks];
        const Frag gb = SH::OWN_LDS ? row_frag(own.bh, own.bl, own_off + 32 * ks) : gf[SH::OWN_LDS ? 0 : ks];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          s[mt] = mfma3(row_frag(t.ah, t.al, row_off + mt * 16 * sd + 32 * ks), qb, s[mt]);
          dpv[mt] = mfma3(row_frag(t.bh, t.bl, row_off + mt * 16 * sd + 32 * ks), gb, dpv[mt]);
        }
      }
    bool on[8];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int4 kp = *reinterpret_cast<const int4*>(keep + 16 * mt + 4 * g);
      const bool row = lse2 != ninf;
      on[4 * mt + 0] = row && kp.x, on[4 * mt + 1] = row && kp.y, on[4 * mt + 2] = row && kp.z, on[4 * mt + 3] = row && kp.w;
    }
    float p[8], ds[8];
    probs8<DROP>(s, dpv, on, l2, dl, q_scale, drop, (((uint64_t)b * H + h) * Lq + qi) * Lk + j0, 1, g, p, ds);
    const Frag df = split8(make_float4(ds[0], ds[1], ds[2], ds[3]), make_float4(ds[4], ds[5], ds[6], ds[7]));
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (nt0 + nt < nnt) acc[nt] = mfma3(tr_frag(t.ah, t.al, tr_off + 16 * (nt0 + nt), sd), df, acc[nt]);
  }
  if (!q_ok) return;
  float* orow = dq + ((int64_t)b * Lq + qi) * lddq + (int64_t)h * dh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    if (nt0 + nt < nnt) store4(orow, 16 * (nt0 + nt) + 4 * g, acc[nt], out_scale, dh, ovec != 0);
}

template <int DPMAX, bool DROP>
__global__ void __launch_bounds__(256, 2) k_attention_mfma_bwd_dkv(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                                int64_t ldk, const float* __restrict__ v, int64_t ldv,
                                                                const int64_t* __restrict__ mask, const float* __restrict__ lse,
                                                                const float* __restrict__ dout, int64_t lddo,
                                                                const float* __restrict__ delta, float* __restrict__ dk, int64_t lddk,
                                                                float* __restrict__ dv, int64_t lddv, int Lq, int Lk, int dh,
                                                                float q_scale, float out_scale, int vec, int ovec, DropArgs drop) {
  typedef Shape<DPMAX> SH;
  constexpr int KS = SH::KS, NT = SH::NTW;
  extern __shared__ uint4 smem[];
  const int dp = (dh + 31) & ~31, sd = dp + 8, nks = dp >> 5, nnt = (dh + 15) >> 4;
  const Tile t = carve_tile(smem, sd);   // a: Q, b: dO
  float* lse2s = reinterpret_cast<float*>(t.words);
  float* dls = lse2s + kTile;
  const Tile own = carve_tile(lse2s + 64, sd);   // a: K, b: V of the owned keys (OWN_LDS)
  const int b = blockIdx.z, h = blockIdx.y, H = gridDim.y;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
  const int nt0 = (w % SH::DS) * NT;
  const int own0 = blockIdx.x * SH::OWN, kj = own0 + (w / SH::DS) * 16 + c16;
  const bool k_ok = kj < Lk;
  const float ninf = -__builtin_inff();
  const int own_off = ((w / SH::DS) * 16 + c16) * sd + 8 * g;
  Frag kf[SH::OWN_LDS ? 1 : KS], vf[SH::OWN_LDS ? 1 : KS];
  if constexpr (SH::OWN_LDS) {   // (the tile loop's first barrier comes before these planes are read)
    const int n = Lk - own0 < kTile ? Lk - own0 : kTile;
    stage_planes(own.ah, own.al, sd, k + ((int64_t)b * Lk + own0) * ldk + (int64_t)h * dh, ldk, n, dh, dp, vec != 0);
    stage_planes(own.bh, own.bl, sd, v + ((int64_t)b * Lk + own0) * ldv + (int64_t)h * dh, ldv, n, dh, dp, vec != 0);
  } else {
    const float* krow = k + ((int64_t)b * Lk + kj) * ldk + (int64_t)h * dh;
    const float* vrow = v + ((int64_t)b * Lk + kj) * ldv + (int64_t)h * dh;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      kf[s] = global_frag(krow, k_ok, 32 * s + 8 * g, dh, vec != 0, 1.0f);
      vf[s] = global_frag(vrow, k_ok, 32 * s + 8 * g, dh, vec != 0, 1.0f);
    }
  }
  const bool kept = k_ok && (mask == nullptr || mask[(int64_t)b * Lk + kj] != 0);
  q += (int64_t)b * Lq * ldq + (int64_t)h * dh;
  dout += (int64_t)b * Lq * lddo + (int64_t)h * dh;
  lse += ((int64_t)b * H + h) * Lq;
  delta += ((int64_t)b * H + h) * Lq;

  f32x4 ak[NT], av[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) ak[nt] = f32x4{0.f, 0.f, 0.f, 0.f}, av[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int row_off = c16 * sd + 8 * g, tr_off = (4 * g + (c16 >> 2)) * sd + 4 * (lane & 3);

  for (int q0 = 0; q0 < Lq; q0 += kTile) {
    const int q_valid = Lq - q0 < kTile ? Lq - q0 : kTile;
    __syncthreads();   // the previous tile has been read (first tile: nothing)
    stage_planes(t.ah, t.al, sd, q + q0 * ldq, ldq, q_valid, dh, dp, vec != 0);
    stage_planes(t.bh, t.bl, sd, dout + q0 * lddo, lddo, q_valid, dh, dp, vec != 0);
    if (threadIdx.x < kTile) {   // rows past Lq: -inf, 0
      const bool ok = (int)threadIdx.x < q_valid;
      lse2s[threadIdx.x] = ok ? lse[q0 + threadIdx.x] * kLog2e : ninf;
      dls[threadIdx.x] = ok ? delta[q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 dpv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      if (ks < nks) {
        const Frag kb = SH::OWN_LDS ? row_frag(own.ah, own.al, own_off + 32 * ks) : kf[SH::OWN_LDS ? 0 : ks];
        const Frag vb = SH::OWN_LDS ? row_frag(own.bh, own.bl, own_off + 32 * ks) : vf[SH::OWN_LDS ? 0 : ks];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          s[mt] = mfma3(row_frag(t.ah, t.al, row_off + mt * 16 * sd + 32 * ks), kb, s[mt]);
          dpv[mt] = mfma3(row_frag(t.bh, t.bl, row_off + mt * 16 * sd + 32 * ks), vb, dpv[mt]);
        }
      }
    float l2[8], dl[8];
    bool on[8];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const float4 a = ld4(lse2s + 16 * mt + 4 * g), d = ld4(dls + 16 * mt + 4 * g);
      l2[4 * mt + 0] = a.x, l2[4 * mt + 1] = a.y, l2[4 * mt + 2] = a.z, l2[4 * mt + 3] = a.w;
      dl[4 * mt + 0] = d.x, dl[4 * mt + 1] = d.y, dl[4 * mt + 2] = d.z, dl[4 * mt + 3] = d.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) on[e] = kept && l2[e] != ninf;
    float p[8], ds[8];
    probs8<DROP>(s, dpv, on, l2, dl, q_scale, drop, (((uint64_t)b * H + h) * Lq + q0) * Lk + kj, (uint64_t)Lk, g, p, ds);
    const Frag pf = split8(make_float4(p[0], p[1], p[2], p[3]), make_float4(p[4], p[5], p[6], p[7]));
    const Frag df = split8(make_float4(ds[0], ds[1], ds[2], ds[3]), make_float4(ds[4], ds[5], ds[6], ds[7]));
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (nt0 + nt < nnt) {
        av[nt] = mfma3(tr_frag(t.bh, t.bl, tr_off + 16 * (nt0 + nt), sd), pf, av[nt]);
        ak[nt] = mfma3(tr_frag(t.ah, t.al, tr_off + 16 * (nt0 + nt), sd), df, ak[nt]);
      }
  }
  if (!k_ok) return;
  float* krow = dk + ((int64_t)b * Lk + kj) * lddk + (int64_t)h * dh;
  float* vrow = dv + ((int64_t)b * Lk + kj) * lddv + (int64_t)h * dh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    if (nt0 + nt < nnt) {
      store4(krow, 16 * (nt0 + nt) + 4 * g, ak[nt], out_scale, dh, ovec != 0);
      store4(vrow, 16 * (nt0 + nt) + 4 * g, av[nt], 1.0f, dh, ovec != 0);
    }
}

// ---- launchers (AttnCall: attention_common.h; the checks are the callers') -----------------------------------------------
// planes: 4 (the walked tile), or 8 where the owned rows live in LDS too
int tile_lds_bytes(int dh, int planes) { return planes * kTile * (((dh + 31) & ~31) + 8) * 2 + 256; }

// the instantiation of a kernel template for this head dim and dropout, with its dynamic LDS opted in on the call's device
#define DRIN_MFMA_PICK(KERNEL, wide, drop, lds, what, go)                                                     \
  do {                                                                                                         \
    static DynLdsOptIn opt_in[4];                                                                              \
    const int _i = ((wide) ? 2 : 0) + ((drop) ? 1 : 0);                                                        \
    const void* _k = _i == 0   ? reinterpret_cast<const void*>(KERNEL<128, false>)                             \
                     : _i == 1 ? reinterpret_cast<const void*>(KERNEL<128, true>)                              \
                     : _i == 2 ? reinterpret_cast<const void*>(KERNEL<256, false>)                             \
                               : reinterpret_cast<const void*>(KERNEL<256, true>);                             \
    DRIN_TRY(ensure_dynamic_lds(opt_in[_i], _k, (lds), "hipFuncSetAttribute(" what ")"));                      \
    DRIN_TRY(timed(DRIN_KC_ATTN, st, what, [&] {                                                               \
      _i == 0 ? go(KERNEL<128, false>) : _i == 1 ? go(KERNEL<128, true>) : _i == 2 ? go(KERNEL<256, false>) : go(KERNEL<256, true>); \
    }));                                                                                                       \
  } while (0)

bool rows16(const void* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }

}  // namespace

int launch_attention_mfma(const AttnCall& c, const DropArgs* drop, hipStream_t st) {
  const int dh = c.dh;
  const bool vec = dh % 4 == 0 && rows16(c.q, c.ldq) && rows16(c.k, c.ldk) && rows16(c.v, c.ldv);
  const bool ovec = dh % 4 == 0 && rows16(c.out, c.ldo);
  const float q_scale = kLog2e / sqrtf((float)dh);
  const dim3 grid((unsigned)cdiv(c.Lq, dh > 128 ? 32 : 64), (unsigned)c.H, (unsigned)c.B);   // Shape::OWN
  const int lds = tile_lds_bytes(dh, 4);
  const DropArgs da = drop ? *drop : DropArgs{};
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, c.q, c.ldq, c.k, c.ldk, c.v, c.ldv, c.mask, c.out, c.ldo, c.lse, c.Lq, c.Lk, dh,
                       q_scale, (int)vec, (int)ovec, da);
  };
  DRIN_MFMA_PICK(k_attention_mfma, dh > 128, drop != nullptr, lds, "k_attention_mfma", go);
  return DRIN_OK;
}

int launch_attention_mfma_bwd(const AttnCall& c, const DropArgs* drop, hipStream_t st) {
  const int dh = c.dh;
  const bool vec = dh % 4 == 0 && rows16(c.q, c.ldq) && rows16(c.k, c.ldk) && rows16(c.v, c.ldv) && rows16(c.dout, c.lddo);
  const float inv_sqrt = 1.0f / sqrtf((float)dh), q_scale = kLog2e * inv_sqrt;
  const bool wide = dh > 128;
  const int lds = tile_lds_bytes(dh, wide ? 8 : 4), own = wide ? 32 : 64;   // Shape::OWN_LDS, Shape::OWN
  const DropArgs da = drop ? *drop : DropArgs{};
  DRIN_TRY(launch_attention_bwd_delta(c, st));
  if (c.dq != nullptr) {
    const dim3 grid((unsigned)cdiv(c.Lq, own), (unsigned)c.H, (unsigned)c.B);
    const bool ovec = dh % 4 == 0 && rows16(c.dq, c.lddq);
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, c.q, c.ldq, c.k, c.ldk, c.v, c.ldv, c.mask, c.lse, c.dout, c.lddo, c.delta,
                         c.dq, c.lddq, c.Lq, c.Lk, dh, q_scale, inv_sqrt, (int)vec, (int)ovec, da);
    };
    DRIN_MFMA_PICK(k_attention_mfma_bwd_dq, wide, drop != nullptr, lds, "k_attention_mfma_bwd_dq", go);
  }
  if (c.dk == nullptr) return DRIN_OK;
  const dim3 grid((unsigned)cdiv(c.Lk, own), (unsigned)c.H, (unsigned)c.B);
  const bool ovec = dh % 4 == 0 && rows16(c.dk, c.lddk) && rows16(c.dv, c.lddv);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, c.q, c.ldq, c.k, c.ldk, c.v, c.ldv, c.mask, c.lse, c.dout, c.lddo, c.delta, c.dk,
                       c.lddk, c.dv, c.lddv, c.Lq, c.Lk, dh, q_scale, inv_sqrt, (int)vec, (int)ovec, da);
  };
  DRIN_MFMA_PICK(k_attention_mfma_bwd_dkv, wide, drop != nullptr, lds, "k_attention_mfma_bwd_dkv", go);
  return DRIN_OK;
}

}  // namespace drin
