// Linking against the whole entity table: the k best rows of a table [E, D] for every mention of a batch
// [B, D] by cosine, without a [B, E] score matrix.  The ordering contract is stated once in include/drin_hip.h ("cosine top-k")
// and followed by every kernel here through ONE comparison: an order key of the score (order_key: NaN lowest, then -inf ... +inf,
// -0.0 = +0.0) and, between equal keys, the lower row.
//   k_row_inv_norms   inv[e] = 1 / max(|rows[e]|, eps), one wave per row
//   k_topk_partial    (slice of kSlice columns, tile of kTile mentions): the kp best (key, column) of the slice per mention,
//                     kept by a threshold, an LDS candidate buffer and a bitonic sort in registers
//   k_topk_merge      per mention: the running list and the slice lists -> the new running list of kp (key, row), sorted
//   k_topk_finish     per mention: sort kp (score, row) by the contract, write the first k
//   k_pad_rows        x [B, D] -> [round4(B), D], zero rows behind
//   k_widen_rows      bf16 rows -> the same values as fp32 (a chunk of a bf16-stored table on the widen route)
//   k_rank_rows       per mention: the first k of n caller-given (score, row) pairs by the contract, with the input column of each
//                     (drin_rank_rows: the rerank behind a second-stage scoring)
//   k_object_rows     the image-image edge as a term (section 36): the score-weighted sum of one side's normalised object rows and the
//                     sum of its scores; k_topk_forms_combine: the combine of a call with a RATIO term; k_ratio_gather: its re-score
// and the entry points drin_row_inv_norms, drin_topk_update, drin_table_topk(_workspace_bytes), drin_rank_rows, with the _ex twins that
// read table rows STORED as bf16 in place (section 34: k_row_inv_norms<__bf16>, the product routed by the GEMM module, the re-score
// k_cosine_gather<__bf16>).  A storage-templated kernel has ONE launcher that takes the row dtype.  The workspace of drin_table_topk
// and of drin_table_topk_sum is one description (topk_layout.h: TopkLayout; the single-table form is the summed one at S = 1
// without the factors and the cosines), and the size query and the run of either form go through one plan_topk (section 35).
// The block of dot products is
// ENTITY-major, as the product y[Ec, Bp] = rows_chunk x^T leaves it: element (mention b, column c) at block[c * ld + b].
// No atomics, no scratch memory; a workgroup of the three selection kernels is ONE wave, so its barriers order that wave's LDS
// traffic and wait for nobody.
#include "device_utils.h"
#include "row_checks.h"
#include "topk_layout.h"

namespace drin {
namespace {

constexpr int kSlice = kTopkSlice;        // columns per partial workgroup
constexpr int kTile = 8;                  // mentions per partial workgroup: 32 contiguous bytes of every block row
constexpr int kMaxKp = kTopkMaxKp;
constexpr int kStageLd = 65;              // floats per staged mention row (64 columns + 1: the transposing writes spread over banks)

static_assert(DRIN_TOPK_KP(1) == 64 && DRIN_TOPK_KP(65) == 128 && DRIN_TOPK_KP(256) == kMaxKp, "kp: the power of two >= max(k, 64)");

constexpr int64_t kNoRow = INT64_MAX;     // the row of an empty list entry inside the kernels (-1 in the state buffers)

// Order key of a score: a > b as unsigned iff score a ranks before score b.  0 is kept for "empty", NaN is 1, -inf 0x007FFFFF.
__device__ __forceinline__ uint32_t order_key(float v) {
  if (v != v) return 1u;
  const uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_of_order(uint32_t k) {
  if (k <= 1u) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ bool ranks_before(uint32_t ka, int64_t ra, uint32_t kb, int64_t rb) { return ka > kb || (ka == kb && ra < rb); }

__device__ __forceinline__ int lanes_below(uint64_t mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return (uint64_t)hi << 32 | lo;
}

// One wave per row, four rows per workgroup, the rest by grid stride: k_cosine_gather's lane loop and wave sum of its yy.
// RowT: float, or __bf16 for rows stored as bf16 (widened exactly by ld4: the bits of the float instantiation on the widened rows).
template <typename RowT>
__global__ void __launch_bounds__(256) k_row_inv_norms(const RowT* __restrict__ rows, int64_t num_rows, int D4, float eps,
                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < num_rows; e += (int64_t)gridDim.x * 4) {
    const RowT* yr = rows + e * (int64_t)D4 * 4;
    float yy = 0.f;
    for (int c4 = lane; c4 < D4; c4 += 64) {
      const float4 b = ld4(yr + c4 * 4);
      yy += dot4(b, b);
    }
    yy = wave_sum(yy);
    if (lane == 0) out[e] = 1.0f / fmaxf(sqrtf(yy), eps);
  }
}

// out [n4 quads] = the bf16 values of in, widened exactly (a 16-bit shift): the chunk of a bf16-stored table that a product outside
// the plane kernel's contract reads as fp32 (the widen route of launch_gemm_nt).  8 bytes in, 16 out per lane.
__global__ void __launch_bounds__(256) k_widen_rows(const __bf16* __restrict__ in, float* __restrict__ out, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) st4(out + i * 4, ld4(in + i * 4));
}

__global__ void __launch_bounds__(256) k_pad_rows(const float* __restrict__ x, float* __restrict__ out, int64_t n4_in, int64_t n4_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4_out; i += (int64_t)gridDim.x * 256)
    st4(out + i * 4, i < n4_in ? ld4(x + i * 4) : make_float4(0.f, 0.f, 0.f, 0.f));
}

// ---- the summed-cosine form ----------------------------------------------------------------------
// The S blocks of dot products of one chunk -> ONE block of scores: out[c * ld + b] = sum_s block_s[c * ld + b] * inv_s[c] *
// (scale_s[b] * weight_s), in term order, every multiply and add rounded to fp32 on its own (no contraction: the sum can be
// restated bit for bit).  A pure stream over S blocks in and one block out: a thread keeps ONE quad of mentions - its S float4 of
// per-mention factors are read once - and walks rows of the block, 16 bytes per lane per block; a workgroup is 2^tx_log2 quads
// wide and 256 >> tx_log2 rows tall, so that a wave's lanes cover whole rows of a narrow block (rows are contiguous when
// ld = Bp).  out may alias block 0: a thread reads its own 16 bytes of every block before it writes them.
struct CombineTerms {
  const float* block[DRIN_TOPK_MAX_TERMS];
  const float* inv[DRIN_TOPK_MAX_TERMS];     // [cols], already moved to the chunk's first row
  const float* scale[DRIN_TOPK_MAX_TERMS];   // [ld]
  float weight[DRIN_TOPK_MAX_TERMS];
};
// (hipcc contracts a * b + c by default, and HIP's __fmul_rn / __fadd_rn are inline functions around the plain operators,
//  compiled under that default: a multiply and an add made of them still fuse.  The operators under this pragma do not -
//  tests/test_table_topk_sum_host.py reads the ISA for an fma.  The pragma holds under hipcc's default -ffp-contract=fast-honor-pragmas:
//  the build must not pass -ffp-contract=fast, which ignores it)
__device__ __forceinline__ float4 mul4_rn(float4 a, float4 b) {
#pragma clang fp contract(off)
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float4 mul4_rn(float4 a, float s) { return mul4_rn(a, make_float4(s, s, s, s)); }
__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
#pragma clang fp contract(off)
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
template <int S>
__global__ void __launch_bounds__(256) k_topk_combine(CombineTerms t, float* out, int64_t ld, int64_t cols, int tx_log2) {
  const int64_t q4 = ((int64_t)blockIdx.x << tx_log2 | (threadIdx.x & ((1 << tx_log2) - 1))) * 4;   // first mention of the quad
  if (q4 >= ld) return;                                   // no barrier below
  const int ty = threadIdx.x >> tx_log2, rows_tall = 256 >> tx_log2;
  float4 f[S];
#pragma unroll
  for (int s = 0; s < S; ++s) f[s] = mul4_rn(ld4(t.scale[s] + q4), t.weight[s]);
  for (int64_t c = (int64_t)blockIdx.y * rows_tall + ty; c < cols; c += (int64_t)gridDim.y * rows_tall) {
    float4 v[S];
#pragma unroll
    for (int s = 0; s < S; ++s) v[s] = ld4(t.block[s] + c * ld + q4);
    float4 acc = mul4_rn(mul4_rn(v[0], t.inv[0][c]), f[0]);
#pragma unroll
    for (int s = 1; s < S; ++s) acc = add4_rn(acc, mul4_rn(mul4_rn(v[s], t.inv[s][c]), f[s]));
    st4(out + c * ld + q4, acc);
  }
}

// out[i] = w_0 c_0[i], then + w_s c_s[i] for s = 1 ..: the fp32 chain over the S re-scored cosines cos [S][n], every multiply
// and add rounded on its own; n % 4 == 0.
struct ChainWeights {
  float w[DRIN_TOPK_MAX_TERMS];
};
__global__ void __launch_bounds__(256) k_weighted_cosine_sum(const float* __restrict__ cos, int S, int64_t n4, ChainWeights cw,
                                                             float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 acc = mul4_rn(ld4(cos + i * 4), cw.w[0]);
#pragma unroll
    for (int s = 1; s < DRIN_TOPK_MAX_TERMS; ++s)          // constant indices into the argument struct
      if (s < S) acc = add4_rn(acc, mul4_rn(ld4(cos + ((int64_t)s * n4 + i) * 4), cw.w[s]));
    st4(out + i * 4, acc);
  }
}

// ---- the RATIO form: the image-image edge as a term -----------------------------------------------------
// out[r, :] = sum_j score[r, j] obj[r, j, :] / max(|obj[r, j, :]|, eps), mass[r] = sum_j score[r, j]: the side of model.py:84-92
// that belongs to one mention (K = Km) or one entity (K = Ke).  One wave per output row, four per workgroup, the rest by grid
// stride; lanes take column quads lane, lane + 64, ... as k_row_inv_norms does.  REG (R4 <= 512): an object row is read ONCE into
// eight float4 slots per lane (k_miei_lds keeps its row the same way) and stays there between its norm and its scaled
// accumulation.  Past that the wave takes the K scales first (lane j keeps scale j) and reads every row a second time.  Either way:
// yy in the lane order of k_row_inv_norms, one division per object row, fp32 FMAs and the score sum in ascending j.
// T: float, or __bf16 for objects and scores stored as bf16 (widened exactly: the bits of the float instantiation on the widened values).
constexpr int kObjectMaxK = 16;
template <typename T, bool REG>
__global__ void __launch_bounds__(256) k_object_rows(const T* __restrict__ obj, const T* __restrict__ score, int64_t n, int K, int R4,
                                                     float eps, float* __restrict__ out, float* __restrict__ mass) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
    const T* rows = obj + r * K * (int64_t)R4 * 4;
    const T* sc = score + r * K;
    float* dst = out + r * (int64_t)R4 * 4;
    float m = 0.f;
    if (REG) {
      float4 acc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int j = 0; j < K; ++j) {
        const T* yr = rows + j * (int64_t)R4 * 4;
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c4 = lane + 64 * k;
          v[k] = c4 < R4 ? ld4_stream(yr + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);   // read once
        }
        float yy = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) yy += dot4(v[k], v[k]);   // (an empty slot adds +0: the lane loop's sum)
        yy = wave_sum(yy);
        const float w = (float)sc[j];
        const float s = w / fmaxf(sqrtf(yy), eps);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = fma4(s, v[k], acc[k]);
        m += w;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c4 = lane + 64 * k;
        if (c4 < R4) st4(dst + c4 * 4, acc[k]);
      }
    } else {
      float mine = 0.f;                                      // lane j keeps the scale of object row j (K <= 16 < 64)
      for (int j = 0; j < K; ++j) {
        const T* yr = rows + j * (int64_t)R4 * 4;
        float yy = 0.f;
        for (int c4 = lane; c4 < R4; c4 += 64) {
          const float4 b = ld4(yr + c4 * 4);
          yy += dot4(b, b);
        }
        yy = wave_sum(yy);
        const float w = (float)sc[j];
        const float s = w / fmaxf(sqrtf(yy), eps);
        if (lane == j) mine = s;
        m += w;
      }
      for (int c0 = 0; c0 < R4; c0 += 64) {                  // wave-uniform trips: the scales are read across lanes
        const int c4 = c0 + lane;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < K; ++j) {
          const float s = __shfl(mine, j);
          if (c4 < R4) acc = fma4(s, ld4(rows + (j * (int64_t)R4 + c4) * 4), acc);
        }
        if (c4 < R4) st4(dst + c4 * 4, acc);
      }
    }
    if (lane == 0) mass[r] = m;
  }
}

// x_mass [B] -> [Bp], zeros behind: the per-mention factor region of a RATIO term
__global__ void __launch_bounds__(256) k_pad_mass(const float* __restrict__ x, float* __restrict__ out, int B, int Bp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < Bp) out[i] = i < B ? x[i] : 0.f;
}

// The combine with a form per term (bit s of ratio_mask: term s is a RATIO): a COSINE term is k_topk_combine's step, with its
// sequence and bits; a RATIO term reads the masses where the other reads inverse norms and factors - t.inv[s] = row_mass at the
// chunk's first row, t.scale[s] = x_mass padded to ld - and is d = row_mass[c] x_mass[b]; d = d + eps; t = block / d; t = t w,
// each rounded to fp32 on its own, the divide correctly rounded.  The mask is uniform over the launch: scalar branches.
struct FormTerms {
  CombineTerms t;
  float eps[DRIN_TOPK_MAX_TERMS];
  uint32_t ratio_mask;
};
__device__ __forceinline__ float4 div4_rn(float4 a, float4 b) {
#pragma clang fp contract(off)
  return make_float4(a.x / b.x, a.y / b.y, a.z / b.z, a.w / b.w);
}
template <int S>
__global__ void __launch_bounds__(256) k_topk_forms_combine(FormTerms ft, float* out, int64_t ld, int64_t cols, int tx_log2) {
  const CombineTerms& t = ft.t;
  const int64_t q4 = ((int64_t)blockIdx.x << tx_log2 | (threadIdx.x & ((1 << tx_log2) - 1))) * 4;   // first mention of the quad
  if (q4 >= ld) return;                                   // no barrier below
  const int ty = threadIdx.x >> tx_log2, rows_tall = 256 >> tx_log2;
  float4 f[S];                                            // COSINE: scale x weight; RATIO: the mentions' masses
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const float4 g = ld4(t.scale[s] + q4);
    f[s] = (ft.ratio_mask >> s & 1u) ? g : mul4_rn(g, t.weight[s]);
  }
  for (int64_t c = (int64_t)blockIdx.y * rows_tall + ty; c < cols; c += (int64_t)gridDim.y * rows_tall) {
    float4 v[S];
#pragma unroll
    for (int s = 0; s < S; ++s) v[s] = ld4(t.block[s] + c * ld + q4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      float4 term;
      if (ft.ratio_mask >> s & 1u) {
        const float e = ft.eps[s];
        const float4 d = add4_rn(mul4_rn(f[s], t.inv[s][c]), make_float4(e, e, e, e));
        term = mul4_rn(div4_rn(v[s], d), t.weight[s]);
      } else {
        term = mul4_rn(mul4_rn(v[s], t.inv[s][c]), f[s]);
      }
      acc = s == 0 ? term : add4_rn(acc, term);
    }
    st4(out + c * ld + q4, acc);
  }
}

// out[b, n] = (x[b] . rows[index[b, n]]) / (x_mass[b] row_mass[index[b, n]] + eps): k_cosine_gather's wave per pair, lane loop, dot4 and
// wave_sum of xy on a clamped row, then the ratio - product, sum and divide rounded one by one (the combine's sequence).
__global__ void __launch_bounds__(256) k_ratio_gather(const float* __restrict__ x, const float* __restrict__ x_mass,
                                                      const float* __restrict__ rows, const float* __restrict__ row_mass,
                                                      const int64_t* __restrict__ index, int64_t num_rows, float* __restrict__ out,
                                                      int64_t pairs, int N, int D4, float eps, int32_t* status, int64_t pair_base) {
  int64_t p, b;
  if (!wave_pair(pairs, N, p, b)) return;
  const int lane = threadIdx.x & 63;
  const int64_t raw = index[p];
  const int64_t e = raw < 0 ? 0 : (raw >= num_rows ? num_rows - 1 : raw);
  if (e != raw && lane == 0) report_bad_index(status, pair_base + p, raw);
  const float* xr = x + b * (int64_t)D4 * 4;
  const float* yr = rows + e * (int64_t)D4 * 4;
  float xy = 0.f;
  for (int c4 = lane; c4 < D4; c4 += 64) xy += dot4(ld4(xr + c4 * 4), ld4(yr + c4 * 4));
  xy = wave_sum(xy);
  if (lane == 0) {
#pragma clang fp contract(off)
    float d = x_mass[b] * row_mass[e];
    d = d + eps;
    out[p] = xy / d;
  }
}

// Descending bitonic sort of 64 R composites held R per lane (element r * 64 + lane), in registers: a stride below 64 exchanges
// lanes (__shfl_xor: no LDS traffic, no barrier), a stride from 64 up exchanges two of the lane's own registers.
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
  return (uint64_t)hi << 32 | lo;
}
// one pass at a stride below 64: element r * 64 + lane meets lane ^ j's
template <int R>
__device__ __forceinline__ void lane_stage(uint64_t (&v)[R], int lane, int k2, int j) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t other = shfl_xor64(v[r], j);
    const bool want_max = ((((r << 6) | lane) & k2) == 0) == ((lane & j) == 0);
    v[r] = (want_max == (other > v[r])) ? other : v[r];
  }
}
template <int R>
__device__ __forceinline__ void sort_desc_regs(uint64_t (&v)[R], int lane) {
  // runs of up to 64: lane passes only, the pass loops stay rolled (the stride is a run-time operand of the exchange)
#pragma unroll 1
  for (int k2 = 2; k2 <= 64; k2 <<= 1)
#pragma unroll 1
    for (int j = k2 >> 1; j > 0; j >>= 1) lane_stage<R>(v, lane, k2, j);
  // runs of 128 and up: the strides from 64 up pair REGISTERS, so these few levels unroll and v[] is indexed by constants only
#pragma unroll
  for (int k2 = 128; k2 <= 64 * R; k2 <<= 1) {
#pragma unroll
    for (int j = k2 >> 1; j >= 64; j >>= 1) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if ((r & (j >> 6)) != 0) continue;
        const uint64_t a = v[r], b = v[r | (j >> 6)];
        const bool swap = (((r << 6) & k2) == 0) ? a < b : a > b;   // k2 >= 128: the direction is the register's
        v[r] = swap ? b : a, v[r | (j >> 6)] = swap ? a : b;
      }
    }
#pragma unroll 1
    for (int j = 32; j > 0; j >>= 1) lane_stage<R>(v, lane, k2, j);
  }
}

// The KP best columns of one slice for each mention of one tile.  A candidate is ONE 64-bit composite, order key above, 2^32 - 1 -
// column below: composites of a slice are distinct and a larger one ranks first, so the order inside a slice is the contract's.
// Per mention: a threshold (0, or - from the second call on - just under the running list's last key: what ranks after KP known
// rows cannot enter), a buffer of 2 KP composites that takes what beats the threshold (ballot + lane count: the columns' order,
// no atomics), and - when the next 64 may not fit, and after the slice's last step - a sort that keeps the KP best and raises the
// threshold to the KP-th.  Lane m keeps count and threshold of mention m.  slices [gridDim.x][batch][KP], sorted, 0 = empty.
template <int KP>
__global__ void __launch_bounds__(64) k_topk_partial(const float* __restrict__ block, int64_t ld, int batch, int64_t cols,
                                                     const float* __restrict__ inv, const float* __restrict__ run_keys,
                                                     const int64_t* __restrict__ run_rows, uint64_t* __restrict__ slices) {
  constexpr int cap = 2 * KP, R = cap / 64;
  __shared__ uint64_t buf[kTile * cap];
  __shared__ float stage[kTile * kStageLd];
  const int lane = threadIdx.x;
  const int64_t c_begin = (int64_t)blockIdx.x * kSlice, c_end = cols < c_begin + kSlice ? cols : c_begin + kSlice;
  const int b0 = (int)blockIdx.y * kTile, nm = batch - b0 < kTile ? batch - b0 : kTile;
  int cnt = 0;
  uint64_t thr = 0;
  if (run_rows != nullptr && lane < nm) {
    const int64_t last = ((int64_t)(b0 + lane) + 1) * KP - 1;
    if (run_rows[last] >= 0) thr = ((uint64_t)order_key(run_keys[last]) << 32) - 1;   // keys >= the list's last one pass
  }
  for (int64_t c0 = c_begin; c0 < c_end; c0 += 64) {
    const bool last_step = c0 + 64 >= c_end;
    // 64 columns x kTile mentions: two 16-byte loads per lane, transposed into the stage
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int col = (lane >> 1) + 32 * i, b = b0 + 4 * (lane & 1);
      const int64_t c = c0 + col;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < c_end && b < ld) v = ld4(block + c * ld + b);   // ld % 4 == 0: the four floats lie inside row c
      float* s = stage + 4 * (lane & 1) * kStageLd + col;
      s[0] = v.x, s[kStageLd] = v.y, s[2 * kStageLd] = v.z, s[3 * kStageLd] = v.w;
    }
    const int64_t cl = c0 + lane;
    const bool valid = cl < c_end;
    const float scale = (inv != nullptr && valid) ? inv[cl] : 1.0f;
    __syncthreads();
    for (int m = 0; m < nm; ++m) {
      const float key = stage[m * kStageLd + lane] * scale;
      const uint64_t comp = valid ? ((uint64_t)order_key(key) << 32 | (uint64_t)(0xFFFFFFFFu - (uint32_t)cl)) : 0;
      int n = __shfl(cnt, m);
      uint64_t t = shfl64(thr, m);
      const bool pass = comp > t;
      const uint64_t mask = __ballot(pass);
      uint64_t* mine = buf + m * cap;
      if (pass) mine[n + lanes_below(mask)] = comp;           // n <= cap - 64 here
      n += __popcll(mask);
      if (n > cap - 64 || last_step) {                         // wave-uniform
        __syncthreads();                                       // the appends of other lanes
        uint64_t v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = r * 64 + lane < n ? mine[r * 64 + lane] : 0;
        sort_desc_regs<R>(v, lane);
        if (n >= KP) n = KP, t = shfl64(v[R / 2 - 1], 63);     // element KP - 1
        if (last_step) {
          uint64_t* out = slices + ((int64_t)blockIdx.x * batch + b0 + m) * KP;
#pragma unroll
          for (int r = 0; r < R / 2; ++r) out[r * 64 + lane] = v[r];
        } else {
#pragma unroll
          for (int r = 0; r < R / 2; ++r) mine[r * 64 + lane] = v[r];   // each lane rewrites elements it alone read
        }
      }
      if (lane == m) cnt = n, thr = t;
    }
    __syncthreads();
  }
}

// One mention: fold the slice lists of this call into the running list.  Both are sorted, so a step is a bitonic MERGE (the
// slice list read backwards behind the running one) of 2 kp entries, log2(2 kp) passes; a slice list whose best entry ranks
// after the running list's last is skipped.  Entries here are (order key, table row): rows need 64 bits.
__global__ void __launch_bounds__(64) k_topk_merge(const uint64_t* __restrict__ slices, int num_slices, int batch, int kp,
                                                   int64_t col_base, float* __restrict__ run_keys, int64_t* __restrict__ run_rows,
                                                   int first) {
  __shared__ uint32_t sk[2 * kMaxKp];
  __shared__ int64_t sr[2 * kMaxKp];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  for (int i = lane; i < kp; i += 64) {
    const int64_t r = first ? -1 : run_rows[b * kp + i];
    sk[i] = r < 0 ? 0u : order_key(run_keys[b * kp + i]);
    sr[i] = r < 0 ? kNoRow : r;
  }
  __syncthreads();
  for (int s = 0; s < num_slices; ++s) {
    const uint64_t* list = slices + ((int64_t)s * batch + b) * kp;
    const uint64_t best = list[0];
    if (best == 0) continue;
    if (!ranks_before((uint32_t)(best >> 32), col_base + (int64_t)(0xFFFFFFFFu - (uint32_t)best), sk[kp - 1], sr[kp - 1])) continue;
    for (int i = lane; i < kp; i += 64) {
      const uint64_t c = list[kp - 1 - i];
      sk[kp + i] = (uint32_t)(c >> 32);
      sr[kp + i] = c == 0 ? kNoRow : col_base + (int64_t)(0xFFFFFFFFu - (uint32_t)c);
    }
    __syncthreads();
    for (int j = kp; j > 0; j >>= 1) {
      for (int t = lane; t < kp; t += 64) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const uint32_t ki = sk[i], kq = sk[p];
        const int64_t ri = sr[i], rq = sr[p];
        if (ranks_before(kq, rq, ki, ri)) sk[i] = kq, sr[i] = rq, sk[p] = ki, sr[p] = ri;
      }
      __syncthreads();
    }
  }
  for (int i = lane; i < kp; i += 64) {
    run_keys[b * kp + i] = key_of_order(sk[i]);
    run_rows[b * kp + i] = sk[i] == 0 ? -1 : sr[i];
  }
}

// One mention: kp (score, row) pairs (row < 0: empty, ranks last) sorted by the contract; the first k are written, the scores
// with the bits they came with.
__global__ void __launch_bounds__(64) k_topk_finish(const float* __restrict__ keys, const int64_t* __restrict__ rows, int kp, int k,
                                                    float* __restrict__ out_keys, int64_t* __restrict__ out_rows) {
  __shared__ uint32_t sk[kMaxKp];
  __shared__ int64_t sr[kMaxKp];
  __shared__ float sf[kMaxKp];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  for (int i = lane; i < kp; i += 64) {
    const int64_t r = rows[b * kp + i];
    const float f = keys[b * kp + i];
    sk[i] = r < 0 ? 0u : order_key(f);
    sr[i] = r < 0 ? kNoRow : r;
    sf[i] = f;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= kp; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (kp >> 1); t += 64) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const uint32_t ki = sk[i], kq = sk[p];
        const int64_t ri = sr[i], rq = sr[p];
        const bool swap = ((i & k2) == 0) ? ranks_before(kq, rq, ki, ri) : ranks_before(ki, ri, kq, rq);
        if (swap) {
          const float fi = sf[i], fq = sf[p];
          sk[i] = kq, sr[i] = rq, sf[i] = fq, sk[p] = ki, sr[p] = ri, sf[p] = fi;
        }
      }
      __syncthreads();
    }
  for (int i = lane; i < k; i += 64) {
    out_keys[b * k + i] = sk[i] == 0 ? __uint_as_float(0x7FC00000u) : sf[i];
    out_rows[b * k + i] = sk[i] == 0 ? -1 : sr[i];
  }
}

// One mention: n (score, row) pairs of a caller's list - a row may be named twice - sorted by the contract with one more rule,
// between equal scores on equal rows the lower input column (slot) first, so the order is total on any input.  A bitonic sort
// over P = the power of two >= n entries of (order key, slot, row) in LDS; the P - n padding entries carry key 0 - below every
// score's key - and rank last.  The first k are written: scores canonical (key_of_order), rows, and the slots when asked for.
constexpr int kMaxRankRows = 4096;   // 16 bytes per entry: 64 KB of LDS at most
__device__ __forceinline__ bool ranks_before3(uint32_t ka, int64_t ra, uint32_t sa, uint32_t kb, int64_t rb, uint32_t sb) {
  return ka > kb || (ka == kb && (ra < rb || (ra == rb && sa < sb)));
}
__global__ void __launch_bounds__(256) k_rank_rows(const float* __restrict__ scores, const int64_t* __restrict__ rows, int n, int P, int k,
                                                   float* __restrict__ out_scores, int64_t* __restrict__ out_rows,
                                                   int32_t* __restrict__ out_slots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rank_lds[];
  int64_t* sr = reinterpret_cast<int64_t*>(rank_lds);          // [P]
  uint32_t* sk = reinterpret_cast<uint32_t*>(sr + P);          // [P]
  uint32_t* ss = sk + P;                                       // [P]
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  for (int i = tid; i < P; i += 256) {
    const bool real = i < n;
    sk[i] = real ? order_key(scores[b * n + i]) : 0u;
    sr[i] = real ? rows[b * n + i] : kNoRow;
    ss[i] = (uint32_t)i;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const uint32_t ki = sk[i], kq = sk[p], si = ss[i], sq = ss[p];
        const int64_t ri = sr[i], rq = sr[p];
        const bool swap = ((i & k2) == 0) ? ranks_before3(kq, rq, sq, ki, ri, si) : ranks_before3(ki, ri, si, kq, rq, sq);
        if (swap) sk[i] = kq, sr[i] = rq, ss[i] = sq, sk[p] = ki, sr[p] = ri, ss[p] = si;
      }
      __syncthreads();
    }
  for (int i = tid; i < k; i += 256) {   // k <= n: never a padding entry
    out_scores[b * k + i] = key_of_order(sk[i]);
    out_rows[b * k + i] = sr[i];
    if (out_slots != nullptr) out_slots[b * k + i] = (int32_t)ss[i];
  }
}

size_t topk_scratch_bytes(int64_t batch, int64_t cols, int kp) { return (size_t)cdiv(cols, kSlice) * (size_t)batch * kp * sizeof(uint64_t); }
int64_t slices_of(int64_t cols) { return cdiv(cols, kSlice); }

// the selection of one block: partial lists per slice, then the merge into the running list
int launch_topk_update(const float* block, int64_t ld, int batch, int64_t cols, int64_t col_base, const float* inv, int kp,
                       float* keys, int64_t* rows, uint64_t* slices, bool first, hipStream_t st) {
  const int64_t ns = slices_of(cols);
  auto partial = kp == 64 ? k_topk_partial<64> : (kp == 128 ? k_topk_partial<128> : k_topk_partial<256>);
  DRIN_TRY(timed(DRIN_KC_EDGE, st, "k_topk_partial", [&] {
    hipLaunchKernelGGL(partial, dim3((unsigned)ns, (unsigned)cdiv(batch, kTile)), dim3(64), 0, st, block, ld, batch, cols, inv,
                       first ? nullptr : keys, first ? nullptr : rows, slices);
  }));
  return timed(DRIN_KC_EDGE, st, "k_topk_merge", [&] {
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)batch), dim3(64), 0, st, slices, (int)ns, batch, kp, col_base, keys, rows, first ? 1 : 0);
  });
}

int launch_topk_finish(const float* keys, const int64_t* rows, int batch, int kp, int k, float* out_keys, int64_t* out_rows, hipStream_t st) {
  return timed(DRIN_KC_EDGE, st, "k_topk_finish", [&] {
    hipLaunchKernelGGL(k_topk_finish, dim3((unsigned)batch), dim3(64), 0, st, keys, rows, kp, k, out_keys, out_rows);
  });
}

int launch_rank_rows(const float* scores, const int64_t* rows, int batch, int n, int k, float* out_scores, int64_t* out_rows,
                     int32_t* out_slots, hipStream_t st) {
  int P = 1;
  while (P < n) P <<= 1;
  const int lds = P * 16;
  static DynLdsOptIn opt_in;
  DRIN_TRY(ensure_dynamic_lds(opt_in, reinterpret_cast<const void*>(k_rank_rows), kMaxRankRows * 16, "hipFuncSetAttribute(rank_rows)"));
  return timed(DRIN_KC_EDGE, st, "k_rank_rows", [&] {
    hipLaunchKernelGGL(k_rank_rows, dim3((unsigned)batch), dim3(256), lds, st, scores, rows, n, P, k, out_scores, out_rows, out_slots);
  });
}

// row_dtype: how the rows are stored (DRIN_FEAT_F32 / DRIN_FEAT_BF16) - the instantiation and the timer's name
int launch_row_inv_norms(const void* rows, int row_dtype, int64_t num_rows, int width, float eps, float* out, hipStream_t st) {
  const int64_t blocks = row_blocks(num_rows);
  if (row_dtype != DRIN_FEAT_BF16)
    return timed(DRIN_KC_EDGE, st, "k_row_inv_norms", [&] {
      hipLaunchKernelGGL(k_row_inv_norms<float>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const float*>(rows), num_rows, width / 4,
                         eps, out);
    });
  return timed(DRIN_KC_EDGE, st, "k_row_inv_norms_bf16", [&] {
    hipLaunchKernelGGL(k_row_inv_norms<__bf16>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const __bf16*>(rows), num_rows, width / 4,
                       eps, out);
  });
}
// x [B, D] -> xpad [Bp, D], zero rows behind
int launch_pad_rows(const float* x, float* xpad, int B, int Bp, int D, hipStream_t st) {
  const int64_t n4_in = (int64_t)B * D / 4, n4_out = (int64_t)Bp * D / 4;
  return timed(DRIN_KC_EDGE, st, "k_pad_rows", [&] {
    hipLaunchKernelGGL(k_pad_rows, dim3((unsigned)(cdiv(n4_out, 256) < 4096 ? cdiv(n4_out, 256) : 4096)), dim3(256), 0, st, x, xpad, n4_in, n4_out);
  });
}
// the product block[n, Bp] = rows_chunk xpad^T of one chunk: fp32 rows as ever; bf16-stored rows declared as such, with the planes of
// xpad and the widen region the layout carved - the GEMM module picks the route (gemm.h: NtProduct::x_bf16)
int launch_chunk_product(const void* rows, int row_dtype, int64_t e0, int64_t n, int D, const float* xpad, const float* planes, float* widen,
                         size_t widen_floats, float* block, int Bp, int precision, hipStream_t st) {
  if (row_dtype != DRIN_FEAT_BF16)
    return launch_gemm_nt({{static_cast<const float*>(rows) + e0 * D, D}, {xpad, D}, nullptr, block, Bp, n, Bp, D}, precision, st);
  NtProduct p{{nullptr, D}, {xpad, D}, nullptr, block, Bp, n, Bp, D};
  p.x_bf16 = static_cast<const uint16_t*>(rows) + e0 * D;
  p.x_widen = scratch_at(widen, 0, widen_floats);
  return launch_gemm_nt(p.with_planes(planes), precision, st);
}

int check_topk_shape(const char* who, int64_t E, int batch, int width, int k) {
  DRIN_TRY(check_count(who, "num_entities", E, 1, INT64_MAX / 4096));
  DRIN_TRY(check_count(who, "batch", batch, 1, kMaxGridY));
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "k", k, 1, kMaxKp));
  if (k > E) {
    set_error("%s: k = %lld exceeds num_entities = %lld", who, (long long)k, (long long)E);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

int check_precision_topk(const char* who, int precision) {
  if (precision != DRIN_PREC_F32 && precision != DRIN_PREC_BF16X3) {
    set_error("%s: precision %d is not DRIN_PREC_F32 / DRIN_PREC_BF16X3", who, precision);
    return DRIN_E_UNSUPPORTED;
  }
  return DRIN_OK;
}

// The plan of one call of either form (topk_layout.h: TopkLayout): the checks that the size query and the run share - shape, how the
// rows are stored, precision, chunk - then the layout, and for a run (`have` not NULL) that the caller's workspace holds it.  A
// query maps any failure to 0 bytes; drin_last_error names `who`, the spelling that was called.
int plan_topk(const char* who, const int* widths, const int* dtypes, int S, bool summed, int batch, int64_t E, int k, int64_t chunk_entities,
              int precision, const size_t* have, TopkLayout* W) {
  DRIN_TRY(check_topk_shape(who, E, batch, widths[0], k));
  for (int s = 0; s < S; ++s) DRIN_TRY(check_row_dtype(who, dtypes[s], widths[s]));
  DRIN_TRY(check_precision_topk(who, precision));
  if (chunk_entities < 0) {
    set_error("%s: chunk_entities = %lld is negative", who, (long long)chunk_entities);
    return DRIN_E_SHAPE;
  }
  if (!W->build(widths, dtypes, S, summed, batch, E, k, chunk_entities, precision)) {
    set_error("%s: chunk_entities = %lld is out of range (at most 2^30 rows, the workspace must fit in size_t)", who,
              (long long)chunk_entities);
    return DRIN_E_SHAPE;
  }
  if (have != nullptr && *have < W->total_floats * sizeof(float)) {
    set_error("%s: workspace %zu bytes < %zu", who, *have, W->total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  return DRIN_OK;
}

// ---- the summed-cosine form: launchers, the live terms of a call --------------------------------------------------------------
int launch_topk_combine(const CombineTerms& t, int S, float* out, int64_t ld, int64_t cols, hipStream_t st) {
  const int64_t quads = ld / 4;
  int tx_log2 = 0;
  while (tx_log2 < 8 && ((int64_t)1 << tx_log2) < quads) ++tx_log2;
  const int64_t rows_tall = 256 >> tx_log2;
  const int64_t gx = cdiv(quads, (int64_t)1 << tx_log2);          // ld <= 2^31 - 1: at most 2^21
  int64_t gy = cdiv(cols, rows_tall * 8);                         // eight rows per thread; past the cap a thread walks more
  gy = gy < 1 ? 1 : (gy > kMaxGridY ? kMaxGridY : gy);
  auto kernel = S == 1 ? k_topk_combine<1> : S == 2 ? k_topk_combine<2> : S == 3 ? k_topk_combine<3> : k_topk_combine<4>;
  return timed(DRIN_KC_EDGE, st, "k_topk_combine", [&] {
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, t, out, ld, cols, tx_log2);
  });
}

int launch_weighted_cosine_sum(const float* cos, int S, int64_t n, const ChainWeights& cw, float* out, hipStream_t st) {
  const int64_t n4 = n / 4, blocks = cdiv(n4, 256) < 4096 ? cdiv(n4, 256) : 4096;
  return timed(DRIN_KC_EDGE, st, "k_weighted_cosine_sum", [&] {
    hipLaunchKernelGGL(k_weighted_cosine_sum, dim3((unsigned)blocks), dim3(256), 0, st, cos, S, n4, cw, out);
  });
}

// ---- the RATIO form: launchers ------------------------------------------------------------------------------------------------
// the combine of a call with at least one RATIO term (none: launch_topk_combine, the old launch); the grid is launch_topk_combine's
int launch_topk_forms_combine(const FormTerms& ft, int S, float* out, int64_t ld, int64_t cols, hipStream_t st) {
  const int64_t quads = ld / 4;
  int tx_log2 = 0;
  while (tx_log2 < 8 && ((int64_t)1 << tx_log2) < quads) ++tx_log2;
  const int64_t rows_tall = 256 >> tx_log2;
  const int64_t gx = cdiv(quads, (int64_t)1 << tx_log2);
  int64_t gy = cdiv(cols, rows_tall * 8);
  gy = gy < 1 ? 1 : (gy > kMaxGridY ? kMaxGridY : gy);
  auto kernel = S == 1 ? k_topk_forms_combine<1> : S == 2 ? k_topk_forms_combine<2> : S == 3 ? k_topk_forms_combine<3> : k_topk_forms_combine<4>;
  return timed(DRIN_KC_EDGE, st, "k_topk_forms_combine", [&] {
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, ft, out, ld, cols, tx_log2);
  });
}

int launch_pad_mass(const float* x_mass, float* out, int B, int Bp, hipStream_t st) {
  return timed(DRIN_KC_EDGE, st, "k_pad_mass", [&] {
    hipLaunchKernelGGL(k_pad_mass, dim3((unsigned)cdiv(Bp, 256)), dim3(256), 0, st, x_mass, out, B, Bp);
  });
}

int launch_ratio_gather(const float* x, const float* x_mass, const float* rows, const float* row_mass, const int64_t* index, int64_t num_rows,
                        float* out, int B, int N, int D, float eps, int32_t* status, hipStream_t st) {
  const int64_t pairs = (int64_t)B * N;
  if (pairs <= 0) return DRIN_OK;
  return timed(DRIN_KC_EDGE, st, "k_ratio_gather", [&] {
    hipLaunchKernelGGL(k_ratio_gather, pair_grid(B, N), dim3(256), 0, st, x, x_mass, rows, row_mass, index, num_rows, out, pairs, N, D / 4, eps,
                       status, (int64_t)0);
  });
}

// dtype: how objects and scores are stored - the instantiation and the timer's name; rows by grid stride: no cap on n to slice for
template <typename T>
int launch_object_rows_as(const char* name, const void* obj, const void* score, int64_t n, int K, int R, float eps, float* out, float* mass,
                          hipStream_t st) {
  const int64_t blocks = row_blocks(n);
  auto kernel = R / 4 <= 512 ? k_object_rows<T, true> : k_object_rows<T, false>;
  return timed(DRIN_KC_POOL, st, name, [&] {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const T*>(obj), static_cast<const T*>(score), n, K, R / 4, eps,
                       out, mass);
  });
}
int launch_object_rows(const void* obj, const void* score, int dtype, int64_t n, int K, int R, float eps, float* out, float* mass, hipStream_t st) {
  if (dtype != DRIN_FEAT_BF16) return launch_object_rows_as<float>("k_object_rows", obj, score, n, K, R, eps, out, mass, st);
  return launch_object_rows_as<__bf16>("k_object_rows_bf16", obj, score, n, K, R, eps, out, mass, st);
}

bool is_finite32(float v) { return v - v == 0.0f; }

// The live terms of a call, in order: a term of weight 0 is dropped here, before anything looks at its pointers.  `pointers`:
// also NULL and alignment of the live terms' three arrays (the size query reads widths and weights only).
struct LiveTerms {
  drin_topk_term term[DRIN_TOPK_MAX_TERMS];
  int widths[DRIN_TOPK_MAX_TERMS];
  int dtypes[DRIN_TOPK_MAX_TERMS];   // how term s stores its rows (row_dtypes of the *_ex twins; DRIN_FEAT_F32 without them)
  drin_topk_form form[DRIN_TOPK_MAX_TERMS];   // the form of term s (forms of the *_forms entry points; DRIN_TOPK_COSINE without them)
  uint32_t ratio_mask = 0;           // bit s: live term s is a DRIN_TOPK_RATIO
  int S = 0;
};
// the form entry of term s, checked: form, that a RATIO term's rows are fp32, eps, and (`pointers`) its two mass arrays
int check_form(const char* who, int s, const drin_topk_form& f, int dtype, bool pointers) {
  if (f.form != DRIN_TOPK_COSINE && f.form != DRIN_TOPK_RATIO) {
    set_error("%s: term %d: form %d is not DRIN_TOPK_COSINE / DRIN_TOPK_RATIO", who, s, f.form);
    return DRIN_E_UNSUPPORTED;
  }
  if (f.form == DRIN_TOPK_COSINE) return DRIN_OK;
  if (dtype != DRIN_FEAT_F32) {
    set_error("%s: term %d: the rows of a DRIN_TOPK_RATIO term are fp32 (row dtype %d)", who, s, dtype);
    return DRIN_E_UNSUPPORTED;
  }
  if (!is_finite32(f.eps)) {
    set_error("%s: term %d: eps is not finite", who, s);
    return DRIN_E_SHAPE;
  }
  if (!pointers) return DRIN_OK;
  if (!f.x_mass || !f.row_mass) {
    set_error("%s: term %d: %s is NULL", who, s, !f.x_mass ? "x_mass" : "row_mass");
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(f.x_mass) & 3u) != 0 || (reinterpret_cast<uintptr_t>(f.row_mass) & 3u) != 0) {
    set_error("%s: term %d: x_mass and row_mass must be 4-byte aligned", who, s);
    return DRIN_E_ALIGN;
  }
  return DRIN_OK;
}
// row_dtypes: HOST array [num_terms] or NULL (all fp32); forms: HOST array [num_terms] or NULL (all cosines); a dropped term's
// entries are not read
int live_terms(const char* who, const drin_topk_term* terms, int num_terms, bool pointers, LiveTerms* out, const int32_t* row_dtypes = nullptr,
               const drin_topk_form* forms = nullptr) {
  if (!terms) {
    set_error("%s: terms is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_count(who, "num_terms", num_terms, 1, DRIN_TOPK_MAX_TERMS));
  for (int s = 0; s < num_terms; ++s) {
    const drin_topk_term& t = terms[s];
    if (!(t.weight - t.weight == 0.0f)) {
      set_error("%s: term %d: weight is not finite", who, s);
      return DRIN_E_SHAPE;
    }
    if (t.weight == 0.0f) continue;
    if (t.width <= 0 || t.width % 4) {
      set_error("%s: term %d: width %d must be a positive multiple of 4 (16-byte lane accesses)", who, s, t.width);
      return DRIN_E_SHAPE;
    }
    const int dtype = row_dtypes != nullptr ? row_dtypes[s] : DRIN_FEAT_F32;
    DRIN_TRY(check_row_dtype(who, dtype, t.width));
    drin_topk_form form = {};   // DRIN_TOPK_COSINE
    if (forms != nullptr) form = forms[s];
    DRIN_TRY(check_form(who, s, form, dtype, pointers));
    const bool ratio = form.form == DRIN_TOPK_RATIO;
    if (pointers) {
      const NamedPtr ptrs[] = {{"x", t.x, true}, {"rows", t.rows, true}, {"row_inv_norms", t.row_inv_norms, !ratio}};
      for (const NamedPtr& p : ptrs) {
        if (!p.required) continue;                            // a RATIO term's inverse norms are not read
        if (!p.p) {
          set_error("%s: term %d: %s is NULL", who, s, p.name);
          return DRIN_E_NULL;
        }
        if (!aligned16(p.p)) {
          set_error("%s: term %d: %s is not 16-byte aligned", who, s, p.name);
          return DRIN_E_ALIGN;
        }
      }
    }
    out->widths[out->S] = t.width;
    out->dtypes[out->S] = dtype;
    out->form[out->S] = form;
    if (ratio) out->ratio_mask |= 1u << out->S;
    out->term[out->S++] = t;
  }
  if (out->S == 0) {
    set_error("%s: no live term (every weight is 0)", who);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

}  // namespace

int launch_widen_rows(const void* rows_bf16, float* out, int64_t n, hipStream_t st) {
  if (n <= 0) return DRIN_OK;
  const int64_t n4 = n / 4, blocks = cdiv(n4, 256) < 65536 ? cdiv(n4, 256) : 65536;   // past the cap a thread walks several quads
  return timed(DRIN_KC_EDGE, st, "k_widen_rows", [&] {
    hipLaunchKernelGGL(k_widen_rows, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const __bf16*>(rows_bf16), out, n4);
  });
}

// drin_host_selftest's two spellings of the one check (topk_layout.h: topk_layout_fault)
static int topk_layout_selfcheck(const int* widths, const int* dtypes, int S, bool summed, int batch, int64_t E, int k, int64_t chunk_entities,
                                 int precision) {
  const char* bad = topk_layout_fault(widths, dtypes, S, summed, batch, E, k, chunk_entities, precision);
  if (bad == nullptr) return DRIN_OK;
  set_error("selftest: TopkLayout (%s) S=%d B=%d E=%lld k=%d chunk=%lld: %s does not hold", summed ? "summed" : "single", S, batch, (long long)E,
            k, (long long)chunk_entities, bad);
  return DRIN_E_WORKSPACE;
}
int table_topk_sum_layout_selfcheck(const int* widths, int S, int batch, int64_t E, int k, int64_t chunk_entities, const int* dtypes,
                                    int precision) {
  return topk_layout_selfcheck(widths, dtypes, S, true, batch, E, k, chunk_entities, precision);
}
int table_topk_layout_selfcheck(int batch, int64_t E, int D, int k, int64_t chunk_entities, int row_dtype, int precision) {
  return topk_layout_selfcheck(&D, &row_dtype, 1, false, batch, E, k, chunk_entities, precision);
}

}  // namespace drin

using namespace drin;

// Each entry point below and its *_ex twin are ONE body: the twin adds how the table rows are stored, the old spelling is
// DRIN_FEAT_F32 - the code it always ran, its bits.  `who` names the spelling that was called.
static int row_inv_norms(const char* who, const void* rows, int row_dtype, int64_t num_entities, int32_t width, float eps, float* out,
                         void* stream) {
  DRIN_CHECK_POINTERS(who, {"rows", rows, true});
  if (!out) {
    set_error("%s: out is NULL", who);
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(out) & 3u) != 0) {
    set_error("%s: out is not 4-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_count(who, "num_entities", num_entities, 1, INT64_MAX / 4096));
  DRIN_TRY(check_row_dtype(who, row_dtype, width));
  DRIN_TRY(check_width4(who, width));
  if (!(eps > 0.0f)) {
    set_error("%s: eps must be positive", who);
    return DRIN_E_SHAPE;
  }
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_row_inv_norms(rows, row_dtype, num_entities, width, eps, out, (hipStream_t)stream);
}
int drin_row_inv_norms(const float* rows, int64_t num_entities, int32_t width, float eps, float* out, void* stream) {
  return row_inv_norms("drin_row_inv_norms", rows, DRIN_FEAT_F32, num_entities, width, eps, out, stream);
}
int drin_row_inv_norms_ex(const void* rows, int32_t row_dtype, int64_t num_entities, int32_t width, float eps, float* out, void* stream) {
  return row_inv_norms("drin_row_inv_norms_ex", rows, row_dtype, num_entities, width, eps, out, stream);
}

int drin_topk_update(const float* block, int64_t ld, int32_t batch, int64_t cols, int64_t col_base, const float* col_inv_norms, int32_t k,
                     float* state_keys, int64_t* state_rows, void* scratch, size_t scratch_bytes, int32_t first, float* out_keys,
                     int64_t* out_rows, void* stream) {
  const char* who = "drin_topk_update";
  DRIN_CHECK_POINTERS(who, {"block", block, cols > 0}, {"state_keys", state_keys, true}, {"state_rows", state_rows, true},
                      {"scratch", scratch, cols > 0});
  if ((reinterpret_cast<uintptr_t>(col_inv_norms) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_keys) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(out_rows) & 7u) != 0) {
    set_error("%s: col_inv_norms and out_keys must be 4-byte, out_rows 8-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  if ((out_keys == nullptr) != (out_rows == nullptr)) {
    set_error("%s: out_keys and out_rows go together (both NULL: no finishing pass)", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_count(who, "batch", batch, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "k", k, 1, kMaxKp));
  DRIN_TRY(check_count(who, "cols", cols, 0, INT32_MAX));
  DRIN_TRY(check_count(who, "col_base", col_base, 0, INT64_MAX / 4096));
  if (cols == 0 && (first || out_keys == nullptr)) {
    set_error("%s: cols = 0 is the finishing call: it needs out_keys / out_rows and first = 0", who);
    return DRIN_E_SHAPE;
  }
  if (cols > 0 && (ld % 4 != 0 || ld < ((int64_t)batch + 3) / 4 * 4 || ld > INT32_MAX)) {
    set_error("%s: ld = %lld must be a multiple of 4, at least batch rounded up to one and at most 2^31 - 1", who, (long long)ld);
    return DRIN_E_SHAPE;
  }
  const int kp = DRIN_TOPK_KP(k);
  const size_t need = topk_scratch_bytes(batch, cols, kp);
  if (scratch_bytes < need) {
    set_error("%s: scratch %zu bytes < %zu", who, scratch_bytes, need);
    return DRIN_E_WORKSPACE;
  }
  DRIN_BIND_DEVICE(stream, state_keys, who);
  hipStream_t st = (hipStream_t)stream;
  if (cols > 0)
    DRIN_TRY(launch_topk_update(block, ld, batch, cols, col_base, col_inv_norms, kp, state_keys, state_rows, static_cast<uint64_t*>(scratch),
                                first != 0, st));
  if (out_keys != nullptr) DRIN_TRY(launch_topk_finish(state_keys, state_rows, batch, kp, k, out_keys, out_rows, st));
  return DRIN_OK;
}

static size_t table_topk_workspace_bytes(const char* who, int32_t batch, int64_t num_entities, int32_t width, int32_t k, int64_t chunk_entities,
                                         int row_dtype, int precision) {
  TopkLayout W;
  if (plan_topk(who, &width, &row_dtype, 1, false, batch, num_entities, k, chunk_entities, precision, nullptr, &W) != DRIN_OK) return 0;
  return W.total_floats * sizeof(float);
}
size_t drin_table_topk_workspace_bytes(int32_t batch, int64_t num_entities, int32_t width, int32_t k, int64_t chunk_entities) {
  return table_topk_workspace_bytes("drin_table_topk_workspace_bytes", batch, num_entities, width, k, chunk_entities, DRIN_FEAT_F32,
                                    DRIN_PREC_F32);
}
size_t drin_table_topk_workspace_bytes_ex(int32_t batch, int64_t num_entities, int32_t width, int32_t k, int64_t chunk_entities,
                                          int32_t row_dtype, int32_t precision) {
  return table_topk_workspace_bytes("drin_table_topk_workspace_bytes_ex", batch, num_entities, width, k, chunk_entities, row_dtype, precision);
}

static int table_topk(const char* who, const float* x, const void* rows, int row_dtype, const float* row_inv_norms, int64_t num_entities,
                      int32_t batch, int32_t width, int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities, void* workspace,
                      size_t workspace_bytes, float* out_scores, int64_t* out_rows, void* stream) {
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"rows", rows, true}, {"row_inv_norms", row_inv_norms, true}, {"workspace", workspace, true});
  if (!out_scores || !out_rows) {
    set_error("%s: out_scores / out_rows is NULL", who);
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(out_scores) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_rows) & 7u) != 0) {
    set_error("%s: out_scores must be 4-byte and out_rows 8-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  TopkLayout W;
  DRIN_TRY(plan_topk(who, &width, &row_dtype, 1, false, batch, num_entities, k, chunk_entities, precision, &workspace_bytes, &W));
  DRIN_BIND_DEVICE(stream, out_scores, who);
  RoctxRange range(who);
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const int B = batch, D = width, kp = W.kp, Bp = W.Bp;
  float* planes = W.planes_floats[0] ? ws + W.planes[0] : nullptr;
  float* xpad = ws + W.xpad[0];
  float* block = ws + W.block[0];
  float* keys = ws + W.keys;
  int64_t* list = reinterpret_cast<int64_t*>(ws + W.rows);
  uint64_t* slices = reinterpret_cast<uint64_t*>(ws + W.slices);
  float* scores = ws + W.scores;
  DRIN_TRY(launch_pad_rows(x, xpad, B, Bp, D, st));
  // bf16-stored rows on the plane route: the padded mentions as hi / lo planes, split ONCE per call (hi: Bp D bf16, then lo)
  if (planes != nullptr)
    DRIN_TRY(launch_split_planes(xpad, planes, reinterpret_cast<uint16_t*>(planes) + (size_t)Bp * D, (int64_t)Bp * D, st));
  // per chunk of table rows: y[n, Bp] = rows_chunk x^T - the entities are the ROW side, so launch_gemm_nt routes every chunk by the
  // chunk's size, not by the batch's - then the selection on that block
  for (int64_t e0 = 0; e0 < num_entities; e0 += W.chunk) {
    const int64_t n = num_entities - e0 < W.chunk ? num_entities - e0 : W.chunk;
    DRIN_TRY(launch_chunk_product(rows, row_dtype, e0, n, D, xpad, planes, ws + W.widen, W.widen_floats, block, Bp, precision, st));
    DRIN_TRY(launch_topk_update(block, Bp, B, n, e0, row_inv_norms + e0, kp, keys, list, slices, e0 == 0, st));
  }
  // the kp selected rows of every mention, scored as drin_cosine_rows_indexed_fwd(_ex) scores them (an empty entry, row -1, is
  // clamped silently and stays last), ordered by the contract
  DRIN_TRY(launch_cosine_gather(x, rows, row_dtype, list, num_entities, scores, B, kp, D, cosine_eps, nullptr, 0, st));
  return launch_topk_finish(scores, list, B, kp, k, out_scores, out_rows, st);
}
int drin_table_topk(const float* x, const float* rows, const float* row_inv_norms, int64_t num_entities, int32_t batch, int32_t width,
                    int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities, void* workspace, size_t workspace_bytes,
                    float* out_scores, int64_t* out_rows, void* stream) {
  return table_topk("drin_table_topk", x, rows, DRIN_FEAT_F32, row_inv_norms, num_entities, batch, width, k, cosine_eps, precision,
                    chunk_entities, workspace, workspace_bytes, out_scores, out_rows, stream);
}
int drin_table_topk_ex(const float* x, const void* rows, int32_t row_dtype, const float* row_inv_norms, int64_t num_entities, int32_t batch,
                       int32_t width, int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities, void* workspace,
                       size_t workspace_bytes, float* out_scores, int64_t* out_rows, void* stream) {
  return table_topk("drin_table_topk_ex", x, rows, row_dtype, row_inv_norms, num_entities, batch, width, k, cosine_eps, precision,
                    chunk_entities, workspace, workspace_bytes, out_scores, out_rows, stream);
}

// drin_topk_combine and drin_topk_combine_forms are ONE body: forms NULL (the old spelling) or all cosines is the old launch
static int topk_combine(const char* who, const float* const* blocks, const float* const* col_inv_norms, const float* const* row_scales,
                        const float* weights, const drin_topk_form* forms, int32_t num_terms, int64_t ld, int32_t batch, int64_t cols, float* out,
                        void* stream) {
  if (!blocks || !col_inv_norms || !row_scales || !weights || !out) {
    set_error("%s: %s is NULL", who, !blocks ? "blocks" : !col_inv_norms ? "col_inv_norms" : !row_scales ? "row_scales" : !weights ? "weights" : "out");
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_count(who, "num_terms", num_terms, 1, DRIN_TOPK_MAX_TERMS));
  FormTerms ft = {};
  CombineTerms& t = ft.t;
  for (int s = 0; s < num_terms; ++s) {
    if (forms != nullptr && forms[s].form != DRIN_TOPK_COSINE) {   // a RATIO term: the masses stand where inverse norms and factors do
      const drin_topk_form& f = forms[s];
      DRIN_TRY(check_form(who, s, f, DRIN_FEAT_F32, true));
      if (!blocks[s]) {
        set_error("%s: term %d: blocks is NULL", who, s);
        return DRIN_E_NULL;
      }
      if (!aligned16(blocks[s]) || !aligned16(f.x_mass)) {
        set_error("%s: term %d: blocks and x_mass must be 16-byte aligned", who, s);
        return DRIN_E_ALIGN;
      }
      if (!is_finite32(weights[s])) {
        set_error("%s: term %d: weight is not finite", who, s);
        return DRIN_E_SHAPE;
      }
      t.block[s] = blocks[s], t.inv[s] = f.row_mass, t.scale[s] = f.x_mass, t.weight[s] = weights[s];
      ft.eps[s] = f.eps, ft.ratio_mask |= 1u << s;
      continue;
    }
    if (!blocks[s] || !col_inv_norms[s] || !row_scales[s]) {
      set_error("%s: term %d: %s is NULL", who, s, !blocks[s] ? "blocks" : !col_inv_norms[s] ? "col_inv_norms" : "row_scales");
      return DRIN_E_NULL;
    }
    if (!aligned16(blocks[s]) || !aligned16(row_scales[s]) || (reinterpret_cast<uintptr_t>(col_inv_norms[s]) & 3u) != 0) {
      set_error("%s: term %d: blocks and row_scales must be 16-byte, col_inv_norms 4-byte aligned", who, s);
      return DRIN_E_ALIGN;
    }
    if (!(weights[s] - weights[s] == 0.0f)) {
      set_error("%s: term %d: weight is not finite", who, s);
      return DRIN_E_SHAPE;
    }
    t.block[s] = blocks[s], t.inv[s] = col_inv_norms[s], t.scale[s] = row_scales[s], t.weight[s] = weights[s];
  }
  if (!aligned16(out)) {
    set_error("%s: out is not 16-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_count(who, "batch", batch, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "cols", cols, 1, INT32_MAX));
  if (ld % 4 != 0 || ld < ((int64_t)batch + 3) / 4 * 4 || ld > INT32_MAX) {
    set_error("%s: ld = %lld must be a multiple of 4, at least batch rounded up to one and at most 2^31 - 1", who, (long long)ld);
    return DRIN_E_SHAPE;
  }
  DRIN_BIND_DEVICE(stream, out, who);
  if (ft.ratio_mask == 0) return launch_topk_combine(t, num_terms, out, ld, cols, (hipStream_t)stream);
  return launch_topk_forms_combine(ft, num_terms, out, ld, cols, (hipStream_t)stream);
}
int drin_topk_combine(const float* const* blocks, const float* const* col_inv_norms, const float* const* row_scales, const float* weights,
                      int32_t num_terms, int64_t ld, int32_t batch, int64_t cols, float* out, void* stream) {
  return topk_combine("drin_topk_combine", blocks, col_inv_norms, row_scales, weights, nullptr, num_terms, ld, batch, cols, out, stream);
}
int drin_topk_combine_forms(const float* const* blocks, const float* const* col_inv_norms, const float* const* row_scales, const float* weights,
                            const drin_topk_form* forms, int32_t num_terms, int64_t ld, int32_t batch, int64_t cols, float* out, void* stream) {
  return topk_combine("drin_topk_combine_forms", blocks, col_inv_norms, row_scales, weights, forms, num_terms, ld, batch, cols, out, stream);
}

static size_t table_topk_sum_workspace_bytes(const char* who, const drin_topk_term* terms, const int32_t* row_dtypes, int32_t num_terms,
                                             int32_t batch, int64_t num_entities, int32_t k, int64_t chunk_entities, int precision,
                                             const drin_topk_form* forms = nullptr) {
  LiveTerms live;
  if (live_terms(who, terms, num_terms, false, &live, row_dtypes, forms) != DRIN_OK) return 0;
  TopkLayout W;
  if (plan_topk(who, live.widths, live.dtypes, live.S, true, batch, num_entities, k, chunk_entities, precision, nullptr, &W) != DRIN_OK) return 0;
  return W.total_floats * sizeof(float);
}
size_t drin_table_topk_sum_workspace_bytes(const drin_topk_term* terms, int32_t num_terms, int32_t batch, int64_t num_entities, int32_t k,
                                           int64_t chunk_entities) {
  return table_topk_sum_workspace_bytes("drin_table_topk_sum_workspace_bytes", terms, nullptr, num_terms, batch, num_entities, k,
                                        chunk_entities, DRIN_PREC_F32);
}
size_t drin_table_topk_sum_workspace_bytes_ex(const drin_topk_term* terms, const int32_t* row_dtypes, int32_t num_terms, int32_t batch,
                                              int64_t num_entities, int32_t k, int64_t chunk_entities, int32_t precision) {
  const char* who = "drin_table_topk_sum_workspace_bytes_ex";
  if (!row_dtypes) {
    set_error("%s: row_dtypes is NULL", who);
    return 0;
  }
  return table_topk_sum_workspace_bytes(who, terms, row_dtypes, num_terms, batch, num_entities, k, chunk_entities, precision);
}

static int table_topk_sum(const char* who, const drin_topk_term* terms, const int32_t* row_dtypes, const drin_topk_form* forms,
                          int32_t num_terms, int64_t num_entities, int32_t batch, int32_t k, float cosine_eps, int32_t precision,
                          int64_t chunk_entities, void* workspace, size_t workspace_bytes, float* out_scores, int64_t* out_rows, void* stream) {
  LiveTerms live;
  DRIN_TRY(live_terms(who, terms, num_terms, true, &live, row_dtypes, forms));
  DRIN_CHECK_POINTERS(who, {"workspace", workspace, true});
  if (!out_scores || !out_rows) {
    set_error("%s: out_scores / out_rows is NULL", who);
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(out_scores) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_rows) & 7u) != 0) {
    set_error("%s: out_scores must be 4-byte and out_rows 8-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  TopkLayout W;
  DRIN_TRY(plan_topk(who, live.widths, live.dtypes, live.S, true, batch, num_entities, k, chunk_entities, precision, &workspace_bytes, &W));
  DRIN_BIND_DEVICE(stream, out_scores, who);
  RoctxRange range(who);
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const int B = batch, S = live.S, kp = W.kp, Bp = W.Bp;
  float* keys = ws + W.keys;
  int64_t* list = reinterpret_cast<int64_t*>(ws + W.rows);
  uint64_t* slices = reinterpret_cast<uint64_t*>(ws + W.slices);
  float* cos = ws + W.cos;
  float* scores = ws + W.scores;
  FormTerms ft = {};                    // (without a RATIO term only its CombineTerms are used: the old launch)
  CombineTerms& ct = ft.t;
  ChainWeights cw = {};
  ft.ratio_mask = live.ratio_mask;
  // the mentions of every term padded to Bp rows, and their factors 1 / max(|x_s[b]|, eps): unlike the single cosine, the mention
  // norms differ from term to term and do change the ranking (the weight joins them inside the combine)
  for (int s = 0; s < S; ++s) {
    const drin_topk_term& t = live.term[s];
    float* xpad = ws + W.xpad[s];
    DRIN_TRY(launch_pad_rows(t.x, xpad, B, Bp, t.width, st));
    if (live.ratio_mask >> s & 1u) {   // a RATIO term: the factor region holds the mentions' masses, padded with zeros
      DRIN_TRY(launch_pad_mass(live.form[s].x_mass, ws + W.scale[s], B, Bp, st));
      ft.eps[s] = live.form[s].eps;
    } else {
      DRIN_TRY(launch_row_inv_norms(xpad, DRIN_FEAT_F32, Bp, t.width, cosine_eps, ws + W.scale[s], st));
    }
    if (W.planes_floats[s])   // a bf16-stored term on the plane route: its padded mentions as hi / lo planes, once per call
      DRIN_TRY(launch_split_planes(xpad, ws + W.planes[s], reinterpret_cast<uint16_t*>(ws + W.planes[s]) + (size_t)Bp * t.width,
                                   (int64_t)Bp * t.width, st));
    ct.block[s] = ws + W.block[s], ct.scale[s] = ws + W.scale[s], ct.weight[s] = t.weight, cw.w[s] = t.weight;
  }
  // per chunk of table rows: one product per live term into its own entity-major block (kernel choice: the GEMM module's, by the
  // chunk's row count), ONE combine into block 0, then the selection on the combined scores (no inverse norms left to apply)
  float* combined = ws + W.block[0];
  for (int64_t e0 = 0; e0 < num_entities; e0 += W.chunk) {
    const int64_t n = num_entities - e0 < W.chunk ? num_entities - e0 : W.chunk;
    for (int s = 0; s < S; ++s) {
      const drin_topk_term& t = live.term[s];
      DRIN_TRY(launch_chunk_product(t.rows, live.dtypes[s], e0, n, t.width, ws + W.xpad[s], W.planes_floats[s] ? ws + W.planes[s] : nullptr,
                                    ws + W.widen, W.widen_floats, ws + W.block[s], Bp, precision, st));
      ct.inv[s] = ((live.ratio_mask >> s & 1u) ? live.form[s].row_mass : t.row_inv_norms) + e0;
    }
    if (live.ratio_mask == 0)
      DRIN_TRY(launch_topk_combine(ct, S, combined, Bp, n, st));
    else
      DRIN_TRY(launch_topk_forms_combine(ft, S, combined, Bp, n, st));
    DRIN_TRY(launch_topk_update(combined, Bp, B, n, e0, nullptr, kp, keys, list, slices, e0 == 0, st));
  }
  // the kp selected rows scored again, term by term as drin_cosine_rows_indexed_fwd scores them (an empty entry, row -1, is clamped
  // silently and stays last), the fp32 chain over the terms, and the order of the contract
  for (int s = 0; s < S; ++s) {
    const drin_topk_term& t = live.term[s];
    if (live.ratio_mask >> s & 1u) {   // drin_ratio_rows_indexed_fwd's bits
      DRIN_TRY(launch_ratio_gather(t.x, live.form[s].x_mass, t.rows, live.form[s].row_mass, list, num_entities, cos + (size_t)s * B * kp, B, kp,
                                   t.width, live.form[s].eps, nullptr, st));
      continue;
    }
    DRIN_TRY(launch_cosine_gather(t.x, t.rows, live.dtypes[s], list, num_entities, cos + (size_t)s * B * kp, B, kp, t.width, cosine_eps, nullptr, 0,
                                  st));
  }
  DRIN_TRY(launch_weighted_cosine_sum(cos, S, (int64_t)B * kp, cw, scores, st));
  return launch_topk_finish(scores, list, B, kp, k, out_scores, out_rows, st);
}
int drin_table_topk_sum(const drin_topk_term* terms, int32_t num_terms, int64_t num_entities, int32_t batch, int32_t k, float cosine_eps,
                        int32_t precision, int64_t chunk_entities, void* workspace, size_t workspace_bytes, float* out_scores,
                        int64_t* out_rows, void* stream) {
  return table_topk_sum("drin_table_topk_sum", terms, nullptr, nullptr, num_terms, num_entities, batch, k, cosine_eps, precision, chunk_entities,
                        workspace, workspace_bytes, out_scores, out_rows, stream);
}
int drin_table_topk_sum_ex(const drin_topk_term* terms, const int32_t* row_dtypes, int32_t num_terms, int64_t num_entities, int32_t batch,
                           int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities, void* workspace, size_t workspace_bytes,
                           float* out_scores, int64_t* out_rows, void* stream) {
  const char* who = "drin_table_topk_sum_ex";
  if (!row_dtypes) {
    set_error("%s: row_dtypes is NULL", who);
    return DRIN_E_NULL;
  }
  return table_topk_sum(who, terms, row_dtypes, nullptr, num_terms, num_entities, batch, k, cosine_eps, precision, chunk_entities, workspace,
                        workspace_bytes, out_scores, out_rows, stream);
}
size_t drin_table_topk_sum_forms_workspace_bytes(const drin_topk_term* terms, const int32_t* row_dtypes, const drin_topk_form* forms,
                                                 int32_t num_terms, int32_t batch, int64_t num_entities, int32_t k, int64_t chunk_entities,
                                                 int32_t precision) {
  return table_topk_sum_workspace_bytes("drin_table_topk_sum_forms_workspace_bytes", terms, row_dtypes, num_terms, batch, num_entities, k,
                                        chunk_entities, precision, forms);
}
int drin_table_topk_sum_forms(const drin_topk_term* terms, const int32_t* row_dtypes, const drin_topk_form* forms, int32_t num_terms,
                              int64_t num_entities, int32_t batch, int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities,
                              void* workspace, size_t workspace_bytes, float* out_scores, int64_t* out_rows, void* stream) {
  return table_topk_sum("drin_table_topk_sum_forms", terms, row_dtypes, forms, num_terms, num_entities, batch, k, cosine_eps, precision,
                        chunk_entities, workspace, workspace_bytes, out_scores, out_rows, stream);
}

int drin_object_rows(const void* obj, const void* score, int32_t dtype, int64_t n, int32_t K, int32_t width, float eps, float* out, float* mass,
                     void* stream) {
  const char* who = "drin_object_rows";
  DRIN_CHECK_POINTERS(who, {"obj", obj, true}, {"out", out, true});
  if (!score || !mass) {
    set_error("%s: %s is NULL", who, !score ? "score" : "mass");
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_row_dtype(who, dtype, width));
  if ((reinterpret_cast<uintptr_t>(score) & (dtype == DRIN_FEAT_BF16 ? 1u : 3u)) != 0 || (reinterpret_cast<uintptr_t>(mass) & 3u) != 0) {
    set_error("%s: score must be aligned to its element and mass 4-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_count(who, "n", n, 1, INT64_MAX / 4096));
  DRIN_TRY(check_count(who, "K", K, 1, kObjectMaxK));
  DRIN_TRY(check_width4(who, width));
  if (!(eps > 0.0f)) {
    set_error("%s: eps must be positive", who);
    return DRIN_E_SHAPE;
  }
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_object_rows(obj, score, dtype, n, K, width, eps, out, mass, (hipStream_t)stream);
}

int drin_ratio_rows_indexed_fwd(const float* x, const float* x_mass, const float* rows, const float* row_mass, const int64_t* index,
                                int64_t num_entities, float* out, int32_t batch, int32_t num_candidates, int32_t width, float eps,
                                int32_t* index_status, void* stream) {
  const char* who = "drin_ratio_rows_indexed_fwd";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"rows", rows, true});
  if (!x_mass || !row_mass || !index || !out) {
    set_error("%s: %s is NULL", who, !x_mass ? "x_mass" : !row_mass ? "row_mass" : !index ? "index" : "out");
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(index) & 7u) != 0 || (reinterpret_cast<uintptr_t>(index_status) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(x_mass) & 3u) != 0 || (reinterpret_cast<uintptr_t>(row_mass) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(out) & 3u) != 0) {
    set_error("%s: index must be 8-byte, x_mass, row_mass, out and index_status 4-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_count(who, "num_entities", num_entities, 1, INT64_MAX / 4096));
  DRIN_TRY(check_width4(who, width));
  if (!is_finite32(eps)) {
    set_error("%s: eps is not finite", who);
    return DRIN_E_SHAPE;
  }
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "num_candidates", num_candidates, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "batch * num_candidates", (int64_t)batch * num_candidates, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_ratio_gather(x, x_mass, rows, row_mass, index, num_entities, out, batch, num_candidates, width, eps, index_status,
                             (hipStream_t)stream);
}

int drin_rank_rows(const float* scores, const int64_t* rows, int32_t batch, int32_t n, int32_t k, float* out_scores, int64_t* out_rows,
                   int32_t* out_slots, void* stream) {
  const char* who = "drin_rank_rows";
  if (!scores || !rows || !out_scores || !out_rows) {
    set_error("%s: %s is NULL", who, !scores ? "scores" : !rows ? "rows" : !out_scores ? "out_scores" : "out_rows");
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(scores) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_scores) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(out_slots) & 3u) != 0 || (reinterpret_cast<uintptr_t>(rows) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(out_rows) & 7u) != 0) {
    set_error("%s: scores, out_scores and out_slots must be 4-byte, rows and out_rows 8-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_count(who, "batch", batch, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "n", n, 1, kMaxRankRows));
  DRIN_TRY(check_count(who, "k", k, 1, kMaxRankRows));
  if (k > n) {
    set_error("%s: k = %d exceeds n = %d", who, k, n);
    return DRIN_E_SHAPE;
  }
  DRIN_BIND_DEVICE(stream, out_scores, who);
  return launch_rank_rows(scores, rows, batch, n, k, out_scores, out_rows, out_slots, (hipStream_t)stream);
}
