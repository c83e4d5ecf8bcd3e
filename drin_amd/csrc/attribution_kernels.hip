// Gradient x input attribution: the contractions that stand where the input-gradient kernels expand.
//   k_token_attribution   out[p, t] = <tokens[row, t, :], g_pool[p, :]> / cnt on the tokens the entity pooling averages
//                         (ghmfc.py:245-249), exactly 0 elsewhere: the counterpart of k_token_block_bwd (input_grad_kernels.hip),
//                         which writes g_pool / cnt to those rows of a [pairs, T, D] gradient; here that gradient never exists
//   k_rows_dot            out[r] = <x[r, :], g[r, :]>
// Both are HBM-bound reads of rows that are used once (16-byte non-temporal loads), every output is WRITTEN by exactly one lane and
// every sum runs in a fixed order (lane partials, the DPP wave sum, wave partials in wave order): no atomics beyond the error-path
// report of a clamped index, no scratch memory, the same bits every run.
#include "device_utils.h"
#include "row_checks.h"

namespace drin {
namespace {

// sixteen bytes of a row: four fp32 or eight bf16 columns (widened exactly: a bf16 is the upper half of its fp32)
template <typename T_>
struct Chunk {
  static constexpr int V = 4;
};
template <>
struct Chunk<__bf16> {
  static constexpr int V = 8;
};
__device__ __forceinline__ u32x4_t zero16() {
  u32x4_t z = {0u, 0u, 0u, 0u};
  return z;
}
template <typename T_>
__device__ __forceinline__ float dot16(u32x4_t raw, const float4* g, float acc);
template <>
__device__ __forceinline__ float dot16<float>(u32x4_t raw, const float4* g, float acc) {
  typedef float f4_t __attribute__((ext_vector_type(4)));
  const f4_t x = __builtin_bit_cast(f4_t, raw);   // (the whole vector: a bit cast of one element lvalue reads element 0)
  return acc + dot4(make_float4(x[0], x[1], x[2], x[3]), g[0]);
}
template <>
__device__ __forceinline__ float dot16<__bf16>(u32x4_t raw, const float4* g, float acc) {
  const float4 a = make_float4(__builtin_bit_cast(float, raw[0] << 16), __builtin_bit_cast(float, raw[0] & 0xffff0000u),
                               __builtin_bit_cast(float, raw[1] << 16), __builtin_bit_cast(float, raw[1] & 0xffff0000u));
  const float4 b = make_float4(__builtin_bit_cast(float, raw[2] << 16), __builtin_bit_cast(float, raw[2] & 0xffff0000u),
                               __builtin_bit_cast(float, raw[3] << 16), __builtin_bit_cast(float, raw[3] & 0xffff0000u));
  return (acc + dot4(a, g[0])) + dot4(b, g[1]);
}

__device__ __forceinline__ int64_t clamp_row(int64_t raw, int64_t num_rows) { return raw < 0 ? 0 : (raw >= num_rows ? num_rows - 1 : raw); }

// rows 1 .. stop - 1 are averaged by the pooling: k_entity_token_mean's slice rules (python's negative stop for ntok == 0)
__device__ __forceinline__ int pool_stop(int ntok, int T) {
  int stop = ntok - 1;
  if (stop < 0) stop += T;
  if (stop < 0) stop = 0;
  if (stop > T) stop = T;
  return stop;
}

struct PairRows {
  const int64_t* index;   // [pairs] rows of the table, or NULL: pair p reads row p
  int64_t num_rows;       // E
  int64_t pair_base;      // added to p in a report (a slice of a larger call)
  int32_t* status;        // int32[4] or NULL
};

// One wave walks tokens first, first + step, ... < stop of one pair, two rows in flight, and lane 0 stores each row's sum / den.
// SLOTS > 0: the width fits SLOTS 16-byte chunks per lane (guarded: C <= 64 * SLOTS chunks in a row) and the pair's gradient row
// stays in registers across the token loop; SLOTS == 0: any width, the gradient chunks are re-read (L1 / L2 hits) per row pair.
template <typename T_, int SLOTS>
__device__ __forceinline__ void attribute_tokens(const T_* __restrict__ rows, const float* __restrict__ g, float* __restrict__ out,
                                                 int first, int step, int stop, int C, float den, int lane) {
  constexpr int V = Chunk<T_>::V, G4 = V / 4;
  const int64_t row_bytes = (int64_t)C * 16;
  const char* base = reinterpret_cast<const char*>(rows);
  if constexpr (SLOTS > 0) {
    float4 gr[SLOTS][G4];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c = s * 64 + lane;
#pragma unroll
      for (int k = 0; k < G4; ++k) gr[s][k] = c < C ? ld4(g + (int64_t)c * V + k * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int t = first; t < stop; t += 2 * step) {
      const bool two = t + step < stop;   // wave-uniform
      u32x4_t r0[SLOTS], r1[SLOTS];
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int c = s * 64 + lane;
        r0[s] = c < C ? ld16_stream(base + t * row_bytes + (int64_t)c * 16) : zero16();
        r1[s] = (two && c < C) ? ld16_stream(base + (t + step) * row_bytes + (int64_t)c * 16) : zero16();
      }
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        a0 = dot16<T_>(r0[s], gr[s], a0);
        a1 = dot16<T_>(r1[s], gr[s], a1);
      }
      a0 = wave_sum(a0);
      a1 = wave_sum(a1);
      if (lane == 0) {
        out[t] = a0 / den;
        if (two) out[t + step] = a1 / den;
      }
    }
  } else {
    for (int t = first; t < stop; t += 2 * step) {
      const bool two = t + step < stop;
      float a0 = 0.f, a1 = 0.f;
      for (int c = lane; c < C; c += 64) {
        const u32x4_t r0 = ld16_stream(base + t * row_bytes + (int64_t)c * 16);
        const u32x4_t r1 = two ? ld16_stream(base + (t + step) * row_bytes + (int64_t)c * 16) : zero16();
        float4 gr[G4];
#pragma unroll
        for (int k = 0; k < G4; ++k) gr[k] = ld4(g + (int64_t)c * V + k * 4);
        a0 = dot16<T_>(r0, gr, a0);
        a1 = dot16<T_>(r1, gr, a1);
      }
      a0 = wave_sum(a0);
      a1 = wave_sum(a1);
      if (lane == 0) {
        out[t] = a0 / den;
        if (two) out[t + step] = a1 / den;
      }
    }
  }
}

// One workgroup of 256 threads per pair: the mask row is read once (each thread its tokens, four wave sums through LDS), wave w
// walks tokens 1 + w, 5 + w, ...; the threads then write the zeros of token 0 and of the tokens behind the slice.  C = width in
// 16-byte chunks.  grid: (pairs of this slice).
template <typename T_, int SLOTS>
__global__ void __launch_bounds__(256) k_token_attribution(const T_* __restrict__ tokens, const int64_t* __restrict__ mask,
                                                           const float* __restrict__ g_pool, float* __restrict__ out, int T, int C,
                                                           PairRows rows) {
  __shared__ int s_cnt[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = blockIdx.x;
  int64_t src = p;
  if (rows.index != nullptr) {
    const int64_t raw = rows.index[p];
    src = clamp_row(raw, rows.num_rows);   // before any address is formed from it
    if (src != raw && threadIdx.x == 0) report_bad_index(rows.status, rows.pair_base + p, raw);
  }
  int cnt = 0;
  for (int t = threadIdx.x; t < T; t += 256) cnt += (int)mask[src * T + t];
  cnt = (int)wave_sum((float)cnt);   // T <= 2^24: exact in fp32
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  const int stop = pool_stop((s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]), T);
  constexpr int V = Chunk<T_>::V;
  float* o = out + p * (int64_t)T;
  attribute_tokens<T_, SLOTS>(tokens + src * (int64_t)T * C * V, g_pool + p * (int64_t)C * V, o, 1 + wave, 4, stop, C,
                              (float)(stop - 1), lane);
  for (int t = threadIdx.x; t < T; t += 256)
    if (t == 0 || t >= stop) o[t] = 0.0f;
}

// Short token rows (at most kWavePairMaxKept tokens can be kept): one wave per pair, four pairs per workgroup, no LDS.
// grid: (ceil(pairs of this slice / 4)).
constexpr int kWavePairMaxKept = 4;
template <typename T_, int SLOTS>
__global__ void __launch_bounds__(256) k_token_attribution_wave(const T_* __restrict__ tokens, const int64_t* __restrict__ mask,
                                                                const float* __restrict__ g_pool, float* __restrict__ out,
                                                                int64_t pairs, int T, int C, PairRows rows) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= pairs) return;
  int64_t src = p;
  if (rows.index != nullptr) {
    const int64_t raw = rows.index[p];
    src = clamp_row(raw, rows.num_rows);
    if (src != raw && lane == 0) report_bad_index(rows.status, rows.pair_base + p, raw);
  }
  int cnt = 0;
  for (int t = lane; t < T; t += 64) cnt += (int)mask[src * T + t];
  const int stop = pool_stop((int)wave_sum((float)cnt), T);
  constexpr int V = Chunk<T_>::V;
  float* o = out + p * (int64_t)T;
  attribute_tokens<T_, SLOTS>(tokens + src * (int64_t)T * C * V, g_pool + p * (int64_t)C * V, o, 1, 1, stop, C, (float)(stop - 1),
                              lane);
  for (int t = lane; t < T; t += 64)
    if (t == 0 || t >= stop) o[t] = 0.0f;
}

// out[r] = <x[r, :], g[r, :]>, one wave per row, four rows per workgroup, the rest by grid stride
template <typename T_>
__global__ void __launch_bounds__(256) k_rows_dot(const T_* __restrict__ x, const float* __restrict__ g, float* __restrict__ out,
                                                  int64_t rows, int C) {
  constexpr int V = Chunk<T_>::V, G4 = V / 4;
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    const char* xr = reinterpret_cast<const char*>(x) + r * (int64_t)C * 16;
    const float* gr = g + r * (int64_t)C * V;
    float a = 0.f;
    for (int c = lane; c < C; c += 64) {
      const u32x4_t raw = ld16_stream(xr + (int64_t)c * 16);
      float4 gv[G4];
#pragma unroll
      for (int k = 0; k < G4; ++k) gv[k] = ld4_stream(gr + (int64_t)c * V + k * 4);
      a = dot16<T_>(raw, gv, a);
    }
    a = wave_sum(a);
    if (lane == 0) out[r] = a;
  }
}

// the same with a workgroup per row (rows wider than kRowsDotWaveWidth): the four wave sums are added in wave order
constexpr int kRowsDotWaveWidth = 2048;
template <typename T_>
__global__ void __launch_bounds__(256) k_rows_dot_wide(const T_* __restrict__ x, const float* __restrict__ g, float* __restrict__ out,
                                                       int64_t rows, int C) {
  constexpr int V = Chunk<T_>::V, G4 = V / 4;
  __shared__ float part[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const char* xr = reinterpret_cast<const char*>(x) + r * (int64_t)C * 16;
    const float* gr = g + r * (int64_t)C * V;
    float a = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
      const u32x4_t raw = ld16_stream(xr + (int64_t)c * 16);
      float4 gv[G4];
#pragma unroll
      for (int k = 0; k < G4; ++k) gv[k] = ld4_stream(gr + (int64_t)c * V + k * 4);
      a = dot16<T_>(raw, gv, a);
    }
    a = wave_sum(a);
    if (lane == 0) part[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) out[r] = (part[0] + part[1]) + (part[2] + part[3]);
    __syncthreads();   // part is rewritten by the next row
  }
}

// chunks per row that the register-resident instantiation holds: 4 slots of fp32 chunks, 2 of bf16 chunks = widths up to 1024
template <typename T_>
constexpr int kRegSlots = 16 / Chunk<T_>::V;

template <typename T_>
int launch_token_attribution_t(const T_* tokens, const int64_t* mask, const int64_t* index, int64_t num_rows, int32_t* status,
                               const float* g_pool, float* out, int64_t pairs, int T, int D, hipStream_t st) {
  constexpr int V = Chunk<T_>::V;
  const int C = D / V;
  const bool reg = C <= 64 * kRegSlots<T_>;
  const bool per_wave = T - 2 <= kWavePairMaxKept;
  const int ppb = per_wave ? 4 : 1;   // pairs per workgroup
  // slices of kMaxGridY workgroups: every pointer moves by the slice's first pair (a table and its index do not: the index does)
  return for_grid_slices(cdiv(pairs, ppb), [&](int64_t wg0, int nwg) -> int {
    const int64_t p0 = wg0 * ppb;
    const int64_t np = pairs - p0 < (int64_t)nwg * ppb ? pairs - p0 : (int64_t)nwg * ppb;
    const T_* tk = index ? tokens : tokens + p0 * T * D;
    const int64_t* mk = index ? mask : mask + p0 * T;
    const PairRows rows{index ? index + p0 : nullptr, num_rows, p0, status};
    const float* g = g_pool + p0 * D;
    float* o = out + p0 * T;
    KernelTimer timer(DRIN_KC_POOL, st);
    if (per_wave) {
      if (reg)
        hipLaunchKernelGGL((k_token_attribution_wave<T_, kRegSlots<T_>>), dim3((unsigned)nwg), dim3(256), 0, st, tk, mk, g, o, np, T, C, rows);
      else
        hipLaunchKernelGGL((k_token_attribution_wave<T_, 0>), dim3((unsigned)nwg), dim3(256), 0, st, tk, mk, g, o, np, T, C, rows);
    } else {
      if (reg)
        hipLaunchKernelGGL((k_token_attribution<T_, kRegSlots<T_>>), dim3((unsigned)nwg), dim3(256), 0, st, tk, mk, g, o, T, C, rows);
      else
        hipLaunchKernelGGL((k_token_attribution<T_, 0>), dim3((unsigned)nwg), dim3(256), 0, st, tk, mk, g, o, T, C, rows);
    }
    DRIN_CHECK_LAUNCH("k_token_attribution");
    return DRIN_OK;
  });
}

template <typename T_>
int launch_rows_dot_t(const T_* x, const float* g, float* out, int64_t rows, int width, hipStream_t st) {
  const int C = width / Chunk<T_>::V;
  return timed(DRIN_KC_POOL, st, "k_rows_dot", [&] {
    if (width > kRowsDotWaveWidth) {
      const int64_t blocks = rows < kMaxRowBlocks ? rows : kMaxRowBlocks;
      hipLaunchKernelGGL(k_rows_dot_wide<T_>, dim3((unsigned)blocks), dim3(256), 0, st, x, g, out, rows, C);
    } else {
      hipLaunchKernelGGL(k_rows_dot<T_>, dim3((unsigned)row_blocks(rows)), dim3(256), 0, st, x, g, out, rows, C);
    }
  });
}

int check_dtype_width(const char* who, const char* what, int dtype, int width) {
  if (dtype != DRIN_FEAT_F32 && dtype != DRIN_FEAT_BF16) {
    set_error("%s: %s = %d is neither DRIN_FEAT_F32 nor DRIN_FEAT_BF16", who, what, dtype);
    return DRIN_E_SHAPE;
  }
  const int v = dtype == DRIN_FEAT_BF16 ? 8 : 4;
  if (width <= 0 || width % v) {
    set_error("%s: width %d must be a positive multiple of %d (16-byte lane accesses of %s rows)", who, width, v,
              dtype == DRIN_FEAT_BF16 ? "bf16" : "fp32");
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

}  // namespace
}  // namespace drin

using namespace drin;

int drin_token_attribution(const void* tokens, int32_t token_dtype, const int64_t* mask, const int64_t* entity_index,
                           int64_t num_entities, int32_t* index_status, const float* grad_pooled, float* out, int64_t pairs,
                           int32_t T, int32_t width, void* stream) {
  const char* who = "drin_token_attribution";
  DRIN_CHECK_POINTERS(who, {"tokens", tokens, true}, {"grad_pooled", grad_pooled, true}, {"out", out, true});
  if (!mask) {
    set_error("%s: mask is NULL", who);
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(mask) & 7u) != 0 || (reinterpret_cast<uintptr_t>(entity_index) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(index_status) & 3u) != 0) {
    set_error("%s: mask and entity_index must be 8-byte and index_status 4-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_dtype_width(who, "token_dtype", token_dtype, width));
  DRIN_TRY(check_count(who, "T", T, 1, 1 << 24));
  DRIN_TRY(check_count(who, "pairs", pairs, 0, INT64_MAX / 4096));
  if (entity_index) DRIN_TRY(check_count(who, "num_entities (with entity_index)", num_entities, 1, INT64_MAX / 4096));
  if (pairs == 0) return DRIN_OK;
  DRIN_BIND_DEVICE(stream, out, who);
  if (token_dtype == DRIN_FEAT_BF16)
    return launch_token_attribution_t(static_cast<const __bf16*>(tokens), mask, entity_index, num_entities, index_status, grad_pooled,
                                      out, pairs, T, width, (hipStream_t)stream);
  return launch_token_attribution_t(static_cast<const float*>(tokens), mask, entity_index, num_entities, index_status, grad_pooled, out,
                                    pairs, T, width, (hipStream_t)stream);
}

int drin_rows_dot(const void* x, int32_t x_dtype, const float* g, float* out, int64_t rows, int32_t width, void* stream) {
  const char* who = "drin_rows_dot";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"g", g, true});
  if (!out) {
    set_error("%s: out is NULL", who);
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(out) & 3u) != 0) {
    set_error("%s: out must be 4-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_dtype_width(who, "x_dtype", x_dtype, width));
  DRIN_TRY(check_count(who, "rows", rows, 0, (int64_t)1 << 31));
  if (rows == 0) return DRIN_OK;
  DRIN_BIND_DEVICE(stream, out, who);
  if (x_dtype == DRIN_FEAT_BF16) return launch_rows_dot_t(static_cast<const __bf16*>(x), g, out, rows, width, (hipStream_t)stream);
  return launch_rows_dot_t(static_cast<const float*>(x), g, out, rows, width, (hipStream_t)stream);
}
