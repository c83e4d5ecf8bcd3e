// The two CLIP edges of DRIN for candidates chosen at run time: for candidate rows index [B, N] of a table
//   miet[b, n] = scale * cos(m_clip_image[b, :], t_clip_text[index[b, n], :])
//   mtei[b, n] = scale * cos(m_clip_text[b, :],  t_clip_image[index[b, n], :])
// - what preprocess/clip.py:158-172 computes offline per pair as CLIPModel's logits_per_image / logits_per_text, exp(logit_scale) x
// the cosine of the projected embeddings (model.py:203 divides by that scale again).
//   k_cross_modal_edges<V, EDGES, RowT>   (RowT: the table rows as stored, float or __bf16 - drin_cross_modal_edges_ex, section 34)
//                                   a gather of EDGES table rows per pair, shaped for that: a wave takes `per_wave` CONSECUTIVE
//                                   candidates of ONE mention, 4 / EDGES of them per trip (four table rows in flight per wave);
//                                   it holds the mention's rows (V float4 slots per lane and row) and their squared norms in
//                                   registers across its candidates, reads its candidates' indices once, for both edges, and
//                                   issues every table-row load of a trip before the first of them is waited for
// Per pair the arithmetic is k_cosine_gather's (ghmfc_table.hip): the lane loop c4 = lane, lane + 64, ..., dot4, wave_sum,
// cosine_from_sums - so every output is, bit for bit, scale * what drin_cosine_rows_indexed_fwd returns for the same rows.
// An index outside [0, E - 1] is clamped BEFORE an address is formed from it and reported through report_bad_index.
// No atomics beyond that error-path report, no scratch memory, no LDS: the same bits every run.
#include "device_utils.h"
#include "row_checks.h"

namespace drin {
namespace {

// RowT: how the TABLE rows are stored - float, or __bf16 (an 8-byte lane load of four bf16, widened exactly
// by ld4, in the same column mapping - so the sums, their order and the bits are those of the float instantiation on the widened
// table).  The mention rows stay fp32.
template <typename RowT>
struct CrossEdgeArgs {
  const float* x[2];      // mention rows [B, D] of edge 0 / 1 (one edge alone: slot 0)
  const RowT* rows[2];    // table rows [E, D] of the same edge
  float* out[2];          // [B, N]
  const int64_t* index;   // [B, N]
  int64_t num_rows;
  int N, D4, per_wave;    // per_wave: candidates per wave, a multiple of the trip (4 / EDGES), at most 64
  float scale, eps;
  int32_t* status;
  int64_t pair_base;      // of mention 0 of this launch in the caller's index (the reported pair)
};

constexpr int kEdgeRowsInFlight = 4;   // table rows per wave and trip
constexpr int kEdgeMaxSlots = 2;       // V: widths up to 512 (the reference's CLIP) are held in registers; wider rows take V = 0

__device__ __forceinline__ int64_t readlane64(int64_t v, int src) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), src);
  return (int64_t)((uint64_t)hi << 32 | lo);
}

// V > 0: a row is V float4 slots per lane (D4 <= 64 V).  V = 0: any width - the mention rows are read again beside every trip's
// table rows, column slot by column slot (the same sums in the same order).  grid (ceil(N / (4 per_wave)), B).
template <int V, int EDGES, typename RowT>
__global__ void __launch_bounds__(256) k_cross_modal_edges(CrossEdgeArgs<RowT> a) {
  constexpr int K = kEdgeRowsInFlight / EDGES;   // candidates per trip
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t b = blockIdx.y;
  const int n0 = ((int)blockIdx.x * 4 + wave) * a.per_wave;
  if (n0 >= a.N) return;
  const int count = a.N - n0 < a.per_wave ? a.N - n0 : a.per_wave;
  const int64_t p0 = b * a.N + n0;
  const int D4 = a.D4;
  // the wave's candidates: lane i holds the clamped row of candidate n0 + i (one read of index per pair, for both edges)
  int64_t mine = 0;
  if (lane < count) {
    const int64_t raw = a.index[p0 + lane];
    mine = raw < 0 ? 0 : (raw >= a.num_rows ? a.num_rows - 1 : raw);
    if (mine != raw) report_bad_index(a.status, a.pair_base + p0 + lane, raw);
  }
  const float* xr[EDGES];
#pragma unroll
  for (int e = 0; e < EDGES; ++e) xr[e] = a.x[e] + b * (int64_t)D4 * 4;
  float4 xv[EDGES][V > 0 ? V : 1];
  float xx[EDGES];
  if constexpr (V > 0) {
#pragma unroll
    for (int e = 0; e < EDGES; ++e)
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int c4 = lane + 64 * v;
        xv[e][v] = c4 < D4 ? ld4(xr[e] + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
    for (int e = 0; e < EDGES; ++e) {
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v)
        if (lane + 64 * v < D4) s += dot4(xv[e][v], xv[e][v]);
      xx[e] = wave_sum(s);
    }
  }
  for (int t = 0; t < count; t += K) {
    const RowT* yr[K][EDGES];
    bool live[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      live[k] = t + k < count;                                        // wave-uniform
      const int64_t row = readlane64(mine, live[k] ? t + k : 0);
#pragma unroll
      for (int e = 0; e < EDGES; ++e) yr[k][e] = a.rows[e] + row * (int64_t)D4 * 4;
    }
    float xy[K][EDGES], yy[K][EDGES];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int e = 0; e < EDGES; ++e) xy[k][e] = 0.f, yy[k][e] = 0.f;
    if constexpr (V > 0) {
      float4 yv[K][EDGES][V];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int e = 0; e < EDGES; ++e)
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const int c4 = lane + 64 * v;
            yv[k][e][v] = (live[k] && c4 < D4) ? ld4(yr[k][e] + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int e = 0; e < EDGES; ++e)
#pragma unroll
          for (int v = 0; v < V; ++v)
            if (lane + 64 * v < D4) {
              xy[k][e] += dot4(xv[e][v], yv[k][e][v]);
              yy[k][e] += dot4(yv[k][e][v], yv[k][e][v]);
            }
    } else {
#pragma unroll
      for (int e = 0; e < EDGES; ++e) xx[e] = 0.f;
      for (int c4 = lane; c4 < D4; c4 += 64) {
        float4 xs[EDGES], ys[K][EDGES];
#pragma unroll
        for (int e = 0; e < EDGES; ++e) xs[e] = ld4(xr[e] + c4 * 4);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int e = 0; e < EDGES; ++e) ys[k][e] = live[k] ? ld4(yr[k][e] + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int e = 0; e < EDGES; ++e) xx[e] += dot4(xs[e], xs[e]);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int e = 0; e < EDGES; ++e) {
            xy[k][e] += dot4(xs[e], ys[k][e]);
            yy[k][e] += dot4(ys[k][e], ys[k][e]);
          }
      }
#pragma unroll
      for (int e = 0; e < EDGES; ++e) xx[e] = wave_sum(xx[e]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int e = 0; e < EDGES; ++e) {
        const float sxy = wave_sum(xy[k][e]), syy = wave_sum(yy[k][e]);
        if (live[k] && lane == 0) a.out[e][p0 + t + k] = a.scale * cosine_from_sums(sxy, xx[e], syy, a.eps);
      }
  }
}

template <int EDGES, typename RowT>
auto cross_edges_kernel(int D4) {
  const int slots = (D4 + 63) / 64;
  return slots <= 1 ? k_cross_modal_edges<1, EDGES, RowT>
                    : slots <= kEdgeMaxSlots ? k_cross_modal_edges<2, EDGES, RowT> : k_cross_modal_edges<0, EDGES, RowT>;
}

// Candidates per wave: as many trips as leave every CU its sixteen waves (a short call stays one trip per wave - the mention
// rows are then read once per trip from L2), at most four trips.  The bits do not depend on it.
int cross_edges_per_wave(int B, int N, int trip) {
  constexpr int64_t kWaves = 256 * 16;
  int per_wave = trip;
  while (per_wave < 4 * trip && (int64_t)B * cdiv(N, 2 * per_wave) >= kWaves) per_wave *= 2;
  return per_wave;
}

template <typename RowT>
int launch_cross_modal_edges_t(const float* m_image, const float* m_text, const RowT* t_text, const RowT* t_image, const int64_t* index,
                               int64_t num_rows, int B, int N, int D, float scale, float eps, float* miet, float* mtei, int32_t* status,
                               hipStream_t st) {
  if (B <= 0 || N <= 0) return DRIN_OK;
  CrossEdgeArgs<RowT> a = {};
  int edges = 0;
  if (miet != nullptr) a.x[edges] = m_image, a.rows[edges] = t_text, a.out[edges] = miet, ++edges;
  if (mtei != nullptr) a.x[edges] = m_text, a.rows[edges] = t_image, a.out[edges] = mtei, ++edges;
  if (edges == 0) return DRIN_OK;
  a.index = index, a.num_rows = num_rows, a.N = N, a.D4 = D / 4, a.scale = scale, a.eps = eps, a.status = status;
  a.per_wave = cross_edges_per_wave(B, N, kEdgeRowsInFlight / edges);
  auto kern = edges == 2 ? cross_edges_kernel<2, RowT>(a.D4) : cross_edges_kernel<1, RowT>(a.D4);
  const char* name = sizeof(RowT) == 2 ? "k_cross_modal_edges_bf16" : "k_cross_modal_edges";
  // (column groups of 4 waves, mention): B <= kMaxGridY is the entry point's bound, so one slice - the loop is the pair kernels'
  return for_grid_slices(B, [&](int64_t b0, int nb) -> int {
    CrossEdgeArgs<RowT> s = a;
    for (int e = 0; e < edges; ++e) s.x[e] += b0 * (int64_t)D, s.out[e] += b0 * (int64_t)N;
    s.index += b0 * (int64_t)N, s.pair_base = b0 * (int64_t)N;
    return timed(DRIN_KC_EDGE, st, name, [&] {
      hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(N, 4 * a.per_wave), (unsigned)nb), dim3(256), 0, st, s);
    });
  });
}

// row_dtype: how both tables are stored (DRIN_FEAT_F32 / DRIN_FEAT_BF16)
int launch_cross_modal_edges(const float* m_image, const float* m_text, const void* t_text, const void* t_image, int row_dtype,
                             const int64_t* index, int64_t num_rows, int B, int N, int D, float scale, float eps, float* miet, float* mtei,
                             int32_t* status, hipStream_t st) {
  if (row_dtype != DRIN_FEAT_BF16)
    return launch_cross_modal_edges_t(m_image, m_text, static_cast<const float*>(t_text), static_cast<const float*>(t_image), index, num_rows, B,
                                      N, D, scale, eps, miet, mtei, status, st);
  return launch_cross_modal_edges_t(m_image, m_text, static_cast<const __bf16*>(t_text), static_cast<const __bf16*>(t_image), index, num_rows, B,
                                    N, D, scale, eps, miet, mtei, status, st);
}

}  // namespace
}  // namespace drin

using namespace drin;

// the checks and the launch of both spellings: `who` names the one that was called
static int cross_modal_edges(const char* who, const float* mention_clip_image, const float* mention_clip_text, const void* table_clip_text,
                             const void* table_clip_image, int row_dtype, const int64_t* index, int64_t num_entities, int32_t batch,
                             int32_t num_candidates, int32_t width, float scale, float eps, float* miet, float* mtei, int32_t* index_status,
                             void* stream) {
  // an edge is its mention rows, its table rows and its output: all three, or none of them
  const bool has_miet = mention_clip_image || table_clip_text || miet, has_mtei = mention_clip_text || table_clip_image || mtei;
  if (!has_miet && !has_mtei) {
    set_error("%s: both edges are left out (every row pointer and both outputs are NULL)", who);
    return DRIN_E_NULL;
  }
  DRIN_CHECK_POINTERS(who, {"mention_clip_image", mention_clip_image, has_miet}, {"table_clip_text", table_clip_text, has_miet},
                      {"mention_clip_text", mention_clip_text, has_mtei}, {"table_clip_image", table_clip_image, has_mtei});
  if ((has_miet && !miet) || (has_mtei && !mtei)) {
    set_error("%s: %s is NULL while its edge's rows are given (an edge is left out with its three pointers NULL together)", who,
              has_miet && !miet ? "miet" : "mtei");
    return DRIN_E_NULL;
  }
  if (!index) {
    set_error("%s: index is NULL", who);
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(index) & 7u) != 0 || (reinterpret_cast<uintptr_t>(index_status) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(miet) & 3u) != 0 || (reinterpret_cast<uintptr_t>(mtei) & 3u) != 0) {
    set_error("%s: index must be 8-byte, index_status, miet and mtei 4-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_TRY(check_count(who, "num_entities", num_entities, 1, INT64_MAX / 4096));
  DRIN_TRY(check_row_dtype(who, row_dtype, width));
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "num_candidates", num_candidates, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "batch * num_candidates", (int64_t)batch * num_candidates, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, miet ? miet : mtei, who);
  return launch_cross_modal_edges(mention_clip_image, mention_clip_text, table_clip_text, table_clip_image, row_dtype, index, num_entities, batch,
                                  num_candidates, width, scale, eps, miet, mtei, index_status, (hipStream_t)stream);
}

int drin_cross_modal_edges(const float* mention_clip_image, const float* mention_clip_text, const float* table_clip_text,
                           const float* table_clip_image, const int64_t* index, int64_t num_entities, int32_t batch,
                           int32_t num_candidates, int32_t width, float scale, float eps, float* miet, float* mtei,
                           int32_t* index_status, void* stream) {
  return cross_modal_edges("drin_cross_modal_edges", mention_clip_image, mention_clip_text, table_clip_text, table_clip_image, DRIN_FEAT_F32,
                           index, num_entities, batch, num_candidates, width, scale, eps, miet, mtei, index_status, stream);
}

int drin_cross_modal_edges_ex(const float* mention_clip_image, const float* mention_clip_text, const void* table_clip_text,
                              const void* table_clip_image, int32_t row_dtype, const int64_t* index, int64_t num_entities, int32_t batch,
                              int32_t num_candidates, int32_t width, float scale, float eps, float* miet, float* mtei,
                              int32_t* index_status, void* stream) {
  return cross_modal_edges("drin_cross_modal_edges_ex", mention_clip_image, mention_clip_text, table_clip_text, table_clip_image, row_dtype,
                           index, num_entities, batch, num_candidates, width, scale, eps, miet, mtei, index_status, stream);
}
