// The mention representation head of DRIN's other text-vertex encoders (reference: baselines/ghmfc.py:54-70,152-199 under
// drin/model.py:21,58,71-76): with mention_final_layer_name "none" or "transformer" the mention-text
// vertex is repr(intermediate(mention_text)) with no Linear behind it and the text-text edge takes repr(mention_text) of the
// RAW block, repr being Avg.avg over the mention span ("avg extract") or the max over all L positions ("max pool").
// k_mention_rows writes both rows (and, for the max, the positions) in one launch; k_mention_rows_bwd writes every element of
// the two blocks' gradients once.  No atomics, no scratch memory, no memset-then-add: the same bits every run.
#include "device_utils.h"
#include "internal.h"
#include "row_checks.h"

namespace drin {
namespace {

constexpr int kReprAvg = DRIN_REPR_AVG_EXTRACT, kReprMax = DRIN_REPR_MAX_POOL;

// [lo, hi) = start : end as a Python slice of L positions clips it (k_span_mean's rules)
__device__ __forceinline__ void clip_span(int64_t s, int64_t e, int L, int& lo, int& hi) {
  if (s < 0) s = s + L < 0 ? 0 : s + L;
  if (e < 0) e = e + L < 0 ? 0 : e + L;
  if (e > L) e = L;
  if (s > L) s = L;
  lo = (int)s, hi = (int)e;
}

// repr of the float4 column of ONE block [L, D]: x points at (position 0, this thread's column quad), rows are D4 * 4 apart.
// Thread = (column quad, row group rg of four); the four groups meet in LDS and group 0 leaves with the result.
//   max: positions rg, rg + 4, ... of ALL L, k_seq_max<true>'s sequence of max_nan / max_nan_pos - its bits and positions
//   avg: positions lo + rg, lo + rg + 4, ... < hi summed, the four sums added as (0 + 1) + (2 + 3), divided by hi - lo
//        (an empty span: 0 / 0 = NaN, as torch.mean of an empty slice)
// Every thread of the workgroup calls it (two barriers inside); `live` = this thread's column exists.
template <int REPR, typename T>
__device__ __forceinline__ void block_repr(const T* __restrict__ x, bool live, int rg, int lane, int L, int D4, int lo, int hi,
                                           float4 (*part)[64], int4 (*part_i)[64], float4& val, int4& at) {
  if constexpr (REPR == kReprMax) {
    const float ninf = -__builtin_inff();
    float4 mx = make_float4(ninf, ninf, ninf, ninf);
    at = make_int4(rg, rg, rg, rg);   // (a row group past L keeps -inf here: it loses every tie against group 0's position)
    if (live)
      for (int s = rg; s < L; s += 4) {
        const float4 t = ld4(x + (int64_t)s * D4 * 4);
        at = make_int4(max_nan_pos(mx.x, at.x, t.x, s), max_nan_pos(mx.y, at.y, t.y, s), max_nan_pos(mx.z, at.z, t.z, s),
                       max_nan_pos(mx.w, at.w, t.w, s));
        mx = make_float4(max_nan(mx.x, t.x), max_nan(mx.y, t.y), max_nan(mx.z, t.z), max_nan(mx.w, t.w));
      }
    part[rg][lane] = mx;
    part_i[rg][lane] = at;
    __syncthreads();
    if (rg == 0) {
#pragma unroll
      for (int i = 1; i < 4; ++i) {
        const float4 t = part[i][lane];
        const int4 ti = part_i[i][lane];
        at = make_int4(max_nan_pos(mx.x, at.x, t.x, ti.x), max_nan_pos(mx.y, at.y, t.y, ti.y), max_nan_pos(mx.z, at.z, t.z, ti.z),
                       max_nan_pos(mx.w, at.w, t.w, ti.w));
        mx = make_float4(max_nan(mx.x, t.x), max_nan(mx.y, t.y), max_nan(mx.z, t.z), max_nan(mx.w, t.w));
      }
      val = mx;
    }
  } else {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
      for (int s = lo + rg; s < hi; s += 4) acc = acc + ld4(x + (int64_t)s * D4 * 4);
    part[rg][lane] = acc;
    __syncthreads();
    if (rg == 0) {
      acc = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      const float cnt = hi > lo ? (float)(hi - lo) : 0.0f;
      val = make_float4(acc.x / cnt, acc.y / cnt, acc.z / cnt, acc.w / cnt);
    }
  }
  __syncthreads();   // the next block of the same workgroup reuses `part`
}

// grid (cdiv(D4, 64), B).  edge_row[b] = repr(raw[b]); vertex_row[b] = repr(enc[b]) (ENC) or the edge row's values (the same
// function of the same block: nothing is read twice).  REPR max: idx_edge / idx_vertex [B, D] int32 take the positions.
template <typename T, int REPR, bool ENC>
__global__ void __launch_bounds__(256) k_mention_rows(const T* __restrict__ raw, const float* __restrict__ enc,
                                                      const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                      float* __restrict__ edge_row, float* __restrict__ vertex_row,
                                                      int* __restrict__ idx_edge, int* __restrict__ idx_vertex, int L, int D4) {
  __shared__ float4 part[4][64];
  __shared__ int4 part_i[REPR == kReprMax ? 4 : 1][64];
  const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c4 = blockIdx.x * 64 + lane;
  const int64_t b = blockIdx.y;
  const bool live = c4 < D4;
  int lo = 0, hi = L;
  if constexpr (REPR == kReprAvg) clip_span(start[b], end[b], L, lo, hi);
  const int64_t in_off = (b * L * D4 + c4) * 4, out_off = (b * D4 + c4) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  int4 at = make_int4(0, 0, 0, 0);
  block_repr<REPR, T>(raw + in_off, live, rg, lane, L, D4, lo, hi, part, part_i, v, at);
  if (rg == 0 && live) {
    st4(edge_row + out_off, v);
    if constexpr (REPR == kReprMax) *reinterpret_cast<int4*>(idx_edge + out_off) = at;
    if constexpr (!ENC) {
      st4(vertex_row + out_off, v);
      if constexpr (REPR == kReprMax) *reinterpret_cast<int4*>(idx_vertex + out_off) = at;
    }
  }
  if constexpr (ENC) {
    block_repr<REPR, float>(enc + in_off, live, rg, lane, L, D4, lo, hi, part, part_i, v, at);
    if (rg == 0 && live) {
      st4(vertex_row + out_off, v);
      if constexpr (REPR == kReprMax) *reinterpret_cast<int4*>(idx_vertex + out_off) = at;
    }
  }
}

// what position s of a block receives from the gradient g of its repr row: g / (hi - lo) inside the span, g at the maximum's
// position; exactly 0 elsewhere (g_len: g already divided by the span length)
template <int REPR>
__device__ __forceinline__ float4 repr_term(float4 g_len, int4 at, int s, int lo, int hi) {
  if constexpr (REPR == kReprMax)
    return make_float4(at.x == s ? g_len.x : 0.f, at.y == s ? g_len.y : 0.f, at.z == s ? g_len.z : 0.f, at.w == s ? g_len.w : 0.f);
  return s >= lo && s < hi ? g_len : make_float4(0.f, 0.f, 0.f, 0.f);
}

// grid (cdiv(D4, 64), B, row slices): thread = (column quad, row group); position s = 4 blockIdx.z + rg, step 4 gridDim.z.
// d_raw[b, s] = the edge row's term (+ the vertex row's term when BOTH: there is no encoded block, both rows are functions of
// the raw one - one write); d_enc[b, s] = the vertex row's term.  Every element of a non-NULL destination is written once.
// g_edge / g_vertex NULL: that row passes no gradient (zeros).
template <int REPR, bool BOTH>
__global__ void __launch_bounds__(256) k_mention_rows_bwd(const float* __restrict__ g_edge, const float* __restrict__ g_vertex,
                                                          const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                          const int* __restrict__ idx_edge, const int* __restrict__ idx_vertex,
                                                          float* __restrict__ d_raw, float* __restrict__ d_enc, int L, int D4) {
  const int c4 = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const int64_t b = blockIdx.y;
  if (c4 >= D4) return;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t row_off = (b * D4 + c4) * 4;
  float4 ge = g_edge ? ld4(g_edge + row_off) : zero, gv = g_vertex ? ld4(g_vertex + row_off) : zero;
  int4 ae = make_int4(-1, -1, -1, -1), av = ae;
  int lo = 0, hi = 0;
  if constexpr (REPR == kReprMax) {
    ae = *reinterpret_cast<const int4*>(idx_edge + row_off);
    av = *reinterpret_cast<const int4*>(idx_vertex + row_off);
  } else {
    clip_span(start[b], end[b], L, lo, hi);
    const float cnt = (float)(hi - lo);   // read inside the span only, where it is positive
    ge = make_float4(ge.x / cnt, ge.y / cnt, ge.z / cnt, ge.w / cnt);
    gv = make_float4(gv.x / cnt, gv.y / cnt, gv.z / cnt, gv.w / cnt);
  }
  for (int s = blockIdx.z * 4 + rg; s < L; s += 4 * gridDim.z) {
    const int64_t off = ((b * L + s) * D4 + c4) * 4;
    const float4 te = repr_term<REPR>(ge, ae, s, lo, hi), tv = repr_term<REPR>(gv, av, s, lo, hi);
    if (d_raw != nullptr) st4(d_raw + off, BOTH ? te + tv : te);
    if (d_enc != nullptr) st4(d_enc + off, tv);
  }
}

constexpr int kBwdRowSlices = 8;   // workgroups along L of k_mention_rows_bwd (a store-bound kernel: B x D / 256 alone is 192 at the reference shape)

template <typename T>
int launch_mention_rows_t(const T* raw, const float* enc, const int64_t* start, const int64_t* end, int repr, float* edge_row,
                          float* vertex_row, int* idx_edge, int* idx_vertex, int B, int L, int D, hipStream_t st) {
  const int D4 = D / 4;
  return for_grid_slices(B, [&](int64_t b0, int nb) -> int {
    const dim3 grid((unsigned)cdiv(D4, 64), (unsigned)nb), block(256);
    const int64_t in = b0 * L * D, out = b0 * D;
    const T* r = raw + in;
    const float* e = enc ? enc + in : nullptr;
    const int64_t *s = start ? start + b0 : nullptr, *t = end ? end + b0 : nullptr;
    int *ie = idx_edge ? idx_edge + out : nullptr, *iv = idx_vertex ? idx_vertex + out : nullptr;
    return timed(DRIN_KC_POOL, st, "k_mention_rows", [&] {
      if (repr == kReprMax) {
        if (enc)
          hipLaunchKernelGGL((k_mention_rows<T, kReprMax, true>), grid, block, 0, st, r, e, s, t, edge_row + out, vertex_row + out, ie, iv, L, D4);
        else
          hipLaunchKernelGGL((k_mention_rows<T, kReprMax, false>), grid, block, 0, st, r, e, s, t, edge_row + out, vertex_row + out, ie, iv, L, D4);
      } else {
        if (enc)
          hipLaunchKernelGGL((k_mention_rows<T, kReprAvg, true>), grid, block, 0, st, r, e, s, t, edge_row + out, vertex_row + out, ie, iv, L, D4);
        else
          hipLaunchKernelGGL((k_mention_rows<T, kReprAvg, false>), grid, block, 0, st, r, e, s, t, edge_row + out, vertex_row + out, ie, iv, L, D4);
      }
    });
  });
}

}  // namespace

int launch_mention_rows(const void* raw, bool raw_bf16, const float* enc, const int64_t* start, const int64_t* end, int repr,
                        float* edge_row, float* vertex_row, int* idx_edge, int* idx_vertex, int B, int L, int D, hipStream_t st) {
  if (B <= 0) return DRIN_OK;
  if (raw_bf16)
    return launch_mention_rows_t<__bf16>(static_cast<const __bf16*>(raw), enc, start, end, repr, edge_row, vertex_row, idx_edge,
                                         idx_vertex, B, L, D, st);
  return launch_mention_rows_t<float>(static_cast<const float*>(raw), enc, start, end, repr, edge_row, vertex_row, idx_edge, idx_vertex,
                                      B, L, D, st);
}

int launch_mention_rows_bwd(const float* g_edge, const float* g_vertex, const int64_t* start, const int64_t* end, const int* idx_edge,
                            const int* idx_vertex, int repr, bool has_encoded, float* d_raw, float* d_enc, int B, int L, int D,
                            hipStream_t st) {
  if (B <= 0 || (d_raw == nullptr && d_enc == nullptr)) return DRIN_OK;
  const int D4 = D / 4;
  const unsigned slices = (unsigned)(cdiv(L, 4) < kBwdRowSlices ? cdiv(L, 4) : kBwdRowSlices);
  return for_grid_slices(B, [&](int64_t b0, int nb) -> int {
    const dim3 grid((unsigned)cdiv(D4, 64), (unsigned)nb, slices), block(256);
    const int64_t blk = b0 * L * D, row = b0 * D;
    const float *ge = g_edge ? g_edge + row : nullptr, *gv = g_vertex ? g_vertex + row : nullptr;
    const int64_t *s = start ? start + b0 : nullptr, *t = end ? end + b0 : nullptr;
    const int *ie = idx_edge ? idx_edge + row : nullptr, *iv = idx_vertex ? idx_vertex + row : nullptr;
    float *dr = d_raw ? d_raw + blk : nullptr, *de = d_enc ? d_enc + blk : nullptr;
    return timed(DRIN_KC_POOL, st, "k_mention_rows_bwd", [&] {
      if (repr == kReprMax) {
        if (has_encoded)
          hipLaunchKernelGGL((k_mention_rows_bwd<kReprMax, false>), grid, block, 0, st, ge, gv, s, t, ie, iv, dr, de, L, D4);
        else
          hipLaunchKernelGGL((k_mention_rows_bwd<kReprMax, true>), grid, block, 0, st, ge, gv, s, t, ie, iv, dr, de, L, D4);
      } else {
        if (has_encoded)
          hipLaunchKernelGGL((k_mention_rows_bwd<kReprAvg, false>), grid, block, 0, st, ge, gv, s, t, ie, iv, dr, de, L, D4);
        else
          hipLaunchKernelGGL((k_mention_rows_bwd<kReprAvg, true>), grid, block, 0, st, ge, gv, s, t, ie, iv, dr, de, L, D4);
      }
    });
  });
}

}  // namespace drin

using namespace drin;

// ---- the two kernels as entry points of their own ------------------------------------------------------
namespace {
int mention_rows_args(const char* who, int32_t representation, const int64_t* start, const int64_t* end, const int32_t* max_index,
                      int32_t batch, int32_t seq_len, int32_t width) {
  if (representation != DRIN_REPR_AVG_EXTRACT && representation != DRIN_REPR_MAX_POOL) {
    set_error("%s: representation = %d is neither DRIN_REPR_AVG_EXTRACT (%d) nor DRIN_REPR_MAX_POOL (%d)", who, representation,
              DRIN_REPR_AVG_EXTRACT, DRIN_REPR_MAX_POOL);
    return DRIN_E_SHAPE;
  }
  if (representation == DRIN_REPR_AVG_EXTRACT && (!start || !end)) {
    set_error("%s: start / end is NULL (the span of DRIN_REPR_AVG_EXTRACT)", who);
    return DRIN_E_NULL;
  }
  DRIN_CHECK_POINTERS(who, {"max_index", max_index, representation == DRIN_REPR_MAX_POOL});
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  return check_count(who, "seq_len", seq_len, 1, INT32_MAX);
}
}  // namespace

int drin_mention_rows_fwd(const void* raw, int32_t raw_dtype, const float* encoded, const int64_t* start, const int64_t* end,
                          int32_t representation, float* edge_row, float* vertex_row, int32_t* max_index, int32_t batch,
                          int32_t seq_len, int32_t width, void* stream) {
  const char* who = "drin_mention_rows_fwd";
  DRIN_CHECK_POINTERS(who, {"raw", raw, true}, {"encoded", encoded, false}, {"edge_row", edge_row, true},
                      {"vertex_row", vertex_row, true});
  if (raw_dtype != DRIN_FEAT_F32 && raw_dtype != DRIN_FEAT_BF16) {
    set_error("%s: raw_dtype = %d is neither DRIN_FEAT_F32 nor DRIN_FEAT_BF16", who, raw_dtype);
    return DRIN_E_SHAPE;
  }
  DRIN_TRY(mention_rows_args(who, representation, start, end, max_index, batch, seq_len, width));
  DRIN_BIND_DEVICE(stream, edge_row, who);
  const bool mx = representation == DRIN_REPR_MAX_POOL;
  return launch_mention_rows(raw, raw_dtype == DRIN_FEAT_BF16, encoded, start, end, representation, edge_row, vertex_row,
                             mx ? max_index : nullptr, mx ? max_index + (size_t)batch * width : nullptr, batch, seq_len, width,
                             (hipStream_t)stream);
}

int drin_mention_rows_bwd(const float* g_edge_row, const float* g_vertex_row, const int64_t* start, const int64_t* end,
                          const int32_t* max_index, int32_t representation, int32_t has_encoded, float* grad_raw, float* grad_encoded,
                          int32_t batch, int32_t seq_len, int32_t width, void* stream) {
  const char* who = "drin_mention_rows_bwd";
  DRIN_CHECK_POINTERS(who, {"g_edge_row", g_edge_row, false}, {"g_vertex_row", g_vertex_row, false}, {"grad_raw", grad_raw, false},
                      {"grad_encoded", grad_encoded, false});
  DRIN_TRY(mention_rows_args(who, representation, start, end, max_index, batch, seq_len, width));
  if (!has_encoded && grad_encoded) {
    set_error("%s: grad_encoded without an encoded block (has_encoded = 0: both rows are functions of the raw block)", who);
    return DRIN_E_SHAPE;
  }
  if (!grad_raw && !grad_encoded) return DRIN_OK;
  DRIN_BIND_DEVICE(stream, grad_raw ? grad_raw : grad_encoded, who);
  const bool mx = representation == DRIN_REPR_MAX_POOL;
  return launch_mention_rows_bwd(g_edge_row, g_vertex_row, start, end, mx ? max_index : nullptr,
                                 mx ? max_index + (size_t)batch * width : nullptr, representation, has_encoded != 0, grad_raw,
                                 grad_encoded, batch, seq_len, width, (hipStream_t)stream);
}
