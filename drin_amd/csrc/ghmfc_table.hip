// The row kernels of GHMFC's table form: candidates are int64 rows of a device-resident entity table
// instead of gathered features - what baselines/data.py's qid2idx gather (data.py:87-93) and the entity half of
// baselines/ghmfc.py (:237-250, :297-298) do per mention on the host and per pair on the device.
//   k_gather_rows      out[i, :] = table[index[i], :]
//   k_cosine_gather    out[b, n] = cos(x[b, :], rows[index[b, n], :])
// and the entry points of the three indexed row operations (the indexed token mean is an instantiation of
// k_entity_token_mean, stream_kernels.hip).  Every index is clamped into [0, E - 1] BEFORE an address is formed from it and
// reported through report_bad_index (device_utils.h; drin_batch.index_status' semantics: sticky, NULL = clamp silently).
// No atomics beyond that error-path report, no scratch memory, 16-byte lane accesses: the same bits every run.
#include "device_utils.h"
#include "row_checks.h"

namespace drin {
namespace {

__device__ __forceinline__ int64_t clamp_row(int64_t raw, int64_t num_rows) { return raw < 0 ? 0 : (raw >= num_rows ? num_rows - 1 : raw); }

// One wave per output row, four rows per workgroup, the rest by grid stride; a lane copies float4 columns lane, lane + 64, ...
__global__ void __launch_bounds__(256) k_gather_rows(const float* __restrict__ table, const int64_t* __restrict__ index,
                                                     int64_t num_rows, float* __restrict__ out, int64_t count, int W4,
                                                     int32_t* status, int64_t pair_base) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < count; i += (int64_t)gridDim.x * 4) {
    const int64_t raw = index[i];
    const int64_t e = clamp_row(raw, num_rows);
    if (e != raw && lane == 0) report_bad_index(status, pair_base + i, raw);
    const float* src = table + e * (int64_t)W4 * 4;
    float* dst = out + i * (int64_t)W4 * 4;
    for (int c4 = lane; c4 < W4; c4 += 64) st4(dst + c4 * 4, ld4(src + c4 * 4));
  }
}

// k_cosine_rows (stream_kernels.hip) with y = a clamped row of a table: the same lane loop, wave sums and cosine_from_sums,
// so the bits of k_cosine_rows on the gathered rows (its scale is 1 there).  RowT: how the table rows are STORED - float, or
// __bf16 (8 bytes per lane and column quad, widened exactly by ld4: the same values in the same sums, so the bits of the float
// instantiation on the widened table).  x stays fp32.
template <typename RowT>
__global__ void __launch_bounds__(256) k_cosine_gather(const float* __restrict__ x, const RowT* __restrict__ rows,
                                                       const int64_t* __restrict__ index, int64_t num_rows, float* __restrict__ out,
                                                       int64_t pairs, int N, int D4, float eps, int32_t* status, int64_t pair_base) {
  int64_t p, b;
  if (!wave_pair(pairs, N, p, b)) return;
  const int lane = threadIdx.x & 63;
  const int64_t raw = index[p];
  const int64_t e = clamp_row(raw, num_rows);
  if (e != raw && lane == 0) report_bad_index(status, pair_base + p, raw);
  const float* xr = x + b * (int64_t)D4 * 4;
  const RowT* yr = rows + e * (int64_t)D4 * 4;
  float xy = 0.f, xx = 0.f, yy = 0.f;
  for (int c4 = lane; c4 < D4; c4 += 64) {
    const float4 a = ld4(xr + c4 * 4), b = ld4(yr + c4 * 4);
    xy += dot4(a, b);
    xx += dot4(a, a);
    yy += dot4(b, b);
  }
  xy = wave_sum(xy);
  xx = wave_sum(xx);
  yy = wave_sum(yy);
  if (lane == 0) out[p] = cosine_from_sums(xy, xx, yy, eps);
}

// what the three entry points share: the table, the index, the status words
int check_table_args(const char* who, const int64_t* index, int64_t num_rows, const int32_t* status) {
  if (!index) {
    set_error("%s: index is NULL", who);
    return DRIN_E_NULL;
  }
  if ((reinterpret_cast<uintptr_t>(index) & 7u) != 0 || (reinterpret_cast<uintptr_t>(status) & 3u) != 0) {
    set_error("%s: index must be 8-byte and index_status 4-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  return check_count(who, "num_entities", num_rows, 1, INT64_MAX / 4096);
}

}  // namespace

int launch_gather_rows(const float* table, const int64_t* index, int64_t num_rows, float* out, int64_t count, int width,
                       int32_t* status, int64_t pair_base, hipStream_t st) {
  if (count <= 0) return DRIN_OK;
  const int64_t blocks = row_blocks(count);
  return timed(DRIN_KC_POOL, st, "k_gather_rows", [&] {
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)blocks), dim3(256), 0, st, table, index, num_rows, out, count, width / 4, status,
                       pair_base);
  });
}

int launch_cosine_gather(const float* x, const void* rows, int row_dtype, const int64_t* index, int64_t num_rows, float* out, int B, int N,
                         int D, float eps, int32_t* status, int64_t pair_base, hipStream_t st) {
  const int64_t pairs = (int64_t)B * N;
  if (pairs <= 0) return DRIN_OK;
  if (row_dtype != DRIN_FEAT_BF16)
    return timed(DRIN_KC_EDGE, st, "k_cosine_gather", [&] {
      hipLaunchKernelGGL(k_cosine_gather<float>, pair_grid(B, N), dim3(256), 0, st, x, static_cast<const float*>(rows), index, num_rows, out,
                         pairs, N, D / 4, eps, status, pair_base);
    });
  return timed(DRIN_KC_EDGE, st, "k_cosine_gather_bf16", [&] {
    hipLaunchKernelGGL(k_cosine_gather<__bf16>, pair_grid(B, N), dim3(256), 0, st, x, static_cast<const __bf16*>(rows), index, num_rows, out,
                       pairs, N, D / 4, eps, status, pair_base);
  });
}

}  // namespace drin

using namespace drin;

int drin_gather_rows(const float* table, const int64_t* index, int64_t num_entities, float* out, int64_t count, int32_t width,
                     int32_t* index_status, void* stream) {
  const char* who = "drin_gather_rows";
  DRIN_CHECK_POINTERS(who, {"table", table, true}, {"out", out, true});
  DRIN_TRY(check_table_args(who, index, num_entities, index_status));
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "count", count, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_gather_rows(table, index, num_entities, out, count, width, index_status, 0, (hipStream_t)stream);
}

int drin_entity_token_mean_indexed(const float* text, const int64_t* mask, const int64_t* index, int64_t num_entities, float* out,
                                   int64_t pairs, int32_t tokens, int32_t width, int32_t* index_status, void* stream) {
  const char* who = "drin_entity_token_mean_indexed";
  DRIN_CHECK_POINTERS(who, {"text", text, true}, {"out", out, true});
  if (!mask) {
    set_error("%s: mask is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_table_args(who, index, num_entities, index_status));
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "pairs", pairs, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "tokens", tokens, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_entity_token_mean_indexed(text, mask, index, num_entities, out, pairs, tokens, width, index_status, 0,
                                          (hipStream_t)stream);
}

int drin_entity_token_pool_indexed(const float* text, const int64_t* mask, const int64_t* index, int64_t num_entities, float* out,
                                   int64_t pairs, int32_t tokens, int32_t width, int32_t pooling, int32_t* index_status, void* stream) {
  const char* who = "drin_entity_token_pool_indexed";
  DRIN_CHECK_POINTERS(who, {"text", text, true}, {"out", out, true});
  if (!mask) {
    set_error("%s: mask is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_table_args(who, index, num_entities, index_status));
  DRIN_TRY(check_entity_pooling(who, pooling));
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "pairs", pairs, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "tokens", tokens, 1, 512));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_entity_token_pool_indexed(text, mask, index, num_entities, out, pairs, tokens, width, pooling, index_status, 0,
                                          (hipStream_t)stream);
}

// the checks and the launch of both spellings: `who` names the one that was called
static int cosine_rows_indexed(const char* who, const float* x, const void* rows, int row_dtype, const int64_t* index, int64_t num_entities,
                               float* out, int32_t batch, int32_t num_candidates, int32_t width, float eps, int32_t* index_status,
                               void* stream) {
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"rows", rows, true});
  if (!out) {
    set_error("%s: out is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_table_args(who, index, num_entities, index_status));
  DRIN_TRY(check_row_dtype(who, row_dtype, width));
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "num_candidates", num_candidates, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "batch * num_candidates", (int64_t)batch * num_candidates, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_cosine_gather(x, rows, row_dtype, index, num_entities, out, batch, num_candidates, width, eps, index_status, 0,
                              (hipStream_t)stream);
}

int drin_cosine_rows_indexed_fwd(const float* x, const float* rows, const int64_t* index, int64_t num_entities, float* out,
                                 int32_t batch, int32_t num_candidates, int32_t width, float eps, int32_t* index_status, void* stream) {
  return cosine_rows_indexed("drin_cosine_rows_indexed_fwd", x, rows, DRIN_FEAT_F32, index, num_entities, out, batch, num_candidates, width,
                             eps, index_status, stream);
}

int drin_cosine_rows_indexed_fwd_ex(const float* x, const void* rows, int32_t row_dtype, const int64_t* index, int64_t num_entities,
                                    float* out, int32_t batch, int32_t num_candidates, int32_t width, float eps, int32_t* index_status,
                                    void* stream) {
  return cosine_rows_indexed("drin_cosine_rows_indexed_fwd_ex", x, rows, row_dtype, index, num_entities, out, batch, num_candidates, width,
                             eps, index_status, stream);
}
