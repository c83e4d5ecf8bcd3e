// The row operations of the GHMFC baseline (reference: baselines/ghmfc.py), forward and backward (DESIGN.md sections 15, 18,
// 20): LayerNorm with a fused residual, the max over a sequence, the gated mix, activation + dropout - kernels, launchers
// and the per-operation entry points with their argument checks (the cosine, the entity token mean and the span mean
// launch kernels of stream_kernels.hip / backward_kernels.hip).
// No atomics (column sums go through per-workgroup partial rows added in a fixed order), no scratch memory: the same bits
// every run.
#include "attention_common.h"
#include "device_utils.h"
#include "row_checks.h"
#include "row_ops.h"

namespace drin {
namespace {

// ---- y = LayerNorm(x [+ res]) (ghmfc.py:121-127), one wave per row, the row in registers (row_ops.h) -------------------
// y may be x or res: a wave holds its whole row before it stores.  mean_out / rstd_out [rows] (both or neither): the row
// statistics the backward recomputes xhat from (drin_layernorm_res_train_fwd); NULL in the scoring pass.
template <int DV>
__global__ void __launch_bounds__(256) k_layernorm_res(const float* x, const float* res, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* y, float* __restrict__ mean_out,
                                                       float* __restrict__ rstd_out, int64_t rows, int E4, float eps) {
  const int lane = threadIdx.x & 63;
  const float inv_e = 1.0f / (float)(E4 * 4);
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    Row<DV> h = load_row<DV>(x + row * E4 * 4, lane, E4);
    if (res != nullptr) {
      const Row<DV> r = load_row<DV>(res + row * E4 * 4, lane, E4);
#pragma unroll
      for (int jj = 0; jj < DV; ++jj) h.v[jj] = h.v[jj] + r.v[jj];
    }
    float s = 0.f;
#pragma unroll
    for (int jj = 0; jj < DV; ++jj) s += (h.v[jj].x + h.v[jj].y) + (h.v[jj].z + h.v[jj].w);
    const float mu = wave_sum(s) * inv_e;
    float qv = 0.f;
#pragma unroll
    for (int jj = 0; jj < DV; ++jj)
      if (lane + 64 * jj < E4) {
        const float dx = h.v[jj].x - mu, dy = h.v[jj].y - mu, dz = h.v[jj].z - mu, dw = h.v[jj].w - mu;
        qv += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      }
    const float rstd = 1.0f / sqrtf(wave_sum(qv) * inv_e + eps);
    if (mean_out != nullptr && lane == 0) mean_out[row] = mu, rstd_out[row] = rstd;
#pragma unroll
    for (int jj = 0; jj < DV; ++jj) {
      const int c4 = lane + 64 * jj;
      if (c4 < E4) {
        const float4 gm = ld4(gamma + c4 * 4), bt = ld4(beta + c4 * 4);
        h.v[jj] = make_float4(fmaf((h.v[jj].x - mu) * rstd, gm.x, bt.x), fmaf((h.v[jj].y - mu) * rstd, gm.y, bt.y),
                              fmaf((h.v[jj].z - mu) * rstd, gm.z, bt.z), fmaf((h.v[jj].w - mu) * rstd, gm.w, bt.w));
      }
    }
    store_row<DV>(y + row * E4 * 4, h, lane, E4);
  }
}

// ---- out[b, :] = max over ALL s of x[b, s, :] (ghmfc.py:143,145: padded positions take part; a NaN wins, as torch.max) ----
// grid (cdiv(E4, 64), B): thread (column quad, row group of four), the four groups meet in LDS.
// (max_nan / max_nan_pos: device_utils.h - k_mention_rows of mention_rows.hip runs the same sequence)
template <bool IDX>
__global__ void __launch_bounds__(256) k_seq_max(const float* __restrict__ x, float* __restrict__ out, int* __restrict__ idx, int S,
                                                 int E4) {
  __shared__ float4 part[4][64];
  __shared__ int4 part_i[IDX ? 4 : 1][64];
  const int c4 = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const int64_t b = blockIdx.y;
  const float ninf = -__builtin_inff();
  float4 mx = make_float4(ninf, ninf, ninf, ninf);
  int4 at = make_int4(rg, rg, rg, rg);   // (a row group past S keeps -inf here: it loses every tie against group 0's position)
  if (c4 < E4)
    for (int s = rg; s < S; s += 4) {
      const float4 t = ld4(x + ((b * S + s) * E4 + c4) * 4);
      if constexpr (IDX)
        at = make_int4(max_nan_pos(mx.x, at.x, t.x, s), max_nan_pos(mx.y, at.y, t.y, s), max_nan_pos(mx.z, at.z, t.z, s),
                       max_nan_pos(mx.w, at.w, t.w, s));
      mx = make_float4(max_nan(mx.x, t.x), max_nan(mx.y, t.y), max_nan(mx.z, t.z), max_nan(mx.w, t.w));
    }
  part[rg][threadIdx.x & 63] = mx;
  if constexpr (IDX) part_i[rg][threadIdx.x & 63] = at;
  __syncthreads();
  if (rg != 0 || c4 >= E4) return;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const float4 t = part[i][threadIdx.x];
    if constexpr (IDX) {
      const int4 ti = part_i[i][threadIdx.x];
      at = make_int4(max_nan_pos(mx.x, at.x, t.x, ti.x), max_nan_pos(mx.y, at.y, t.y, ti.y), max_nan_pos(mx.z, at.z, t.z, ti.z),
                     max_nan_pos(mx.w, at.w, t.w, ti.w));
    }
    mx = make_float4(max_nan(mx.x, t.x), max_nan(mx.y, t.y), max_nan(mx.z, t.z), max_nan(mx.w, t.w));
  }
  st4(out + (b * E4 + c4) * 4, mx);
  if constexpr (IDX) *reinterpret_cast<int4*>(idx + (b * E4 + c4) * 4) = at;
}

// dx[b, s, c] = dout[b, c] where s == idx[b, c], else 0: every element of dx is written.  Same grid as k_seq_max.
__global__ void __launch_bounds__(256) k_seq_max_bwd(const float* __restrict__ dout, const int* __restrict__ idx, float* __restrict__ dx,
                                                     int S, int E4) {
  const int c4 = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const int64_t b = blockIdx.y;
  if (c4 >= E4) return;
  const float4 g = ld4(dout + (b * E4 + c4) * 4);
  const int4 at = *reinterpret_cast<const int4*>(idx + (b * E4 + c4) * 4);
  for (int s = rg; s < S; s += 4)
    st4(dx + ((b * S + s) * E4 + c4) * 4,
        make_float4(at.x == s ? g.x : 0.f, at.y == s ? g.y : 0.f, at.z == s ? g.z : 0.f, at.w == s ? g.w : 0.f));
}

// ---- the gate (ghmfc.py:144-149): t = gelu(tl), v = gelu(vl), s = softmax(score_linear([t | v])), out = s0 t + s1 v ----------
// One wave per mention; tl / vl are the outputs of text_linear / image_linear, ws [2, 2 D] and bs [2] the score Linear.
__global__ void __launch_bounds__(256) k_gate_mix(const float* __restrict__ tl, const float* __restrict__ vl, const float* __restrict__ ws,
                                                  const float* __restrict__ bs, float* __restrict__ out, int B, int D4) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int64_t D = (int64_t)D4 * 4;
  auto gelu4 = [](float4 a) { return make_float4(gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w)); };
  float z0 = 0.f, z1 = 0.f;
  for (int c4 = lane; c4 < D4; c4 += 64) {
    const float4 t = gelu4(ld4(tl + b * D + c4 * 4)), v = gelu4(ld4(vl + b * D + c4 * 4));
    z0 += dot4(t, ld4(ws + c4 * 4)) + dot4(v, ld4(ws + D + c4 * 4));
    z1 += dot4(t, ld4(ws + 2 * D + c4 * 4)) + dot4(v, ld4(ws + 3 * D + c4 * 4));
  }
  z0 = wave_sum(z0) + bs[0];
  z1 = wave_sum(z1) + bs[1];
  const float zm = fmaxf(z0, z1);
  const float e0 = expf(z0 - zm), e1 = expf(z1 - zm);
  const float s0 = e0 / (e0 + e1), s1 = e1 / (e0 + e1);
  for (int c4 = lane; c4 < D4; c4 += 64) {
    const float4 t = gelu4(ld4(tl + b * D + c4 * 4)), v = gelu4(ld4(vl + b * D + c4 * 4));
    st4(out + b * D + c4 * 4, fma4(s0, t, v * s1));
  }
}

// ---- backward of the row kernels (what autograd runs for ghmfc.py:121-127, :143-149 under train.py:33-34) -----------------
// Column sums over rows (dgamma, dbeta, the score Linear's gradient) are reduced in two ordered levels, no atomics: every
// workgroup stores ONE row of partial sums into the caller's scratch, a second kernel adds the rows of a column in a fixed
// order.  At most kRowBwdBlocks workgroups per launch: a grid-stride loop deals the rows.
constexpr int kRowBwdBlocks = 256;
__device__ __forceinline__ float sum_block_rows(const float* __restrict__ p, int blocks, int64_t ld) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int b = 0;
  for (; b + 4 <= blocks; b += 4) s0 += p[b * ld], s1 += p[(b + 1) * ld], s2 += p[(b + 2) * ld], s3 += p[(b + 3) * ld];
  for (; b < blocks; ++b) s0 += p[b * ld];
  return (s0 + s1) + (s2 + s3);
}
// the four waves' Row<DV> of column sums -> one row `dst` (E4 float4 columns); comb: [4][DV][64]
template <int DV>
__device__ __forceinline__ void block_row_sum(const Row<DV>& a, float4 (*comb)[DV][64], float* __restrict__ dst, int wave, int lane,
                                              int E4) {
  __syncthreads();
#pragma unroll
  for (int j = 0; j < DV; ++j) comb[wave][j][lane] = a.v[j];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int j = 0; j < DV; ++j) {
      const int c4 = lane + 64 * j;
      if (c4 < E4) st4(dst + c4 * 4, (comb[0][j][lane] + comb[1][j][lane]) + (comb[2][j][lane] + comb[3][j][lane]));
    }
  }
}

// y = LN(x [+ res]) backward: with xhat = (x [+ res] - mean) rstd recomputed and g = dy gamma,
//   dh = rstd (g - mean_c(g) - xhat mean_c(g xhat))            the gradient of the pre-norm sum: dx and dres both
//   dgamma = sum_rows dy xhat,  dbeta = sum_rows dy             (SUMS; partial: [gridDim.x][2][E])
// One wave per row, the row in registers like the forward.  dh may be dy.
template <int DV, bool SUMS>
__global__ void __launch_bounds__(256) k_layernorm_res_bwd(const float* __restrict__ x, const float* __restrict__ res,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* dy, float* dh,
                                                           float* __restrict__ partial, int64_t rows, int E4) {
  __shared__ float4 comb[SUMS ? 4 : 1][DV][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float inv_e = 1.0f / (float)(E4 * 4);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  Row<DV> a_dg = zero_row<DV>(), a_db = zero_row<DV>();
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    Row<DV> h = load_row<DV>(x + row * E4 * 4, lane, E4);
    if (res != nullptr) {
      const Row<DV> r = load_row<DV>(res + row * E4 * 4, lane, E4);
#pragma unroll
      for (int jj = 0; jj < DV; ++jj) h.v[jj] = h.v[jj] + r.v[jj];
    }
    Row<DV> g = load_row<DV>(dy + row * E4 * 4, lane, E4);
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int jj = 0; jj < DV; ++jj) {
      const int c4 = lane + 64 * jj;
      if (c4 < E4) {
        const float4 gm = ld4(gamma + c4 * 4);
        const float4 xh = make_float4((h.v[jj].x - mu) * rs, (h.v[jj].y - mu) * rs, (h.v[jj].z - mu) * rs, (h.v[jj].w - mu) * rs);
        const float4 d = g.v[jj];
        if constexpr (SUMS) {
          a_dg.v[jj] = make_float4(fmaf(d.x, xh.x, a_dg.v[jj].x), fmaf(d.y, xh.y, a_dg.v[jj].y), fmaf(d.z, xh.z, a_dg.v[jj].z),
                                   fmaf(d.w, xh.w, a_dg.v[jj].w));
          a_db.v[jj] = a_db.v[jj] + d;
        }
        const float4 gg = make_float4(d.x * gm.x, d.y * gm.y, d.z * gm.z, d.w * gm.w);
        s1 += (gg.x + gg.y) + (gg.z + gg.w);
        s2 += dot4(gg, xh);
        h.v[jj] = xh, g.v[jj] = gg;
      } else {
        h.v[jj] = zero;
      }
    }
    s1 = wave_sum(s1) * inv_e;
    s2 = wave_sum(s2) * inv_e;
#pragma unroll
    for (int jj = 0; jj < DV; ++jj)
      g.v[jj] = make_float4(rs * fmaf(-h.v[jj].x, s2, g.v[jj].x - s1), rs * fmaf(-h.v[jj].y, s2, g.v[jj].y - s1),
                            rs * fmaf(-h.v[jj].z, s2, g.v[jj].z - s1), rs * fmaf(-h.v[jj].w, s2, g.v[jj].w - s1));
    store_row<DV>(dh + row * E4 * 4, g, lane, E4);
  }
  if constexpr (SUMS) {
    float* dst = partial + (int64_t)blockIdx.x * 2 * E4 * 4;
    block_row_sum<DV>(a_dg, comb, dst, wave, lane, E4);
    block_row_sum<DV>(a_db, comb, dst + E4 * 4, wave, lane, E4);
  }
}
// dgamma[c] / dbeta[c] = the sum over the workgroups' rows of partial [blocks][2][E], in order; either may be NULL
__global__ void __launch_bounds__(256) k_layernorm_res_bwd_sums(const float* __restrict__ partial, int blocks, int E,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * E) return;
  float* dst = c < E ? dgamma : dbeta;
  if (dst == nullptr) return;
  dst[c < E ? c : c - E] = sum_block_rows(partial + c, blocks, 2 * (int64_t)E);
}

// d gelu_erf / dx = Phi(x) + x phi(x) with the library erff / expf (the forward's gelu_erf is the exact-erf form too)
__device__ __forceinline__ float gelu_erf_grad_exact(float x) {
  return fmaf(x * 0.39894228040143267794f, expf(-0.5f * x * x), 0.5f * (1.0f + erff(x * 0.70710678118654752440f)));
}
// The gate's backward (ghmfc.py:144-149), one wave per mention; t, v, z, s recomputed with the forward's expressions (the
// second pass over tl / vl / dout hits the cache; only the column sums live in registers across mentions).  With a = sum_c dout_c (t_c - v_c): dz0 = s0 s1 a = -dz1,
//   dt = s0 dout + dz0 ws[0, :D] + dz1 ws[1, :D],  dv = s1 dout + dz0 ws[0, D:] + dz1 ws[1, D:],  dtl = dt gelu'(tl),  dvl = dv gelu'(vl)
// SUMS: the workgroup's sums over its mentions of dz0 t | dz0 v | dz0 -> partial [gridDim.x][2 D + 4]; row 1 of dws and
// dbs[1] are their negatives (dz1 = -dz0 exactly).
template <int DV, bool SUMS>
__global__ void __launch_bounds__(256) k_gate_mix_bwd(const float* __restrict__ tl, const float* __restrict__ vl,
                                                      const float* __restrict__ ws, const float* __restrict__ bs,
                                                      const float* __restrict__ dout, float* __restrict__ dtl, float* __restrict__ dvl,
                                                      float* __restrict__ partial, int B, int D4) {
  __shared__ float4 comb[SUMS ? 4 : 1][DV][64];
  __shared__ float dzs[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t D = (int64_t)D4 * 4;
  auto gelu4 = [](float4 a) { return make_float4(gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w)); };
  auto grad4 = [](float4 a) {
    return make_float4(gelu_erf_grad_exact(a.x), gelu_erf_grad_exact(a.y), gelu_erf_grad_exact(a.z), gelu_erf_grad_exact(a.w));
  };
  Row<DV> a_t = zero_row<DV>(), a_v = zero_row<DV>();
  float a_z = 0.f;
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
    float z0 = 0.f, z1 = 0.f, a = 0.f;
#pragma unroll
    for (int jj = 0; jj < DV; ++jj) {
      const int c4 = lane + 64 * jj;
      if (c4 < D4) {
        const float4 t = gelu4(ld4(tl + b * D + c4 * 4)), v = gelu4(ld4(vl + b * D + c4 * 4)), g = ld4(dout + b * D + c4 * 4);
        z0 += dot4(t, ld4(ws + c4 * 4)) + dot4(v, ld4(ws + D + c4 * 4));
        z1 += dot4(t, ld4(ws + 2 * D + c4 * 4)) + dot4(v, ld4(ws + 3 * D + c4 * 4));
        a += dot4(g, make_float4(t.x - v.x, t.y - v.y, t.z - v.z, t.w - v.w));
      }
    }
    z0 = wave_sum(z0) + bs[0];
    z1 = wave_sum(z1) + bs[1];
    a = wave_sum(a);
    const float zm = fmaxf(z0, z1);
    const float e0 = expf(z0 - zm), e1 = expf(z1 - zm);
    const float s0 = e0 / (e0 + e1), s1 = e1 / (e0 + e1);
    const float dz0 = s0 * s1 * a, dz1 = -dz0;
    a_z += dz0;
#pragma unroll
    for (int jj = 0; jj < DV; ++jj) {
      const int c4 = lane + 64 * jj;
      if (c4 < D4) {
        const float4 g = ld4(dout + b * D + c4 * 4), xt = ld4(tl + b * D + c4 * 4), xv = ld4(vl + b * D + c4 * 4);
        const float4 dt = fma4(dz0, ld4(ws + c4 * 4), fma4(dz1, ld4(ws + 2 * D + c4 * 4), g * s0));
        const float4 dv = fma4(dz0, ld4(ws + D + c4 * 4), fma4(dz1, ld4(ws + 3 * D + c4 * 4), g * s1));
        const float4 gt = grad4(xt), gv = grad4(xv);
        st4(dtl + b * D + c4 * 4, make_float4(dt.x * gt.x, dt.y * gt.y, dt.z * gt.z, dt.w * gt.w));
        st4(dvl + b * D + c4 * 4, make_float4(dv.x * gv.x, dv.y * gv.y, dv.z * gv.z, dv.w * gv.w));
        if constexpr (SUMS) {
          a_t.v[jj] = fma4(dz0, gelu4(xt), a_t.v[jj]);
          a_v.v[jj] = fma4(dz0, gelu4(xv), a_v.v[jj]);
        }
      }
    }
  }
  if constexpr (SUMS) {
    float* dst = partial + (int64_t)blockIdx.x * (2 * D + 4);
    block_row_sum<DV>(a_t, comb, dst, wave, lane, D4);
    block_row_sum<DV>(a_v, comb, dst + D, wave, lane, D4);
    if (lane == 0) dzs[wave] = a_z;
    __syncthreads();
    if (threadIdx.x == 0) dst[2 * D] = (dzs[0] + dzs[1]) + (dzs[2] + dzs[3]);
  }
}
// dws [2, 2 D] and dbs [2] from partial [blocks][2 D + 4], in order; either may be NULL
__global__ void __launch_bounds__(256) k_gate_mix_bwd_sums(const float* __restrict__ partial, int blocks, int D2,
                                                           float* __restrict__ dws, float* __restrict__ dbs) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > D2) return;
  float* dst = c < D2 ? dws : dbs;
  if (dst == nullptr) return;
  const float s = sum_block_rows(partial + c, blocks, (int64_t)D2 + 4);
  if (c < D2)
    dws[c] = s, dws[D2 + c] = -s;
  else
    dbs[0] = s, dbs[1] = -s;
}

// ---- y = act(x) m / (1 - p): the FFN activation and the dropouts of nn.TransformerEncoderLayer (ghmfc.py:75-86) -----------
// Element-wise over [rows, width] contiguous floats, width % 4 == 0: thread = one float4, i.e. the elements 4 i .. 4 i + 3 of
// the flat index e = row * width + col - exactly one Philox evaluation of dropout_mask.h, whose mask this is with the
// geometry (B, H, Lq, Lk) = (rows, 1, 1, width).  A dropped element is exactly 0 (a select, not a product: a dropped NaN
// goes too); DROP = false has no generator code.  relu and relu' are torch's (a NaN passes; relu'(0) = 0); gelu and gelu'
// are the gate's expressions.  y may be x and dx may be dy (no __restrict__ on them).  At most kActBlocks workgroups, the
// rest by grid stride.
constexpr int kActNone = DRIN_ROW_ACT_NONE, kActRelu = DRIN_ROW_ACT_RELU, kActGelu = DRIN_ROW_ACT_GELU;
constexpr int kActBlocks = 2048;
template <int ACT>
__device__ __forceinline__ float row_act(float x) {
  if constexpr (ACT == kActRelu) return x <= 0.f ? 0.f : x;
  if constexpr (ACT == kActGelu) return gelu_erf(x);
  return x;
}
// g act'(x)
template <int ACT>
__device__ __forceinline__ float row_act_bwd(float x, float g) {
  if constexpr (ACT == kActRelu) return x <= 0.f ? 0.f : g;
  if constexpr (ACT == kActGelu) return g * gelu_erf_grad_exact(x);
  return g;
}
__device__ __forceinline__ float4 drop4(float4 v, int64_t quad, const DropArgs& d) {
  const Philox4 r = philox4x32_10(d.seed, d.call, (uint64_t)quad);
  return make_float4(r.w[0] >= d.threshold ? v.x * d.scale : 0.f, r.w[1] >= d.threshold ? v.y * d.scale : 0.f,
                     r.w[2] >= d.threshold ? v.z * d.scale : 0.f, r.w[3] >= d.threshold ? v.w * d.scale : 0.f);
}
template <int ACT, bool DROP>
__global__ void __launch_bounds__(256) k_act_dropout(const float* x, float* y, int64_t n4, DropArgs drop) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 a = ld4(x + i * 4);
    float4 v = make_float4(row_act<ACT>(a.x), row_act<ACT>(a.y), row_act<ACT>(a.z), row_act<ACT>(a.w));
    if constexpr (DROP) v = drop4(v, i, drop);
    st4(y + i * 4, v);
  }
}
// dx = dy act'(x) m / (1 - p), act' recomputed from x; ACT = none never reads x (which may be NULL): the forward's bits
template <int ACT, bool DROP>
__global__ void __launch_bounds__(256) k_act_dropout_bwd(const float* __restrict__ x, const float* dy, float* dx, int64_t n4,
                                                         DropArgs drop) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 v = ld4(dy + i * 4);
    if constexpr (ACT != kActNone) {
      const float4 a = ld4(x + i * 4);
      v = make_float4(row_act_bwd<ACT>(a.x, v.x), row_act_bwd<ACT>(a.y, v.y), row_act_bwd<ACT>(a.z, v.z), row_act_bwd<ACT>(a.w, v.w));
    }
    if constexpr (DROP) v = drop4(v, i, drop);
    st4(dx + i * 4, v);
  }
}

// ---- launchers (kLnMaxWidth: internal.h) ---------------------------------------------------------------------------
int check_row_width(const char* who, int E) {
  if (E % 4 || E <= 0 || E > kLnMaxWidth) {
    set_error("%s: width %d must be a multiple of 4 in [4, %d]", who, E, kLnMaxWidth);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

int launch_seq_max_bwd(const float* dout, const int* idx, float* dx, int B, int S, int E, hipStream_t st) {
  return timed(DRIN_KC_NORM, st, "k_seq_max_bwd", [&] {
    hipLaunchKernelGGL(k_seq_max_bwd, dim3((unsigned)cdiv(E / 4, 64), (unsigned)B), dim3(256), 0, st, dout, idx, dx, S, E / 4);
  });
}

// workgroups of the row backward kernels (and rows of their partial sums) for `rows` rows
int64_t row_bwd_blocks(int64_t rows) { return cdiv(rows, 4) < kRowBwdBlocks ? cdiv(rows, 4) : kRowBwdBlocks; }
// KERNEL<DV, SUMS> for a row of width4 float4 columns (the forward's four DV instantiations)
#define DRIN_ROW_BWD_ONE(KERNEL, DV, sums, ...)              \
  do {                                                       \
    if (sums)                                                \
      hipLaunchKernelGGL((KERNEL<DV, true>), __VA_ARGS__);   \
    else                                                     \
      hipLaunchKernelGGL((KERNEL<DV, false>), __VA_ARGS__);  \
  } while (0)
#define DRIN_ROW_BWD_DISPATCH(KERNEL, width4, sums, ...)                   \
  do {                                                                     \
    if ((width4) <= 64)                                                    \
      DRIN_ROW_BWD_ONE(KERNEL, 1, sums, __VA_ARGS__);                      \
    else if ((width4) <= 128)                                              \
      DRIN_ROW_BWD_ONE(KERNEL, 2, sums, __VA_ARGS__);                      \
    else if ((width4) <= 256)                                              \
      DRIN_ROW_BWD_ONE(KERNEL, 4, sums, __VA_ARGS__);                      \
    else                                                                   \
      DRIN_ROW_BWD_ONE(KERNEL, 8, sums, __VA_ARGS__);                      \
  } while (0)

int launch_layernorm_res_bwd(const float* x, const float* res, const float* mean, const float* rstd, const float* gamma, const float* dy,
                             float* dh, float* dgamma, float* dbeta, float* partial, int64_t rows, int E, hipStream_t st) {
  const bool sums = dgamma != nullptr || dbeta != nullptr;
  const int64_t blocks = row_bwd_blocks(rows);
  const dim3 grid((unsigned)blocks), block(256);
  DRIN_TRY(timed(DRIN_KC_NORM, st, "k_layernorm_res_bwd", [&] {
    DRIN_ROW_BWD_DISPATCH(k_layernorm_res_bwd, E / 4, sums, grid, block, 0, st, x, res, mean, rstd, gamma, dy, dh, partial, rows, E / 4);
  }));
  if (!sums) return DRIN_OK;
  return timed(DRIN_KC_NORM, st, "k_layernorm_res_bwd_sums", [&] {
    hipLaunchKernelGGL(k_layernorm_res_bwd_sums, dim3((unsigned)cdiv(2 * E, 256)), block, 0, st, partial, (int)blocks, E, dgamma, dbeta);
  });
}

int launch_gate_mix_bwd(const float* tl, const float* vl, const float* ws, const float* bs, const float* dout, float* dtl, float* dvl,
                        float* dws, float* dbs, float* partial, int B, int D, hipStream_t st) {
  const bool sums = dws != nullptr || dbs != nullptr;
  const int64_t blocks = row_bwd_blocks(B);
  const dim3 grid((unsigned)blocks), block(256);
  DRIN_TRY(timed(DRIN_KC_NORM, st, "k_gate_mix_bwd", [&] {
    DRIN_ROW_BWD_DISPATCH(k_gate_mix_bwd, D / 4, sums, grid, block, 0, st, tl, vl, ws, bs, dout, dtl, dvl, partial, B, D / 4);
  }));
  if (!sums) return DRIN_OK;
  return timed(DRIN_KC_NORM, st, "k_gate_mix_bwd_sums", [&] {
    hipLaunchKernelGGL(k_gate_mix_bwd_sums, dim3((unsigned)cdiv(2 * D + 1, 256)), block, 0, st, partial, (int)blocks, 2 * D, dws, dbs);
  });
}

// KERNEL<act, DROP> of the three activations; n4 float4s, at most kActBlocks workgroups
#define DRIN_ACT_DISPATCH(KERNEL, act, dropped, ...)                         \
  do {                                                                       \
    if ((act) == kActGelu) {                                                 \
      if (dropped)                                                           \
        hipLaunchKernelGGL((KERNEL<kActGelu, true>), __VA_ARGS__);           \
      else                                                                   \
        hipLaunchKernelGGL((KERNEL<kActGelu, false>), __VA_ARGS__);          \
    } else if ((act) == kActRelu) {                                          \
      if (dropped)                                                           \
        hipLaunchKernelGGL((KERNEL<kActRelu, true>), __VA_ARGS__);           \
      else                                                                   \
        hipLaunchKernelGGL((KERNEL<kActRelu, false>), __VA_ARGS__);          \
    } else {                                                                 \
      if (dropped)                                                           \
        hipLaunchKernelGGL((KERNEL<kActNone, true>), __VA_ARGS__);           \
      else                                                                   \
        hipLaunchKernelGGL((KERNEL<kActNone, false>), __VA_ARGS__);          \
    }                                                                        \
  } while (0)
dim3 act_grid(int64_t n4) { return dim3((unsigned)(cdiv(n4, 256) < kActBlocks ? cdiv(n4, 256) : kActBlocks)); }

int launch_act_dropout(const float* x, float* y, int64_t n4, int act, const DropArgs* drop, hipStream_t st) {
  const DropArgs da = drop ? *drop : DropArgs{};
  return timed(DRIN_KC_NORM, st, "k_act_dropout",
               [&] { DRIN_ACT_DISPATCH(k_act_dropout, act, drop != nullptr, act_grid(n4), dim3(256), 0, st, x, y, n4, da); });
}
int launch_act_dropout_bwd(const float* x, const float* dy, float* dx, int64_t n4, int act, const DropArgs* drop, hipStream_t st) {
  const DropArgs da = drop ? *drop : DropArgs{};
  return timed(DRIN_KC_NORM, st, "k_act_dropout_bwd",
               [&] { DRIN_ACT_DISPATCH(k_act_dropout_bwd, act, drop != nullptr, act_grid(n4), dim3(256), 0, st, x, dy, dx, n4, da); });
}

// (NamedPtr, DRIN_CHECK_POINTERS, check_count, check_width4: row_checks.h)
int check_scratch(const char* who, const float* scratch, size_t have, size_t need) {
  if (!scratch) {
    set_error("%s: scratch is NULL (%zu floats are needed)", who, need);
    return DRIN_E_NULL;
  }
  if (have < need) {
    set_error("%s: scratch of %zu floats < %zu", who, have, need);
    return DRIN_E_WORKSPACE;
  }
  return DRIN_OK;
}
}  // namespace

// the three that the scoring forward composes as well (ghmfc_forward.hip; declared in internal.h)
int launch_layernorm_res(const float* x, const float* res, const float* gamma, const float* beta, float* y, int64_t rows, int E,
                         float eps, hipStream_t st, float* mean, float* rstd) {
  if (rows <= 0) return DRIN_OK;
  DRIN_TRY(check_row_width("layernorm_res", E));
  const int E4 = E / 4;
  const dim3 grid((unsigned)row_blocks(rows));
  return timed(DRIN_KC_NORM, st, "k_layernorm_res", [&] {
    if (E4 <= 64)
      hipLaunchKernelGGL(k_layernorm_res<1>, grid, dim3(256), 0, st, x, res, gamma, beta, y, mean, rstd, rows, E4, eps);
    else if (E4 <= 128)
      hipLaunchKernelGGL(k_layernorm_res<2>, grid, dim3(256), 0, st, x, res, gamma, beta, y, mean, rstd, rows, E4, eps);
    else if (E4 <= 256)
      hipLaunchKernelGGL(k_layernorm_res<4>, grid, dim3(256), 0, st, x, res, gamma, beta, y, mean, rstd, rows, E4, eps);
    else
      hipLaunchKernelGGL(k_layernorm_res<8>, grid, dim3(256), 0, st, x, res, gamma, beta, y, mean, rstd, rows, E4, eps);
  });
}

int launch_seq_max(const float* x, float* out, int B, int S, int E, hipStream_t st, int* idx) {
  return timed(DRIN_KC_NORM, st, "k_seq_max", [&] {
    const dim3 grid((unsigned)cdiv(E / 4, 64), (unsigned)B);
    if (idx == nullptr)
      hipLaunchKernelGGL(k_seq_max<false>, grid, dim3(256), 0, st, x, out, idx, S, E / 4);
    else
      hipLaunchKernelGGL(k_seq_max<true>, grid, dim3(256), 0, st, x, out, idx, S, E / 4);
  });
}

int launch_gate_mix(const float* tl, const float* vl, const float* ws, const float* bs, float* out, int B, int D, hipStream_t st) {
  return timed(DRIN_KC_NORM, st, "k_gate_mix", [&] {
    hipLaunchKernelGGL(k_gate_mix, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, st, tl, vl, ws, bs, out, B, D / 4);
  });
}

}  // namespace drin

using namespace drin;

// ---- the row operations of GHMFC one by one, forward and backward ---------------------------------
int drin_layernorm_res_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* y, float* mean,
                                 float* rstd, int64_t rows, int32_t width, float eps, void* stream) {
  const char* who = "drin_layernorm_res_train_fwd";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"res", res, false}, {"gamma", gamma, true}, {"beta", beta, true}, {"y", y, true});
  if (!mean || !rstd) {
    set_error("%s: mean / rstd is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_row_width(who, width));
  DRIN_TRY(check_count(who, "rows", rows, 1, INT64_MAX / 4096));
  DRIN_BIND_DEVICE(stream, y, who);
  return launch_layernorm_res(x, res, gamma, beta, y, rows, width, eps, (hipStream_t)stream, mean, rstd);
}

size_t drin_layernorm_res_bwd_scratch_floats(int64_t rows, int32_t width) {
  if (rows < 1 || check_row_width("drin_layernorm_res_bwd_scratch_floats", width) != DRIN_OK) return 0;
  return (size_t)row_bwd_blocks(rows) * 2 * (size_t)width;
}

int drin_layernorm_res_bwd(const float* x, const float* res, const float* mean, const float* rstd, const float* gamma, const float* dy,
                           float* dh, float* dgamma, float* dbeta, float* scratch, size_t scratch_floats, int64_t rows, int32_t width,
                           void* stream) {
  const char* who = "drin_layernorm_res_bwd";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"res", res, false}, {"gamma", gamma, true}, {"dy", dy, true}, {"dh", dh, true},
                      {"dgamma", dgamma, false}, {"dbeta", dbeta, false}, {"scratch", scratch, false});
  if (!mean || !rstd) {
    set_error("%s: mean / rstd is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_row_width(who, width));
  DRIN_TRY(check_count(who, "rows", rows, 1, INT64_MAX / 4096));
  if (dgamma || dbeta) DRIN_TRY(check_scratch(who, scratch, scratch_floats, drin_layernorm_res_bwd_scratch_floats(rows, width)));
  DRIN_BIND_DEVICE(stream, dh, who);
  return launch_layernorm_res_bwd(x, res, mean, rstd, gamma, dy, dh, dgamma, dbeta, scratch, rows, width, (hipStream_t)stream);
}

int drin_seq_max_train_fwd(const float* x, float* out, int32_t* idx, int32_t batch, int32_t seq_len, int32_t width, void* stream) {
  const char* who = "drin_seq_max_train_fwd";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"out", out, true}, {"idx", idx, true});
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "seq_len", seq_len, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_seq_max(x, out, batch, seq_len, width, (hipStream_t)stream, idx);
}

int drin_seq_max_bwd(const float* dout, const int32_t* idx, float* dx, int32_t batch, int32_t seq_len, int32_t width, void* stream) {
  const char* who = "drin_seq_max_bwd";
  DRIN_CHECK_POINTERS(who, {"dout", dout, true}, {"idx", idx, true}, {"dx", dx, true});
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, kMaxGridY));
  DRIN_TRY(check_count(who, "seq_len", seq_len, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, dx, who);
  return launch_seq_max_bwd(dout, idx, dx, batch, seq_len, width, (hipStream_t)stream);
}

int drin_gate_mix_fwd(const float* tl, const float* vl, const float* ws, const float* bs, float* out, int32_t batch, int32_t width,
                      void* stream) {
  const char* who = "drin_gate_mix_fwd";
  DRIN_CHECK_POINTERS(who, {"tl", tl, true}, {"vl", vl, true}, {"ws", ws, true}, {"out", out, true});
  if (!bs) {
    set_error("%s: bs is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_gate_mix(tl, vl, ws, bs, out, batch, width, (hipStream_t)stream);
}

size_t drin_gate_mix_bwd_scratch_floats(int32_t batch, int32_t width) {
  if (batch < 1 || check_row_width("drin_gate_mix_bwd_scratch_floats", width) != DRIN_OK) return 0;
  return (size_t)row_bwd_blocks(batch) * (2 * (size_t)width + 4);
}

int drin_gate_mix_bwd(const float* tl, const float* vl, const float* ws, const float* bs, const float* dout, float* dtl, float* dvl,
                      float* dws, float* dbs, float* scratch, size_t scratch_floats, int32_t batch, int32_t width, void* stream) {
  const char* who = "drin_gate_mix_bwd";
  DRIN_CHECK_POINTERS(who, {"tl", tl, true}, {"vl", vl, true}, {"ws", ws, true}, {"dout", dout, true}, {"dtl", dtl, true},
                      {"dvl", dvl, true}, {"dws", dws, false}, {"scratch", scratch, false});
  if (!bs) {
    set_error("%s: bs is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_row_width(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  if (dws || dbs) DRIN_TRY(check_scratch(who, scratch, scratch_floats, drin_gate_mix_bwd_scratch_floats(batch, width)));
  DRIN_BIND_DEVICE(stream, dtl, who);
  return launch_gate_mix_bwd(tl, vl, ws, bs, dout, dtl, dvl, dws, dbs, scratch, batch, width, (hipStream_t)stream);
}

int drin_cosine_rows_fwd(const float* x, const float* y, float* out, int32_t batch, int32_t num_candidates, int32_t width, float eps,
                         void* stream) {
  const char* who = "drin_cosine_rows_fwd";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"y", y, true});
  if (!out) {
    set_error("%s: out is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "num_candidates", num_candidates, 1, kMaxGridY));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_cosine_rows(x, y, width, out, batch, num_candidates, width, eps, 1.0f, (hipStream_t)stream);
}

int drin_cosine_rows_bwd(const float* x, const float* y, const float* dout, float* dx, float* dy, float* scratch, size_t scratch_floats,
                         int32_t batch, int32_t num_candidates, int32_t width, float eps, void* stream) {
  const char* who = "drin_cosine_rows_bwd";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"y", y, true}, {"dx", dx, true}, {"dy", dy, true});
  if (!dout) {
    set_error("%s: dout is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_width4(who, width));
  if (width > 1024) {
    set_error("%s: width %d exceeds 1024 (the cosine backward keeps a row in registers)", who, width);
    return DRIN_E_UNSUPPORTED;
  }
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "num_candidates", num_candidates, 1, kMaxGridY));
  DRIN_TRY(check_scratch(who, scratch, scratch_floats, 3 * (size_t)batch * (size_t)num_candidates));
  DRIN_BIND_DEVICE(stream, dx, who);
  return launch_cosine_bwd(x, y, dout, dx, dy, scratch, batch, num_candidates, width, eps, (hipStream_t)stream);
}

int drin_entity_token_mean(const float* feat, const int64_t* mask, float* out, int64_t pairs, int32_t tokens, int32_t width,
                           void* stream) {
  const char* who = "drin_entity_token_mean";
  DRIN_CHECK_POINTERS(who, {"feat", feat, true}, {"out", out, true});
  if (!mask) {
    set_error("%s: mask is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "pairs", pairs, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "tokens", tokens, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_entity_token_mean(feat, mask, out, pairs, tokens, width, (hipStream_t)stream);
}

int drin_entity_token_pool(const float* feat, const int64_t* mask, float* out, int64_t pairs, int32_t tokens, int32_t width,
                           int32_t pooling, void* stream) {
  const char* who = "drin_entity_token_pool";
  DRIN_CHECK_POINTERS(who, {"feat", feat, true}, {"out", out, true});
  if (!mask) {
    set_error("%s: mask is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_entity_pooling(who, pooling));
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "pairs", pairs, 1, INT32_MAX));
  DRIN_TRY(check_count(who, "tokens", tokens, 1, 512));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_entity_token_pool(feat, mask, out, pairs, tokens, width, pooling, (hipStream_t)stream);
}

// ---- the FFN activation, row dropout and the span mean of GHMFC's other mention encoders ------------
namespace {
int act_dropout_args(const char* who, int64_t rows, int32_t width, int32_t act, float p, uint64_t seed, uint64_t call, DropArgs* drop,
                     bool* use) {
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "rows", rows, 1, INT64_MAX / 4096 / width));
  if (act != DRIN_ROW_ACT_NONE && act != DRIN_ROW_ACT_RELU && act != DRIN_ROW_ACT_GELU) {
    set_error("%s: act = %d is none of DRIN_ROW_ACT_NONE / _RELU / _GELU (%d, %d, %d)", who, act, DRIN_ROW_ACT_NONE, DRIN_ROW_ACT_RELU,
              DRIN_ROW_ACT_GELU);
    return DRIN_E_SHAPE;
  }
  return dropout_args(who, p, seed, call, drop, use);
}
int span_args(const char* who, const int64_t* start, const int64_t* end, int32_t batch, int32_t seq_len, int32_t width) {
  if (!start || !end) {
    set_error("%s: start / end is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, INT32_MAX));
  return check_count(who, "seq_len", seq_len, 1, INT32_MAX);
}
}  // namespace

int drin_act_dropout_fwd(const float* x, float* y, int64_t rows, int32_t width, int32_t act, float p, uint64_t seed, uint64_t call,
                         void* stream) {
  const char* who = "drin_act_dropout_fwd";
  DRIN_CHECK_POINTERS(who, {"x", x, true}, {"y", y, true});
  DropArgs drop;
  bool use;
  DRIN_TRY(act_dropout_args(who, rows, width, act, p, seed, call, &drop, &use));
  DRIN_BIND_DEVICE(stream, y, who);
  return launch_act_dropout(x, y, rows * (width / 4), act, use ? &drop : nullptr, (hipStream_t)stream);
}

int drin_act_dropout_bwd(const float* x, const float* dy, float* dx, int64_t rows, int32_t width, int32_t act, float p, uint64_t seed,
                         uint64_t call, void* stream) {
  const char* who = "drin_act_dropout_bwd";
  DRIN_CHECK_POINTERS(who, {"x", x, act != DRIN_ROW_ACT_NONE}, {"dy", dy, true}, {"dx", dx, true});
  DropArgs drop;
  bool use;
  DRIN_TRY(act_dropout_args(who, rows, width, act, p, seed, call, &drop, &use));
  DRIN_BIND_DEVICE(stream, dx, who);
  return launch_act_dropout_bwd(x, dy, dx, rows * (width / 4), act, use ? &drop : nullptr, (hipStream_t)stream);
}

int drin_span_mean_fwd(const float* seq, const int64_t* start, const int64_t* end, float* out, int32_t batch, int32_t seq_len,
                       int32_t width, void* stream) {
  const char* who = "drin_span_mean_fwd";
  DRIN_CHECK_POINTERS(who, {"seq", seq, true}, {"out", out, true});
  DRIN_TRY(span_args(who, start, end, batch, seq_len, width));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_span_mean(seq, start, end, out, batch, seq_len, width, (hipStream_t)stream);
}

int drin_span_mean_bwd(const float* dout, const int64_t* start, const int64_t* end, float* dseq, int32_t batch, int32_t seq_len,
                       int32_t width, void* stream) {
  const char* who = "drin_span_mean_bwd";
  DRIN_CHECK_POINTERS(who, {"dout", dout, true}, {"dseq", dseq, true});
  DRIN_TRY(span_args(who, start, end, batch, seq_len, width));
  DRIN_BIND_DEVICE(stream, dseq, who);
  return launch_span_mean_bwd(dout, start, end, dseq, batch, seq_len, width, (hipStream_t)stream);
}

