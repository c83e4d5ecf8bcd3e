// Backward of the parameter-free input stages of Model.forward (drin/model.py:164-204): the gradients of the batch
// tensors themselves (drin_backward_ex's drin_input_grads, drin_pool_bwd).  Every output is WRITTEN (no read-modify-write)
// and every sum runs in a fixed order (no atomics): two backward passes give the same bits.
#include <hip/hip_runtime.h>

#include "device_utils.h"
#include "internal.h"

namespace drin {

// ------------------------------------------------------------------------------------------------
// Avg.avg backward (ghmfc.py:54-60): out[b, t, :] = g[b, :] / (e - s) for s <= t < e, 0 elsewhere; s, e clipped exactly as
// k_span_mean clips them (python slice semantics).  An empty span writes zeros (no row of the slice receives anything).
__global__ void __launch_bounds__(256) k_span_mean_bwd(const float* __restrict__ g, const int64_t* __restrict__ start,
                                                       const int64_t* __restrict__ end, float* __restrict__ out, int L,
                                                       int D4) {
  const int t = blockIdx.x;
  const int64_t b = blockIdx.y;
  int64_t s = start[b], e = end[b];
  if (s < 0) s = s + L < 0 ? 0 : s + L;
  if (e < 0) e = e + L < 0 ? 0 : e + L;
  if (e > L) e = L;
  if (s > L) s = L;
  const bool in = t >= s && t < e;
  const float cnt = (float)(e - s);
  float* o = out + (b * L + t) * (int64_t)D4 * 4;
  const float* gr = g + b * (int64_t)D4 * 4;
  for (int c4 = threadIdx.x; c4 < D4; c4 += blockDim.x) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) {
      const float4 x = ld4(gr + c4 * 4);
      v = make_float4(x.x / cnt, x.y / cnt, x.z / cnt, x.w / cnt);
    }
    st4(o + c4 * 4, v);
  }
}

int launch_span_mean_bwd(const float* g, const int64_t* start, const int64_t* end, float* out, int B, int L, int D,
                         hipStream_t st) {
  if (B <= 0) return DRIN_OK;
  return for_grid_slices(B, [&](int64_t b0, int nb) -> int {
    KernelTimer timer(DRIN_KC_POOL, st);
    hipLaunchKernelGGL(k_span_mean_bwd, dim3((unsigned)L, (unsigned)nb), dim3(D / 4 >= 192 ? 192 : 64), 0, st, g + b0 * D,
                       start + b0, end + b0, out + b0 * L * D, L, D / 4);
    DRIN_CHECK_LAUNCH("k_span_mean_bwd");
    return DRIN_OK;
  });
}

// ------------------------------------------------------------------------------------------------
// torch.mean(x, dim=-2) backward (model.py:41-44,78-79,82-83): out[g, s, :] = in[g, :] / S.  Flat grid-stride over float4s.
__global__ void __launch_bounds__(256) k_axis_mean_bwd(const float* __restrict__ in, float* __restrict__ out, int64_t n4,
                                                       int S, int C4) {
  const float fs = (float)S;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c4 = i % C4, g = i / ((int64_t)C4 * S);
    const float4 x = ld4(in + (g * C4 + c4) * 4);
    st4(out + i * 4, make_float4(x.x / fs, x.y / fs, x.z / fs, x.w / fs));
  }
}

int launch_axis_mean_bwd(const float* in, float* out, int64_t groups, int inner, int cols, hipStream_t st) {
  const int64_t n4 = groups * inner * (int64_t)(cols / 4);
  if (n4 <= 0) return DRIN_OK;
  const int64_t blocks = cdiv(n4, 256) < 8192 ? cdiv(n4, 256) : 8192;
  KernelTimer timer(DRIN_KC_POOL, st);
  hipLaunchKernelGGL(k_axis_mean_bwd, dim3((unsigned)blocks), dim3(256), 0, st, in, out, n4, inner, cols / 4);
  DRIN_CHECK_LAUNCH("k_axis_mean_bwd");
  return DRIN_OK;
}

// ------------------------------------------------------------------------------------------------
// Backward of the WikiMEL entity pooling (ghmfc.py:245-249) plus the text-text edge's token-0 read (model.py:73-75):
//   out[p, 0, :] = g_cls[p, :]   (0 without g_cls),   out[p, t, :] = g_pool[p, :] / (stop - 1) for 1 <= t < stop,   0 elsewhere,
// stop = ntok - 1 with the slice rules of k_entity_token_mean (ntok == 0 -> stop = T - 1).  The HBM-bound write of the token
// block: one workgroup per pair, each thread owns V consecutive columns (16-byte stores: 4 fp32 or 8 bf16), keeps the two row
// values in registers and writes every row of the pair once.
template <typename OutT, int V>
__global__ void __launch_bounds__(256) k_token_block_bwd(const float* __restrict__ g_pool, const float* __restrict__ g_cls,
                                                         const int64_t* __restrict__ mask, OutT* __restrict__ out, int T,
                                                         int D) {
  const int64_t p = blockIdx.x;
  int cnt = 0;
  for (int t = threadIdx.x & 63; t < T; t += 64) cnt += (int)mask[p * T + t];
  cnt = (int)wave_sum((float)cnt);
  int stop = cnt - 1;
  if (stop < 0) stop += T;
  if (stop < 0) stop = 0;
  if (stop > T) stop = T;
  const float den = (float)(stop - 1);
  OutT* base = out + p * (int64_t)T * D;
  for (int c = threadIdx.x * V; c < D; c += blockDim.x * V) {
    float gp[V], gc[V];
#pragma unroll
    for (int k = 0; k < V; k += 4) {
      const float4 a = ld4(g_pool + p * D + c + k);
      gp[k] = a.x / den, gp[k + 1] = a.y / den, gp[k + 2] = a.z / den, gp[k + 3] = a.w / den;
      const float4 z = g_cls ? ld4(g_cls + p * D + c + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      gc[k] = z.x, gc[k + 1] = z.y, gc[k + 2] = z.z, gc[k + 3] = z.w;
    }
    for (int t = 0; t < T; ++t) {
      OutT v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = (OutT)(t == 0 ? gc[k] : (t < stop ? gp[k] : 0.f));
      typedef float f4_t __attribute__((ext_vector_type(4)));
      *reinterpret_cast<f4_t*>(base + (int64_t)t * D + c) = *reinterpret_cast<const f4_t*>(v);   // 16 bytes
    }
  }
}

int launch_token_block_bwd(const float* g_pool, const float* g_cls, const int64_t* mask, void* out, int64_t pairs, int T,
                           int D, bool bf16, hipStream_t st) {
  if (pairs <= 0) return DRIN_OK;
  if (bf16 && (D % 8)) {
    set_error("drin_pool_bwd: bf16 token blocks need embed_dim %% 8 == 0 (16-byte stores), got %d", D);
    return DRIN_E_SHAPE;
  }
  const int V = bf16 ? 8 : 4;
  const int per_row = D / V;
  const int threads = per_row >= 192 ? 192 : (per_row > 64 ? 128 : 64);
  for (int64_t p0 = 0; p0 < pairs; p0 += (int64_t)1 << 30) {
    const int64_t np = pairs - p0 < ((int64_t)1 << 30) ? pairs - p0 : ((int64_t)1 << 30);
    KernelTimer timer(DRIN_KC_POOL, st);
    if (bf16)
      hipLaunchKernelGGL((k_token_block_bwd<__bf16, 8>), dim3((unsigned)np), dim3(threads), 0, st, g_pool + p0 * D,
                         g_cls ? g_cls + p0 * D : nullptr, mask + p0 * T, static_cast<__bf16*>(out) + p0 * T * D, T, D);
    else
      hipLaunchKernelGGL((k_token_block_bwd<float, 4>), dim3((unsigned)np), dim3(threads), 0, st, g_pool + p0 * D,
                         g_cls ? g_cls + p0 * D : nullptr, mask + p0 * T, static_cast<float*>(out) + p0 * T * D, T, D);
    DRIN_CHECK_LAUNCH("k_token_block_bwd");
  }
  return DRIN_OK;
}

// ------------------------------------------------------------------------------------------------
// Row sums: out[r] = sum_c in[r, c] (one wave per row).  Vector edges: the initial scalar edges are broadcast over D
// (model.py:202), so their gradient is the row sum of the layer-0 vector edge gradient.
__global__ void __launch_bounds__(256) k_row_sum(const float* __restrict__ in, float* __restrict__ out, int64_t rows, int C4) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int c4 = lane; c4 < C4; c4 += 64) {
    const float4 v = ld4(in + (r * C4 + c4) * 4);
    s += (v.x + v.y) + (v.z + v.w);
  }
  s = wave_sum(s);
  if (lane == 0) out[r] = s;
}

int launch_row_sum(const float* in, float* out, int64_t rows, int C, hipStream_t st) {
  if (rows <= 0) return DRIN_OK;
  KernelTimer timer(DRIN_KC_EDGE, st);
  hipLaunchKernelGGL(k_row_sum, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, st, in, out, rows, C / 4);
  DRIN_CHECK_LAUNCH("k_row_sum");
  return DRIN_OK;
}

// ------------------------------------------------------------------------------------------------
// Backward of the image-image edge (model.py:78-92), miei = S / (W + eps), S = sum_ij cos_ij w_ij, W = sum_ij w_ij,
// w_ij = ms_i es_j - as autograd differentiates it:
//   g_S = g / (W + eps),  g_W = -g S / (W + eps)^2,  g_w_ij = g_S cos_ij + g_W,  g_cos_ij = g_S w_ij
//   d es_j = sum_i g_w_ij ms_i,   d ms_i = sum_n sum_j g_w_nij es_nj,
//   d y_j = sum_i g_cos_ij (x_i / (nx_i ny_j) - [|y_j| > eps] cos_ij y_j / ny_j^2)       (nx = max(|x|, eps), as k_cosine_bwd)
//   d x_i = sum_n sum_j g_cos_nij (y_nj / (nx_i ny_nj) - [|x_i| > eps] cos_nij x_i / nx_i^2)
// Pair kernel: one wave per pair; writes d es, d y (entity side) and, for the mention-side kernel, g_cos, cos, ny per
// (pair, i, j) / (pair, j), the per-pair share of d ms and the norms of the mention rows.
constexpr int kMieiMaxPairs = 64;   // Km * Ke held per wave in LDS

__global__ void __launch_bounds__(256) k_miei_bwd_pair(const float* __restrict__ mobj, const float* __restrict__ mscore,
                                                       const float* __restrict__ eobj, const float* __restrict__ escore,
                                                       const float* __restrict__ g, float* __restrict__ d_escore,
                                                       float* __restrict__ d_eobj, float* __restrict__ gcos_out,
                                                       float* __restrict__ cos_out, float* __restrict__ ny_out,
                                                       float* __restrict__ dms_part, float* __restrict__ nx_out,
                                                       int64_t pairs, int N, int Km, int Ke, int R4, float cos_eps,
                                                       float miei_eps) {
  __shared__ float s_cos[4][kMieiMaxPairs], s_gw[4][kMieiMaxPairs], s_nx[4][kMieiMaxPairs], s_ny[4][kMieiMaxPairs];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + wave;
  if (p >= pairs) return;
  const int64_t b = p / N;
  const int KK = Km * Ke;
  float sim = 0.f, wsum = 0.f;
  for (int i = 0; i < Km; ++i) {
    const float* xr = mobj + (b * Km + i) * (int64_t)R4 * 4;
    const float ms = mscore[b * Km + i];
    for (int j = 0; j < Ke; ++j) {
      const float* yr = eobj + (p * Ke + j) * (int64_t)R4 * 4;
      float xy = 0.f, xx = 0.f, yy = 0.f;
      for (int c4 = lane; c4 < R4; c4 += 64) {
        const float4 a = ld4(xr + c4 * 4), v = ld4(yr + c4 * 4);
        xy += dot4(a, v);
        xx += dot4(a, a);
        yy += dot4(v, v);
      }
      xy = wave_sum(xy);
      xx = wave_sum(xx);
      yy = wave_sum(yy);
      const float c = cosine_from_sums(xy, xx, yy, cos_eps);
      const float w = ms * escore[p * Ke + j];
      sim += c * w;
      wsum += w;
      // every lane writes the same (wave-uniform) value and reads back only what it wrote itself
      s_cos[wave][i * Ke + j] = c;
      s_nx[wave][i] = sqrtf(xx);
      s_ny[wave][j] = sqrtf(yy);
    }
  }
  const float gg = g[p];
  const float den = wsum + miei_eps;
  const float g_s = gg / den;
  const float g_w = -gg * sim / (den * den);
  for (int k = 0; k < KK; ++k) s_gw[wave][k] = g_s * s_cos[wave][k] + g_w;
  if (lane == 0) {
    for (int j = 0; j < Ke; ++j) {
      float s = 0.f;
      for (int i = 0; i < Km; ++i) s += s_gw[wave][i * Ke + j] * mscore[b * Km + i];
      d_escore[p * Ke + j] = s;
      ny_out[p * Ke + j] = s_ny[wave][j];
    }
    for (int i = 0; i < Km; ++i) {
      float s = 0.f;
      for (int j = 0; j < Ke; ++j) s += s_gw[wave][i * Ke + j] * escore[p * Ke + j];
      dms_part[p * Km + i] = s;
      for (int j = 0; j < Ke; ++j) {
        gcos_out[p * KK + i * Ke + j] = g_s * mscore[b * Km + i] * escore[p * Ke + j];
        cos_out[p * KK + i * Ke + j] = s_cos[wave][i * Ke + j];
      }
      if (p % N == 0) nx_out[b * Km + i] = s_nx[wave][i];
    }
  }
  // entity rows: d y_j
  for (int j = 0; j < Ke; ++j) {
    const float nyr = s_ny[wave][j], ny = fmaxf(nyr, cos_eps);
    float ky = 0.f;
    for (int i = 0; i < Km; ++i) ky += g_s * mscore[b * Km + i] * escore[p * Ke + j] * s_cos[wave][i * Ke + j];
    ky = nyr > cos_eps ? ky / (ny * ny) : 0.f;
    const float* yr = eobj + (p * Ke + j) * (int64_t)R4 * 4;
    float* dr = d_eobj + (p * Ke + j) * (int64_t)R4 * 4;
    for (int c4 = lane; c4 < R4; c4 += 64) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 0; i < Km; ++i) {
        const float a = g_s * mscore[b * Km + i] * escore[p * Ke + j] / (fmaxf(s_nx[wave][i], cos_eps) * ny);
        acc = fma4(a, ld4(mobj + (b * Km + i) * (int64_t)R4 * 4 + c4 * 4), acc);
      }
      st4(dr + c4 * 4, fma4(-ky, ld4(yr + c4 * 4), acc));
    }
  }
}

// Mention side: one workgroup per (mention, 64 float4 columns); the four waves split the candidate loop and are combined in
// a fixed order (as k_cosine_bwd_mention).  Column block 0 also sums d ms over the candidates, in order.
__global__ void __launch_bounds__(256) k_miei_bwd_mention(const float* __restrict__ mobj, const float* __restrict__ eobj,
                                                          const float* __restrict__ gcos, const float* __restrict__ cosv,
                                                          const float* __restrict__ nyv, const float* __restrict__ dms_part,
                                                          const float* __restrict__ nxv, float* __restrict__ d_mobj,
                                                          float* __restrict__ d_mscore, int N, int Km, int Ke, int R4,
                                                          float cos_eps) {
  __shared__ float4 part[4][64];
  __shared__ float part_k[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c4 = blockIdx.x * 64 + lane;
  const int64_t b = blockIdx.y;
  const int KK = Km * Ke;
  if (blockIdx.x == 0 && threadIdx.x < Km) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += dms_part[(b * N + n) * Km + threadIdx.x];
    d_mscore[b * Km + threadIdx.x] = s;
  }
  for (int i = 0; i < Km; ++i) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    float sk = 0.f;
    if (c4 < R4) {
      for (int n = wave; n < N; n += 4) {
        const int64_t p = b * N + n;
        for (int j = 0; j < Ke; ++j) {
          const float a = gcos[p * KK + i * Ke + j];
          s = fma4(a / fmaxf(nyv[p * Ke + j], cos_eps), ld4(eobj + (p * Ke + j) * (int64_t)R4 * 4 + (int64_t)c4 * 4), s);
          sk += a * cosv[p * KK + i * Ke + j];
        }
      }
    }
    part[wave][lane] = s;
    part_k[wave][lane] = sk;
    __syncthreads();
    if (wave == 0 && c4 < R4) {
      s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      sk = (part_k[0][lane] + part_k[1][lane]) + (part_k[2][lane] + part_k[3][lane]);
      const float nxr = nxv[b * Km + i], nx = fmaxf(nxr, cos_eps);
      const float k = nxr > cos_eps ? sk / (nx * nx) : 0.f;
      const float4 xv = ld4(mobj + (b * Km + i) * (int64_t)R4 * 4 + (int64_t)c4 * 4);
      float4 r;
      r.x = s.x / nx - k * xv.x;
      r.y = s.y / nx - k * xv.y;
      r.z = s.z / nx - k * xv.z;
      r.w = s.w / nx - k * xv.w;
      st4(d_mobj + (b * Km + i) * (int64_t)R4 * 4 + (int64_t)c4 * 4, r);
    }
    __syncthreads();
  }
}

size_t miei_bwd_scratch_floats(int64_t pairs, int B, int Km, int Ke) {
  auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };
  return 2 * up((size_t)pairs * Km * Ke) + up((size_t)pairs * Ke) + up((size_t)pairs * Km) + up((size_t)B * Km);
}

int launch_miei_bwd(const float* mobj, const float* mscore, const float* eobj, const float* escore, const float* g,
                    float* d_mobj, float* d_mscore, float* d_eobj, float* d_escore, float* scratch, int B, int N, int Km,
                    int Ke, int R, float cos_eps, float miei_eps, hipStream_t st) {
  const int64_t pairs = (int64_t)B * N;
  if (pairs <= 0 || Km <= 0 || Ke <= 0) return DRIN_OK;
  if (Km * Ke > kMieiMaxPairs) {
    set_error("input gradients: mention_objects x entity_objects = %d x %d > %d object pairs is not built", Km, Ke, kMieiMaxPairs);
    return DRIN_E_UNSUPPORTED;
  }
  auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };
  float* gcos = scratch;
  float* cosv = gcos + up((size_t)pairs * Km * Ke);
  float* nyv = cosv + up((size_t)pairs * Km * Ke);
  float* dms = nyv + up((size_t)pairs * Ke);
  float* nxv = dms + up((size_t)pairs * Km);
  {
    KernelTimer timer(DRIN_KC_EDGE, st);
    hipLaunchKernelGGL(k_miei_bwd_pair, dim3((unsigned)cdiv(pairs, 4)), dim3(256), 0, st, mobj, mscore, eobj, escore, g,
                       d_escore, d_eobj, gcos, cosv, nyv, dms, nxv, pairs, N, Km, Ke, R / 4, cos_eps, miei_eps);
    DRIN_CHECK_LAUNCH("k_miei_bwd_pair");
  }
  return for_grid_slices(B, [&](int64_t b0, int nb) -> int {
    const int64_t po = b0 * N;
    KernelTimer timer(DRIN_KC_EDGE, st);
    hipLaunchKernelGGL(k_miei_bwd_mention, dim3((unsigned)cdiv(R / 4, 64), (unsigned)nb), dim3(256), 0, st, mobj + b0 * Km * R,
                       eobj + po * Ke * R, gcos + po * Km * Ke, cosv + po * Km * Ke, nyv + po * Ke, dms + po * Km, nxv + b0 * Km,
                       d_mobj + b0 * Km * R, d_mscore + b0 * Km, N, Km, Ke, R / 4, cos_eps);
    DRIN_CHECK_LAUNCH("k_miei_bwd_mention");
    return DRIN_OK;
  });
}

}  // namespace drin
