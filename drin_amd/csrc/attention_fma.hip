// The softmax-attention core on the FMA pipes, forward and backward with dropout as a template flag (DESIGN.md sections 15,
// 16, 18): the kernels and their launchers.  The matrix-core twin is attention_mfma.hip; the entry points of both and
// their checks are attention_api.hip.  No atomics, no scratch memory, at most 54 KB of static LDS per workgroup: the same
// bits every run.
#include "attention_common.h"
#include "device_utils.h"

namespace drin {
namespace {

// ---- softmax attention (ghmfc.py:120,124: nn.MultiheadAttention -> scaled_dot_product_attention) ----------------------
// One workgroup per (mention, head, 16 query rows): wave w owns query rows 4 w .. 4 w + 3.  Keys go through LDS in tiles
// of KT (64 when the padded head dim is <= 128, else 32: fp32 K and V of one (mention, head) at Lk = 128, dh = 256 are
// 256 KB) with a running max and sum per query row; K and V of a tile take turns in ONE buffer.
//   scores: lane = key.  K rows sit at a stride of 4 * odd floats, so the 16 lanes of a ds_read_b128 group (each group is a
//           complete residue set mod 16, MI355X_MICROARCH.md) meet 16 different bank quads; the q values are broadcast reads.
//           With KT = 32 the two half-waves take two query rows each.
//   p V:    lane = output column (lane, lane + 64, ...: consecutive banks), p of the four rows is one broadcast float4 per key.
// q is staged multiplied by log2(e) / sqrt(dh): the exponentials are exp2.  A key is dropped when mask[b, key] == 0; a row
// with no kept key keeps l = 0 and writes zeros (what torch's kernel gives for an all-masked row: zero weights).
constexpr int kAttnRows = 4, kAttnWaves = 4, kAttnQT = kAttnRows * kAttnWaves;
constexpr int kAttnKvFloats = 64 * 132;   // 64 keys x (128 + 4) >= 32 keys x (256 + 4)

template <int CTRL>
__device__ __forceinline__ float dpp_max_self(float v) {   // every lane of these four controls has a source lane: no fill value
  const int b = __builtin_bit_cast(int, v);
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, CTRL, 0xF, 0xF, false)));
}
__device__ __forceinline__ float wave_max_any(float v) {   // max over the 64 lanes of any values (-inf included)
  v = dpp_max_self<0xB1>(v);
  v = dpp_max_self<0x4E>(v);
  v = dpp_max_self<0x141>(v);
  v = dpp_max_self<0x140>(v);
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// `valid` rows x dh columns of a row-major global block -> LDS rows of stride ds, times mul; rows valid .. rows - 1 and the
// columns dh .. dhp - 1 are zero.  vec: dh % 4 == 0 and the source rows are 16-byte aligned.
__device__ __forceinline__ void stage_rows(float* dst, int ds, const float* src, int64_t ld, int rows, int valid, int dh, int dhp,
                                           bool vec, float mul) {
  if (vec) {
    const int n4 = dh >> 2;
    for (int i = threadIdx.x; i < rows * n4; i += 256) {
      const int r = i / n4, c4 = i - r * n4;
      const float4 x = r < valid ? ld4(src + r * ld + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      st4(dst + r * ds + c4 * 4, x * mul);
    }
  } else {
    for (int i = threadIdx.x; i < rows * dhp; i += 256) {
      const int r = i / dhp, c = i - r * dhp;
      dst[r * ds + c] = (r < valid && c < dh) ? src[r * ld + c] * mul : 0.f;
    }
  }
}

// DROP (drin_attention_dropout_fwd): the weight of (query i, key j) that goes into p V is multiplied by keep / (1 - rate)
// (dropout_mask.h); the running max, the sum l and lse are those of the undropped scores.  A separate instantiation: the
// code of DROP = false is what it was.  (DropArgs: attention_common.h)

template <int KT, bool DROP = false>
__global__ void __launch_bounds__(256) k_attention(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                   const float* __restrict__ v, int64_t ldv, const int64_t* __restrict__ mask,
                                                   float* __restrict__ out, int64_t ldo, float* __restrict__ lse, int Lq, int Lk,
                                                   int dh, float q_scale, int vec, DropArgs drop) {
  constexpr int G = 64 / KT;             // half-waves of the score phase
  constexpr int RPL = kAttnRows / G;     // query rows per lane there
  __shared__ __attribute__((aligned(16))) float kv[kAttnKvFloats];
  __shared__ __attribute__((aligned(16))) float qs[kAttnQT * kAttnMaxDh];
  __shared__ __attribute__((aligned(16))) float ps[kAttnWaves * 64 * kAttnRows];   // [wave][key][row]
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kAttnQT;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int dhp = (dh + 3) & ~3;
  const int ks = 4 * ((dhp >> 2) | 1);
  const float ninf = -__builtin_inff();
  const int q_valid = Lq - q0 < kAttnQT ? Lq - q0 : kAttnQT;
  stage_rows(qs, dhp, q + ((int64_t)b * Lq + q0) * ldq + (int64_t)h * dh, ldq, kAttnQT, q_valid, dh, dhp, vec != 0, q_scale);
  k += (int64_t)b * Lk * ldk + (int64_t)h * dh;
  v += (int64_t)b * Lk * ldv + (int64_t)h * dh;
  if (mask != nullptr) mask += (int64_t)b * Lk;

  float m[kAttnRows], l[kAttnRows], acc[kAttnRows][4];
#pragma unroll
  for (int r = 0; r < kAttnRows; ++r) {
    m[r] = ninf, l[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = 0.f;
  }
  const int g = G == 1 ? 0 : lane / KT, j = lane & (KT - 1);
  const float* qg = qs + (w * kAttnRows + g * RPL) * dhp;
  const float* kr = kv + j * ks;
  float* pw = ps + w * 64 * kAttnRows;

  for (int j0 = 0; j0 < Lk; j0 += KT) {
    const int jn = Lk - j0 < KT ? Lk - j0 : KT;
    __syncthreads();   // the previous tile's V has been read (first tile: nothing)
    stage_rows(kv, ks, k + j0 * ldk, ldk, jn, jn, dh, dhp, vec != 0, 1.0f);
    __syncthreads();   // K (and, the first time, q) are in LDS
    float s[RPL];
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) s[rr] = 0.f;
    for (int c = 0; c < dhp; c += 4) {
      const float4 kk = ld4(kr + c);
#pragma unroll
      for (int rr = 0; rr < RPL; ++rr) {
        const float4 qq = ld4(qg + rr * dhp + c);
        s[rr] = fmaf(qq.x, kk.x, fmaf(qq.y, kk.y, fmaf(qq.z, kk.z, fmaf(qq.w, kk.w, s[rr]))));
      }
    }
    const bool keep = j < jn && (mask == nullptr || mask[j0 + j] != 0);
    float p[kAttnRows];
#pragma unroll
    for (int r = 0; r < kAttnRows; ++r) {
      const float sr = (keep && r / RPL == g) ? s[r % RPL] : ninf;   // rows of the other half-wave: no part in this lane
      const float mn = fmaxf(m[r], wave_max_any(sr));
      const bool none = mn == ninf;                                 // no kept key so far
      const float alpha = none ? 1.0f : exp2f(m[r] - mn);
      p[r] = none ? 0.f : exp2f(sr - mn);
      l[r] = fmaf(l[r], alpha, wave_sum(p[r]));
      m[r] = mn;
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] *= alpha;
    }
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) {   // (p of the other half-wave's rows is exactly 0 in this lane: the sum is a select)
      float pv = G == 2 ? p[rr] + p[(RPL + rr) % kAttnRows] : p[rr];
      if constexpr (DROP) {
        const uint64_t e = (((uint64_t)b * gridDim.y + h) * Lq + (q0 + w * kAttnRows + g * RPL + rr)) * Lk + (j0 + j);
        pv = dropout_keep(drop.seed, drop.call, e, drop.threshold) ? pv * drop.scale : 0.f;
      }
      pw[j * kAttnRows + g * RPL + rr] = pv;
    }
    __syncthreads();   // every wave is through with K; p of this wave is in LDS
    stage_rows(kv, dh, v + j0 * ldv, ldv, jn, jn, dh, dh, vec != 0, 1.0f);
    __syncthreads();
    for (int jj = 0; jj < jn; ++jj) {
      const float4 pp = ld4(pw + jj * kAttnRows);
      const float* vr = kv + jj * dh + lane;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (64 * c < dh) {   // uniform; a lane past dh in the last slot reads inside kv and is never stored
          const float vv = vr[64 * c];
          acc[0][c] = fmaf(pp.x, vv, acc[0][c]);
          acc[1][c] = fmaf(pp.y, vv, acc[1][c]);
          acc[2][c] = fmaf(pp.z, vv, acc[2][c]);
          acc[3][c] = fmaf(pp.w, vv, acc[3][c]);
        }
    }
  }
#pragma unroll
  for (int r = 0; r < kAttnRows; ++r) {
    const int row = q0 + w * kAttnRows + r;
    if (row >= Lq) continue;
    const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;
    if (lse != nullptr && lane == 0)   // natural log of the row's sum of exp(score); m is in log2 units (q_scale)
      lse[((int64_t)b * gridDim.y + h) * Lq + row] = l[r] > 0.f ? (m[r] + log2f(l[r])) * 0.69314718055994530942f : ninf;
    float* o = out + ((int64_t)b * Lq + row) * ldo + (int64_t)h * dh;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (lane + 64 * c < dh) o[lane + 64 * c] = acc[r][c] * inv;
  }
}

// ---- backward of the softmax-attention core (what autograd runs for ghmfc.py:120,124 under train.py:33-34) -----------
// With p = exp(s - lse) recomputed from the forward's row statistic, delta_i = sum_c dO[i, c] O[i, c], dp = dO V^T and
// ds = p (dp - delta):  dQ = ds K / sqrt(dh),  dK = ds^T Q / sqrt(dh),  dV = p^T dO.  Three kernels, no atomics:
//   k_attention_bwd_delta  one wave per (mention, head, query row): delta into the caller's scratch
//   k_attention_bwd_dq     one workgroup per (mention, head, QT query rows), loops over tiles of KT keys
//   k_attention_bwd_dkv    one workgroup per (mention, head, KT keys) owns those keys' dK and dV rows, loops over query tiles
// Tiles: (KT, QT) = (32, 16) when the padded head dim is <= 128, else (16, 8): Q, dO, K and V tiles are all resident
// (50 - 54 KB of static LDS).  Every tile row sits at a stride of 4 * odd floats.  The probabilities of a tile are formed
// one (query, key) pair per thread: the operand that differs over the 16 lanes of a ds_read_b128 group meets 16 different
// bank quads, the other one is a broadcast.  The products into the gradients run lane = column (consecutive banks) with
// the tile's p / ds as broadcast reads.  A dropped key, a key past Lk, a row past Lq and a row whose lse is -inf (no
// kept key) have p = ds = 0 exactly, so their gradient rows are exactly 0.  Gradients are written, not accumulated.
// LS = DHMAX + 4 floats is the 4 * odd row stride of an instance's widest head dim: what its LDS tiles are sized for.
__global__ void __launch_bounds__(256) k_attention_bwd_delta(const float* __restrict__ out, int64_t ldo, const float* __restrict__ dout,
                                                             int64_t lddo, float* __restrict__ delta, int64_t total, int H, int Lq,
                                                             int dh) {
  const int lane = threadIdx.x & 63;
  for (int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); idx < total; idx += (int64_t)gridDim.x * 4) {   // wave-uniform
    const int64_t bh = idx / Lq;
    const int i = (int)(idx - bh * Lq), h = (int)(bh % H);
    const int64_t row = (bh / H) * Lq + i;
    const float* o = out + row * ldo + (int64_t)h * dh;
    const float* g = dout + row * lddo + (int64_t)h * dh;
    float s = 0.f;
    for (int c = lane; c < dh; c += 64) s = fmaf(o[c], g[c], s);
    s = wave_sum(s);
    if (lane == 0) delta[idx] = s;
  }
}

// p and ds of one (QT x KT) tile from the staged rows; I_FAST: consecutive threads take consecutive query rows (the result
// is stored [key][row]), else consecutive keys ([row][key]).  p_out may be NULL.
// DROP: with m = keep / (1 - rate) of the pair (dropout_mask.h; e0 = flat index of the tile's (row 0, key 0), Lk its row
// pitch), p_out receives p m (what multiplies dO into dV) and ds = p (dp m - delta).
template <int KT, int QT, bool I_FAST, bool DROP>
__device__ __forceinline__ void attn_bwd_tile_probs(const float* qs, const float* gs, const float* ks, const float* vs, int ls, int dhp,
                                                    const float* lse2, const float* dl, const int* keep, int q_valid,
                                                    float q_scale, float* p_out, float* ds_out, const DropArgs& drop, uint64_t e0,
                                                    int Lk) {
  const float ninf = -__builtin_inff();
  for (int t = threadIdx.x; t < QT * KT; t += 256) {
    const int i = I_FAST ? t % QT : t / KT, j = I_FAST ? t / QT : t % KT;
    const float *qr = qs + i * ls, *gr = gs + i * ls, *kr = ks + j * ls, *vr = vs + j * ls;
    float s = 0.f, dp = 0.f;
    for (int c = 0; c < dhp; c += 4) {
      const float4 qq = ld4(qr + c), kk = ld4(kr + c), gg = ld4(gr + c), vv = ld4(vr + c);
      s = fmaf(qq.x, kk.x, fmaf(qq.y, kk.y, fmaf(qq.z, kk.z, fmaf(qq.w, kk.w, s))));
      dp = fmaf(gg.x, vv.x, fmaf(gg.y, vv.y, fmaf(gg.z, vv.z, fmaf(gg.w, vv.w, dp))));
    }
    const float l2 = lse2[i];
    const bool on = i < q_valid && keep[j] != 0 && l2 != ninf;
    const float p = on ? exp2f(fmaf(s, q_scale, -l2)) : 0.f;
    const int o = I_FAST ? j * QT + i : i * KT + j;
    if constexpr (DROP) {
      const float m = dropout_keep(drop.seed, drop.call, e0 + (uint64_t)i * Lk + j, drop.threshold) ? drop.scale : 0.f;
      if (p_out != nullptr) p_out[o] = p * m;
      ds_out[o] = on ? p * (dp * m - dl[i]) : 0.f;
    } else {
      if (p_out != nullptr) p_out[o] = p;
      ds_out[o] = on ? p * (dp - dl[i]) : 0.f;
    }
  }
}

// the row statistics of QT query rows from q0 on: lse in log2 units, delta; rows past Lq: -inf, 0
template <int QT>
__device__ __forceinline__ void attn_bwd_stage_stats(float* lse2, float* dl, const float* lse, const float* delta, int64_t at,
                                                     int q_valid) {
  if (threadIdx.x < QT) {
    const bool ok = (int)threadIdx.x < q_valid;
    lse2[threadIdx.x] = ok ? lse[at + threadIdx.x] * 1.44269504088896340736f : -__builtin_inff();
    dl[threadIdx.x] = ok ? delta[at + threadIdx.x] : 0.f;
  }
}

template <int KT, int QT, int DHMAX, bool DROP = false>
__global__ void __launch_bounds__(256) k_attention_bwd_dq(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                          const float* __restrict__ v, int64_t ldv, const int64_t* __restrict__ mask,
                                                          const float* __restrict__ lse, const float* __restrict__ dout, int64_t lddo,
                                                          const float* __restrict__ delta, float* __restrict__ dq, int64_t lddq, int Lq,
                                                          int Lk, int dh, float q_scale, float out_scale, int vec, DropArgs drop) {
  constexpr int LS = DHMAX + 4, RPW = QT / 4, SLOTS = DHMAX / 64;
  __shared__ __attribute__((aligned(16))) float qs[QT * LS];
  __shared__ __attribute__((aligned(16))) float gs[QT * LS];
  __shared__ __attribute__((aligned(16))) float ks[KT * LS];
  __shared__ __attribute__((aligned(16))) float vs[KT * LS];
  __shared__ __attribute__((aligned(16))) float dst[KT * QT];   // ds, [key][row]
  __shared__ float lse2[QT], dl[QT];
  __shared__ int keep[KT];
  const int b = blockIdx.z, h = blockIdx.y, H = gridDim.y, q0 = blockIdx.x * QT;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int dhp = (dh + 3) & ~3, ls = 4 * ((dhp >> 2) | 1);
  const int q_valid = Lq - q0 < QT ? Lq - q0 : QT;
  stage_rows(qs, ls, q + ((int64_t)b * Lq + q0) * ldq + (int64_t)h * dh, ldq, QT, q_valid, dh, dhp, vec != 0, 1.0f);
  stage_rows(gs, ls, dout + ((int64_t)b * Lq + q0) * lddo + (int64_t)h * dh, lddo, QT, q_valid, dh, dhp, vec != 0, 1.0f);
  attn_bwd_stage_stats<QT>(lse2, dl, lse, delta, ((int64_t)b * H + h) * Lq + q0, q_valid);
  k += (int64_t)b * Lk * ldk + (int64_t)h * dh;
  v += (int64_t)b * Lk * ldv + (int64_t)h * dh;
  if (mask != nullptr) mask += (int64_t)b * Lk;

  float acc[RPW][SLOTS];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int c = 0; c < SLOTS; ++c) acc[r][c] = 0.f;

  for (int j0 = 0; j0 < Lk; j0 += KT) {
    const int jn = Lk - j0 < KT ? Lk - j0 : KT;
    __syncthreads();   // the previous tile's K and ds have been read (first tile: nothing)
    stage_rows(ks, ls, k + j0 * ldk, ldk, KT, jn, dh, dhp, vec != 0, 1.0f);
    stage_rows(vs, ls, v + j0 * ldv, ldv, KT, jn, dh, dhp, vec != 0, 1.0f);
    if (threadIdx.x < KT) keep[threadIdx.x] = (int)threadIdx.x < jn && (mask == nullptr || mask[j0 + threadIdx.x] != 0);
    __syncthreads();
    attn_bwd_tile_probs<KT, QT, true, DROP>(qs, gs, ks, vs, ls, dhp, lse2, dl, keep, q_valid, q_scale, nullptr, dst, drop,
                                            (((uint64_t)b * H + h) * Lq + q0) * Lk + j0, Lk);
    __syncthreads();
    for (int jj = 0; jj < jn; ++jj) {
      float d[RPW];
#pragma unroll
      for (int r = 0; r < RPW; ++r) d[r] = dst[jj * QT + w * RPW + r];
      const float* kr = ks + jj * ls + lane;
#pragma unroll
      for (int c = 0; c < SLOTS; ++c)
        if (64 * c < dh) {   // uniform; a lane past dh in the last slot reads inside ks and is never stored
          const float kk = kr[64 * c];
#pragma unroll
          for (int r = 0; r < RPW; ++r) acc[r][c] = fmaf(d[r], kk, acc[r][c]);
        }
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = q0 + w * RPW + r;
    if (row >= Lq) continue;
    float* o = dq + ((int64_t)b * Lq + row) * lddq + (int64_t)h * dh;
#pragma unroll
    for (int c = 0; c < SLOTS; ++c)
      if (lane + 64 * c < dh) o[lane + 64 * c] = acc[r][c] * out_scale;
  }
}

template <int KT, int QT, int DHMAX, bool DROP = false>
__global__ void __launch_bounds__(256) k_attention_bwd_dkv(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                           const float* __restrict__ v, int64_t ldv, const int64_t* __restrict__ mask,
                                                           const float* __restrict__ lse, const float* __restrict__ dout, int64_t lddo,
                                                           const float* __restrict__ delta, float* __restrict__ dk, int64_t lddk,
                                                           float* __restrict__ dv, int64_t lddv, int Lq, int Lk, int dh, float q_scale,
                                                           float out_scale, int vec, DropArgs drop) {
  constexpr int LS = DHMAX + 4, KPW = KT / 4, SLOTS = DHMAX / 64;
  __shared__ __attribute__((aligned(16))) float qs[QT * LS];
  __shared__ __attribute__((aligned(16))) float gs[QT * LS];
  __shared__ __attribute__((aligned(16))) float ks[KT * LS];
  __shared__ __attribute__((aligned(16))) float vs[KT * LS];
  __shared__ __attribute__((aligned(16))) float ps[QT * KT];    // p, [row][key]
  __shared__ __attribute__((aligned(16))) float dss[QT * KT];   // ds, [row][key]
  __shared__ float lse2[QT], dl[QT];
  __shared__ int keep[KT];
  const int b = blockIdx.z, h = blockIdx.y, H = gridDim.y, j0 = blockIdx.x * KT;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int dhp = (dh + 3) & ~3, ls = 4 * ((dhp >> 2) | 1);
  const int jn = Lk - j0 < KT ? Lk - j0 : KT;
  stage_rows(ks, ls, k + ((int64_t)b * Lk + j0) * ldk + (int64_t)h * dh, ldk, KT, jn, dh, dhp, vec != 0, 1.0f);
  stage_rows(vs, ls, v + ((int64_t)b * Lk + j0) * ldv + (int64_t)h * dh, ldv, KT, jn, dh, dhp, vec != 0, 1.0f);
  if (threadIdx.x < KT)
    keep[threadIdx.x] = (int)threadIdx.x < jn && (mask == nullptr || mask[(int64_t)b * Lk + j0 + threadIdx.x] != 0);
  q += (int64_t)b * Lq * ldq + (int64_t)h * dh;
  dout += (int64_t)b * Lq * lddo + (int64_t)h * dh;

  float accv[KPW][SLOTS], acck[KPW][SLOTS];
#pragma unroll
  for (int r = 0; r < KPW; ++r)
#pragma unroll
    for (int c = 0; c < SLOTS; ++c) accv[r][c] = 0.f, acck[r][c] = 0.f;

  for (int q0 = 0; q0 < Lq; q0 += QT) {
    const int q_valid = Lq - q0 < QT ? Lq - q0 : QT;
    __syncthreads();   // the previous tile's Q, dO, p and ds have been read (first tile: nothing)
    stage_rows(qs, ls, q + q0 * ldq, ldq, QT, q_valid, dh, dhp, vec != 0, 1.0f);
    stage_rows(gs, ls, dout + q0 * lddo, lddo, QT, q_valid, dh, dhp, vec != 0, 1.0f);
    attn_bwd_stage_stats<QT>(lse2, dl, lse, delta, ((int64_t)b * H + h) * Lq + q0, q_valid);
    __syncthreads();
    attn_bwd_tile_probs<KT, QT, false, DROP>(qs, gs, ks, vs, ls, dhp, lse2, dl, keep, q_valid, q_scale, ps, dss, drop,
                                             (((uint64_t)b * H + h) * Lq + q0) * Lk + j0, Lk);
    __syncthreads();
    for (int i = 0; i < q_valid; ++i) {
      float pp[KPW], dd[KPW];
#pragma unroll
      for (int r = 0; r < KPW; ++r) pp[r] = ps[i * KT + w * KPW + r], dd[r] = dss[i * KT + w * KPW + r];
#pragma unroll
      for (int c = 0; c < SLOTS; ++c)
        if (64 * c < dh) {   // uniform; a lane past dh in the last slot reads inside qs / gs and is never stored
          const float gg = gs[i * ls + lane + 64 * c], qq = qs[i * ls + lane + 64 * c];
#pragma unroll
          for (int r = 0; r < KPW; ++r) {
            accv[r][c] = fmaf(pp[r], gg, accv[r][c]);
            acck[r][c] = fmaf(dd[r], qq, acck[r][c]);
          }
        }
    }
  }
#pragma unroll
  for (int r = 0; r < KPW; ++r) {
    const int key = j0 + w * KPW + r;
    if (key >= Lk) continue;
    float* ok = dk + ((int64_t)b * Lk + key) * lddk + (int64_t)h * dh;
    float* ov = dv + ((int64_t)b * Lk + key) * lddv + (int64_t)h * dh;
#pragma unroll
    for (int c = 0; c < SLOTS; ++c)
      if (lane + 64 * c < dh) {
        ok[lane + 64 * c] = acck[r][c] * out_scale;
        ov[lane + 64 * c] = accv[r][c];
      }
  }
}

// ---- launchers (AttnCall: attention_common.h; the checks are the callers') ---------------------------------------------
}  // namespace

int launch_attention(const AttnCall& c, const DropArgs* drop, hipStream_t st) {
  const int dh = c.dh;
  const bool vec = dh % 4 == 0 && c.ldq % 4 == 0 && c.ldk % 4 == 0 && c.ldv % 4 == 0 && aligned16(c.q) && aligned16(c.k) && aligned16(c.v);
  const float q_scale = 1.44269504088896340736f / sqrtf((float)dh);
  const dim3 grid((unsigned)cdiv(c.Lq, kAttnQT), (unsigned)c.H, (unsigned)c.B);
  const bool narrow = ((dh + 3) & ~3) <= 128;
  const DropArgs da = drop ? *drop : DropArgs{};
  return timed(DRIN_KC_ATTN, st, "k_attention", [&] {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, c.q, c.ldq, c.k, c.ldk, c.v, c.ldv, c.mask, c.out, c.ldo, c.lse, c.Lq, c.Lk, dh,
                         q_scale, (int)vec, da);
    };
    if (drop == nullptr)
      narrow ? go(k_attention<64>) : go(k_attention<32>);
    else
      narrow ? go(k_attention<64, true>) : go(k_attention<32, true>);
  });
}

int launch_attention_bwd_delta(const AttnCall& c, hipStream_t st) {
  const int64_t rows = (int64_t)c.B * c.H * c.Lq;
  return timed(DRIN_KC_ATTN, st, "k_attention_bwd_delta", [&] {
    const int64_t blocks = cdiv(rows, 4);
    hipLaunchKernelGGL(k_attention_bwd_delta, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, st, c.out, c.ldo,
                       c.dout, c.lddo, c.delta, rows, c.H, c.Lq, c.dh);
  });
}

int launch_attention_bwd(const AttnCall& c, const DropArgs* drop, hipStream_t st) {
  const int dh = c.dh;
  const bool vec = dh % 4 == 0 && c.ldq % 4 == 0 && c.ldk % 4 == 0 && c.ldv % 4 == 0 && c.lddo % 4 == 0 && aligned16(c.q) &&
                   aligned16(c.k) && aligned16(c.v) && aligned16(c.dout);
  const float inv_sqrt = 1.0f / sqrtf((float)dh), q_scale = 1.44269504088896340736f * inv_sqrt;
  const bool wide = ((dh + 3) & ~3) > 128;
  const int KT = wide ? 16 : 32, QT = wide ? 8 : 16;
  const DropArgs da = drop ? *drop : DropArgs{};
  DRIN_TRY(launch_attention_bwd_delta(c, st));
  if (c.dq != nullptr) {
    const dim3 grid((unsigned)cdiv(c.Lq, QT), (unsigned)c.H, (unsigned)c.B);
    DRIN_TRY(timed(DRIN_KC_ATTN, st, "k_attention_bwd_dq", [&] {
      auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, c.q, c.ldq, c.k, c.ldk, c.v, c.ldv, c.mask, c.lse, c.dout, c.lddo, c.delta,
                           c.dq, c.lddq, c.Lq, c.Lk, dh, q_scale, inv_sqrt, (int)vec, da);
      };
      if (drop == nullptr)
        !wide ? go(k_attention_bwd_dq<32, 16, 128>) : go(k_attention_bwd_dq<16, 8, 256>);
      else
        !wide ? go(k_attention_bwd_dq<32, 16, 128, true>) : go(k_attention_bwd_dq<16, 8, 256, true>);
    }));
  }
  if (c.dk == nullptr) return DRIN_OK;
  const dim3 grid((unsigned)cdiv(c.Lk, KT), (unsigned)c.H, (unsigned)c.B);
  return timed(DRIN_KC_ATTN, st, "k_attention_bwd_dkv", [&] {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, c.q, c.ldq, c.k, c.ldk, c.v, c.ldv, c.mask, c.lse, c.dout, c.lddo, c.delta, c.dk,
                         c.lddk, c.dv, c.lddv, c.Lq, c.Lk, dh, q_scale, inv_sqrt, (int)vec, da);
    };
    if (drop == nullptr)
      !wide ? go(k_attention_bwd_dkv<32, 16, 128>) : go(k_attention_bwd_dkv<16, 8, 256>);
    else
      !wide ? go(k_attention_bwd_dkv<32, 16, 128, true>) : go(k_attention_bwd_dkv<16, 8, 256, true>);
  });
}

}  // namespace drin
