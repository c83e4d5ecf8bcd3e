// The GHMFC baseline of the reference (baselines/ghmfc.py, model_type "ghmfc") on gfx950, eval-mode scoring only: the
// softmax-attention core, LayerNorm with a fused residual, the max over a sequence, the gated mix, and the entry points
// drin_attention / drin_ghmfc_*.  What the reference computes and how the launches are laid out: DESIGN.md section 15.
// The attention core also trains: drin_attention_train_fwd keeps the rows' log-sum-exp, drin_attention_bwd is its
// backward.  GHMFC trains on per-operation entry points: the row kernels with
// their training outputs (LayerNorm's statistics, the max's indices), their backward kernels, and attention dropout as a
// template flag of the three attention kernels (the mask function: dropout_mask.h).
//
// Every x W^T + b goes through launch_gemm_nt (the GEMM module picks the kernel); the kernels here are everything else.
// No atomics (column sums go through per-workgroup partial rows added in a fixed order), no scratch memory, at most 54 KB of
// static LDS per workgroup: the same bits every run.
#include "attention_common.h"
#include "device_utils.h"
#include "dropout_mask.h"
#include "internal.h"
#include "row_ops.h"

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
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }
// IDX (drin_seq_max_train_fwd): idx[b, c] = the LOWEST position that attains out[b, c]; when the column holds a NaN, the
// lowest NaN position (numpy.argmax's answer).  The values go through the same max_nan sequence either way: same bits.
// where(a, ia, b, ib): the position that goes with max_nan(a, b) when a sits at ia and b at ib
__device__ __forceinline__ int max_nan_pos(float a, int ia, float b, int ib) {
  const bool b_wins = b > a || (b != b && a == a);
  const bool tie = b == a || (b != b && a != a);
  return b_wins ? ib : (tie && ib < ia ? ib : ia);
}
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

template <typename F>
int timed(int cls, hipStream_t st, const char* what, F&& launch) {
  KernelTimer timer(cls, st);
  launch();
  DRIN_CHECK_LAUNCH(what);
  return DRIN_OK;
}

// ---- launchers ------------------------------------------------------------------------------------------
int launch_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const int64_t* mask,
                     float* out, int64_t ldo, int B, int H, int Lq, int Lk, int dh, hipStream_t st, float* lse = nullptr,
                     const DropArgs* drop = nullptr) {
  DRIN_TRY(check_attention_shape(B, H, Lq, Lk, dh));
  const int64_t E = (int64_t)H * dh;
  if (ldq < E || ldk < E || ldv < E || ldo < E) {
    set_error("attention: row strides (%lld, %lld, %lld, %lld) must be >= heads * head_dim = %lld", (long long)ldq, (long long)ldk,
              (long long)ldv, (long long)ldo, (long long)E);
    return DRIN_E_SHAPE;
  }
  const bool vec = dh % 4 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(v);
  const float q_scale = 1.44269504088896340736f / sqrtf((float)dh);
  const dim3 grid((unsigned)cdiv(Lq, kAttnQT), (unsigned)H, (unsigned)B);
  const bool narrow = ((dh + 3) & ~3) <= 128;
  const DropArgs da = drop ? *drop : DropArgs{};
  return timed(DRIN_KC_ATTN, st, "k_attention", [&] {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, q, ldq, k, ldk, v, ldv, mask, out, ldo, lse, Lq, Lk, dh, q_scale, (int)vec, da);
    };
    if (drop == nullptr)
      narrow ? go(k_attention<64>) : go(k_attention<32>);
    else
      narrow ? go(k_attention<64, true>) : go(k_attention<32, true>);
  });
}

}  // namespace

int launch_attention_bwd_delta(const float* out, int64_t ldo, const float* dout, int64_t lddo, float* delta, int B, int H, int Lq,
                               int dh, hipStream_t st) {
  const int64_t rows = (int64_t)B * H * Lq;
  return timed(DRIN_KC_ATTN, st, "k_attention_bwd_delta", [&] {
    const int64_t blocks = cdiv(rows, 4);
    hipLaunchKernelGGL(k_attention_bwd_delta, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, st, out, ldo, dout,
                       lddo, delta, rows, H, Lq, dh);
  });
}

namespace {
// dq may be NULL (skipped); dk and dv are both given or both NULL.  delta: [B, H, Lq] floats of scratch.
int launch_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const int64_t* mask,
                         const float* out, int64_t ldo, const float* lse, const float* dout, int64_t lddo, float* dq, int64_t lddq,
                         float* dk, int64_t lddk, float* dv, int64_t lddv, float* delta, int B, int H, int Lq, int Lk, int dh,
                         hipStream_t st, const DropArgs* drop = nullptr) {
  const bool vec = dh % 4 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && lddo % 4 == 0 && aligned16(q) && aligned16(k) &&
                   aligned16(v) && aligned16(dout);
  const float inv_sqrt = 1.0f / sqrtf((float)dh), q_scale = 1.44269504088896340736f * inv_sqrt;
  const bool wide = ((dh + 3) & ~3) > 128;
  const int KT = wide ? 16 : 32, QT = wide ? 8 : 16;
  const DropArgs da = drop ? *drop : DropArgs{};
  DRIN_TRY(launch_attention_bwd_delta(out, ldo, dout, lddo, delta, B, H, Lq, dh, st));
  if (dq != nullptr) {
    const dim3 grid((unsigned)cdiv(Lq, QT), (unsigned)H, (unsigned)B);
    DRIN_TRY(timed(DRIN_KC_ATTN, st, "k_attention_bwd_dq", [&] {
      auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, q, ldq, k, ldk, v, ldv, mask, lse, dout, lddo, delta, dq, lddq, Lq, Lk, dh,
                           q_scale, inv_sqrt, (int)vec, da);
      };
      if (drop == nullptr)
        !wide ? go(k_attention_bwd_dq<32, 16, 128>) : go(k_attention_bwd_dq<16, 8, 256>);
      else
        !wide ? go(k_attention_bwd_dq<32, 16, 128, true>) : go(k_attention_bwd_dq<16, 8, 256, true>);
    }));
  }
  if (dk == nullptr) return DRIN_OK;
  const dim3 grid((unsigned)cdiv(Lk, KT), (unsigned)H, (unsigned)B);
  return timed(DRIN_KC_ATTN, st, "k_attention_bwd_dkv", [&] {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, q, ldq, k, ldk, v, ldv, mask, lse, dout, lddo, delta, dk, lddk, dv, lddv, Lq, Lk,
                         dh, q_scale, inv_sqrt, (int)vec, da);
    };
    if (drop == nullptr)
      !wide ? go(k_attention_bwd_dkv<32, 16, 128>) : go(k_attention_bwd_dkv<16, 8, 256>);
    else
      !wide ? go(k_attention_bwd_dkv<32, 16, 128, true>) : go(k_attention_bwd_dkv<16, 8, 256, true>);
  });
}

constexpr int kLnMaxWidth = 2048;   // Row<8>
int check_row_width(const char* who, int E) {
  if (E % 4 || E <= 0 || E > kLnMaxWidth) {
    set_error("%s: width %d must be a multiple of 4 in [4, %d]", who, E, kLnMaxWidth);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}
int launch_layernorm_res(const float* x, const float* res, const float* gamma, const float* beta, float* y, int64_t rows, int E,
                         float eps, hipStream_t st, float* mean = nullptr, float* rstd = nullptr) {
  if (rows <= 0) return DRIN_OK;
  DRIN_TRY(check_row_width("layernorm_res", E));
  const int E4 = E / 4;
  const dim3 grid((unsigned)(cdiv(rows, 4) < 65535 * 16 ? cdiv(rows, 4) : 65535 * 16));
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

int launch_seq_max(const float* x, float* out, int B, int S, int E, hipStream_t st, int* idx = nullptr) {
  return timed(DRIN_KC_NORM, st, "k_seq_max", [&] {
    const dim3 grid((unsigned)cdiv(E / 4, 64), (unsigned)B);
    if (idx == nullptr)
      hipLaunchKernelGGL(k_seq_max<false>, grid, dim3(256), 0, st, x, out, idx, S, E / 4);
    else
      hipLaunchKernelGGL(k_seq_max<true>, grid, dim3(256), 0, st, x, out, idx, S, E / 4);
  });
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

int launch_gate_mix(const float* tl, const float* vl, const float* ws, const float* bs, float* out, int B, int D, hipStream_t st) {
  return timed(DRIN_KC_NORM, st, "k_gate_mix", [&] {
    hipLaunchKernelGGL(k_gate_mix, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, st, tl, vl, ws, bs, out, B, D / 4);
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

// ---- the forward pass ------------------------------------------------------------------------------------
constexpr int kChunk = 256;   // mentions per pass over the workspace

struct GhmfcLayout {
  size_t a, b, kv, pool_t, pool_v, tl, vl, men, epool, ent, total_floats;   // offsets in floats
  void build(const drin_ghmfc_config& c) {
    const size_t Bc = c.batch < kChunk ? c.batch : kChunk, N = c.num_candidates, D = c.embed_dim, R = c.image_dim;
    const size_t L = c.mention_tokens, P = c.image_regions;
    Arena A;
    auto mx = [](size_t x, size_t y) { return x > y ? x : y; };
    const size_t rows = mx(L * D, P * R);
    a = A.take(Bc * rows), b = A.take(Bc * rows);
    kv = A.take(Bc * 2 * mx(mx(L, P) * D, mx(L, P) * R));
    pool_t = A.take(Bc * D), pool_v = A.take(Bc * R), tl = A.take(Bc * D), vl = A.take(Bc * D), men = A.take(Bc * D);
    epool = A.take(c.entity_tokens > 0 ? Bc * N * D : 0), ent = A.take(Bc * N * D);
    total_floats = A.total;
  }
};

int validate_ghmfc_config(const drin_ghmfc_config* c) {
  if (!c) {
    set_error("ghmfc config is NULL");
    return DRIN_E_NULL;
  }
  if (c->batch <= 0 || c->batch > (1 << 20) || c->num_candidates <= 0 || c->num_candidates > 65535 || c->embed_dim <= 0 ||
      c->image_dim <= 0 || c->mention_tokens <= 0 || c->image_regions <= 0 || c->num_heads <= 0 || c->entity_tokens < 0) {
    set_error("ghmfc config: batch in [1, 2^20], num_candidates in [1, 65535], widths, token counts and heads >= 1, entity_tokens >= 0 "
              "(got B=%d N=%d D=%d R=%d L=%d P=%d H=%d T=%d)", c->batch, c->num_candidates, c->embed_dim, c->image_dim,
              c->mention_tokens, c->image_regions, c->num_heads, c->entity_tokens);
    return DRIN_E_SHAPE;
  }
  if (c->embed_dim % 4 || c->image_dim % 4) {
    set_error("ghmfc config: embed_dim=%d and image_dim=%d must be multiples of 4 (16-byte lane accesses)", c->embed_dim, c->image_dim);
    return DRIN_E_SHAPE;
  }
  if (c->embed_dim % c->num_heads || c->image_dim % c->num_heads) {
    set_error("ghmfc config: embed_dim=%d and image_dim=%d must be divisible by num_heads=%d", c->embed_dim, c->image_dim, c->num_heads);
    return DRIN_E_SHAPE;
  }
  if (c->embed_dim / c->num_heads > kAttnMaxDh || c->image_dim / c->num_heads > kAttnMaxDh) {
    set_error("ghmfc config: head dims %d and %d exceed %d", c->embed_dim / c->num_heads, c->image_dim / c->num_heads, kAttnMaxDh);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->mention_tokens > kAttnMaxLk || c->image_regions > kAttnMaxLk || c->entity_tokens > kAttnMaxLk) {
    set_error("ghmfc config: mention_tokens=%d, image_regions=%d and entity_tokens=%d must be <= %d", c->mention_tokens,
              c->image_regions, c->entity_tokens, kAttnMaxLk);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->embed_dim > kLnMaxWidth || c->image_dim > kLnMaxWidth) {
    set_error("ghmfc config: embed_dim=%d and image_dim=%d must be <= %d (LayerNorm keeps a row in registers)", c->embed_dim,
              c->image_dim, kLnMaxWidth);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->precision != DRIN_PREC_F32 && c->precision != DRIN_PREC_BF16X3) {
    set_error("ghmfc config: precision %d is not DRIN_PREC_F32 / DRIN_PREC_BF16X3", c->precision);
    return DRIN_E_UNSUPPORTED;
  }
  return DRIN_OK;
}

// CrossAttention(dim_a = Ea, dim_b = Eb)(seq_a, mask_a, seq_b, mask_b) followed by the max over the La positions
// (ghmfc.py:114-128, :143 / :145).  A, Bf: [Bc La, Ea] row buffers, KV: [Bc max(La, Lb), 2 Ea].  A NULL mask keeps every key.
int cross_attention_max(const drin_ghmfc_cross_params& W, const float* sa, const int64_t* ma, int La, int Ea, const float* sb,
                        const int64_t* mb, int Lb, int Eb, int Bc, int H, float* A, float* Bf, float* KV, float* pooled, int prec,
                        float eps, hipStream_t st) {
  const int64_t Ma = (int64_t)Bc * La, Mb = (int64_t)Bc * Lb;
  const int dh = Ea / H;
  auto gemm = [&](const float* x, int64_t ldx, const float* w, const float* bias, float* y, int64_t ldy, int64_t M, int N, int K) {
    return launch_gemm_nt(x, ldx, w, K, bias, y, ldy, M, N, K, false, prec, st);
  };
  // a attends to b: separate q / k / v weights (kdim = vdim = Eb), one in_proj_bias [3 Ea]; K | V side by side
  DRIN_TRY(gemm(sa, Ea, W.a2b_wq, W.a2b_in_bias, A, Ea, Ma, Ea, Ea));
  DRIN_TRY(gemm(sb, Eb, W.a2b_wk, W.a2b_in_bias + Ea, KV, 2 * (int64_t)Ea, Mb, Ea, Eb));
  DRIN_TRY(gemm(sb, Eb, W.a2b_wv, W.a2b_in_bias + 2 * Ea, KV + Ea, 2 * (int64_t)Ea, Mb, Ea, Eb));
  DRIN_TRY(launch_attention(A, Ea, KV, 2 * (int64_t)Ea, KV + Ea, 2 * (int64_t)Ea, mb, Bf, Ea, Bc, H, La, Lb, dh, st));
  DRIN_TRY(gemm(Bf, Ea, W.a2b_wo, W.a2b_bo, A, Ea, Ma, Ea, Ea));
  DRIN_TRY(launch_layernorm_res(A, nullptr, W.ln0_w, W.ln0_b, A, Ma, Ea, eps, st));
  DRIN_TRY(gemm(A, Ea, W.a2b_ffn_w, W.a2b_ffn_b, Bf, Ea, Ma, Ea, Ea));
  DRIN_TRY(launch_layernorm_res(Bf, A, W.ln1_w, W.ln1_b, A, Ma, Ea, eps, st));
  // the result attends to a: packed in_proj_weight [3 Ea, Ea]; K | V of seq_a are its rows Ea .. 3 Ea, ONE product
  DRIN_TRY(gemm(A, Ea, W.b2a_in_w, W.b2a_in_bias, Bf, Ea, Ma, Ea, Ea));
  DRIN_TRY(gemm(sa, Ea, W.b2a_in_w + (int64_t)Ea * Ea, W.b2a_in_bias + Ea, KV, 2 * (int64_t)Ea, Ma, 2 * Ea, Ea));
  DRIN_TRY(launch_attention(Bf, Ea, KV, 2 * (int64_t)Ea, KV + Ea, 2 * (int64_t)Ea, ma, A, Ea, Bc, H, La, La, dh, st));
  DRIN_TRY(gemm(A, Ea, W.b2a_wo, W.b2a_bo, Bf, Ea, Ma, Ea, Ea));
  DRIN_TRY(launch_layernorm_res(Bf, nullptr, W.ln2_w, W.ln2_b, Bf, Ma, Ea, eps, st));
  DRIN_TRY(gemm(Bf, Ea, W.b2a_ffn_w, W.b2a_ffn_b, A, Ea, Ma, Ea, Ea));
  DRIN_TRY(launch_layernorm_res(A, Bf, W.ln3_w, W.ln3_b, A, Ma, Ea, eps, st));
  return launch_seq_max(A, pooled, Bc, La, Ea, st);
}

}  // namespace

int ghmfc_layout_selfcheck(int batch, int n, int d, int r, int tokens, int regions, int entity_tokens) {
  drin_ghmfc_config c = {};
  c.batch = batch, c.num_candidates = n, c.embed_dim = d, c.image_dim = r, c.mention_tokens = tokens, c.image_regions = regions;
  c.entity_tokens = entity_tokens;
  const size_t Bc = batch < kChunk ? batch : kChunk, N = n, D = d, R = r, L = tokens, P = regions;
  const size_t rows = L * D > P * R ? L * D : P * R, longest = L > P ? L : P, widest = D > R ? D : R;
  GhmfcLayout W;
  W.build(c);
  const Region ws[] = {
      {"a", W.a, Bc * rows}, {"b", W.b, Bc * rows}, {"kv", W.kv, Bc * 2 * longest * widest}, {"pool_t", W.pool_t, Bc * D},
      {"pool_v", W.pool_v, Bc * R}, {"tl", W.tl, Bc * D}, {"vl", W.vl, Bc * D}, {"men", W.men, Bc * D},
      {"epool", W.epool, entity_tokens > 0 ? Bc * N * D : 0}, {"ent", W.ent, Bc * N * D}};
  return regions_hold("GhmfcLayout", ws, (int)(sizeof(ws) / sizeof(ws[0])), W.total_floats);
}

}  // namespace drin

using namespace drin;

int drin_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const int64_t* key_mask,
                   float* out, int64_t ldo, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim,
                   void* stream) {
  DRIN_TRY(check_attention_shape(batch, num_heads, q_len, k_len, head_dim));
  if (!q || !k || !v || !out) {
    set_error("drin_attention: q / k / v / out is NULL");
    return DRIN_E_NULL;
  }
  DRIN_BIND_DEVICE(stream, out, "drin_attention");
  return launch_attention(q, ldq, k, ldk, v, ldv, key_mask, out, ldo, batch, num_heads, q_len, k_len, head_dim, (hipStream_t)stream);
}

namespace {
int attention_train_fwd(const char* who, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                        const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch, int32_t num_heads, int32_t q_len,
                        int32_t k_len, int32_t head_dim, void* stream, const DropArgs* drop) {
  DRIN_TRY(check_attention_shape(batch, num_heads, q_len, k_len, head_dim));
  if (!q || !k || !v || !out || !lse) {
    set_error("%s: q / k / v / out / lse is NULL", who);
    return DRIN_E_NULL;
  }
  const int64_t E = (int64_t)num_heads * head_dim;
  if (ldq < E || ldk < E || ldv < E || ldo < E) {   // (launch_attention's check, ahead of the device binding: host-only)
    set_error("%s: row strides ldq, ldk, ldv, ldo (%lld, %lld, %lld, %lld) must be >= heads * head_dim = %lld", who, (long long)ldq,
              (long long)ldk, (long long)ldv, (long long)ldo, (long long)E);
    return DRIN_E_SHAPE;
  }
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_attention(q, ldq, k, ldk, v, ldv, key_mask, out, ldo, batch, num_heads, q_len, k_len, head_dim, (hipStream_t)stream,
                          lse, drop);
}

int attention_bwd(const char* who, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                  const int64_t* key_mask, const float* out, int64_t ldo, const float* lse, const float* dout, int64_t lddo, float* dq,
                  int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, float* delta_scratch, int32_t batch,
                  int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim, void* stream, const DropArgs* drop) {
  DRIN_TRY(check_attention_shape(batch, num_heads, q_len, k_len, head_dim));
  if (!q || !k || !v || !out || !lse || !dout || !delta_scratch) {
    set_error("%s: q / k / v / out / lse / dout / delta_scratch is NULL", who);
    return DRIN_E_NULL;
  }
  if ((dk == nullptr) != (dv == nullptr)) {
    set_error("%s: dk and dv are both given or both NULL (dk %s, dv %s)", who, dk ? "given" : "NULL", dv ? "given" : "NULL");
    return DRIN_E_NULL;
  }
  const int64_t E = (int64_t)num_heads * head_dim;
  const struct { const char* name; int64_t ld; bool used; } strides[] = {
      {"ldq", ldq, true}, {"ldk", ldk, true}, {"ldv", ldv, true}, {"ldo", ldo, true}, {"lddo", lddo, true},
      {"lddq", lddq, dq != nullptr}, {"lddk", lddk, dk != nullptr}, {"lddv", lddv, dv != nullptr}};
  for (const auto& s : strides)
    if (s.used && s.ld < E) {
      set_error("%s: row stride %s = %lld must be >= heads * head_dim = %lld", who, s.name, (long long)s.ld, (long long)E);
      return DRIN_E_SHAPE;
    }
  if (!dq && !dk) return DRIN_OK;
  DRIN_BIND_DEVICE(stream, delta_scratch, who);
  return launch_attention_bwd(q, ldq, k, ldk, v, ldv, key_mask, out, ldo, lse, dout, lddo, dq, lddq, dk, lddk, dv, lddv, delta_scratch,
                              batch, num_heads, q_len, k_len, head_dim, (hipStream_t)stream, drop);
}

// the row-op entry points: every pointer is read or written 16 bytes per lane
struct NamedPtr {
  const char* name;
  const void* p;
  bool required;
};
int check_pointers(const char* who, const NamedPtr* ptrs, int n) {
  for (int i = 0; i < n; ++i) {
    if (ptrs[i].required && !ptrs[i].p) {
      set_error("%s: %s is NULL", who, ptrs[i].name);
      return DRIN_E_NULL;
    }
    if (ptrs[i].p && !aligned16(ptrs[i].p)) {
      set_error("%s: %s is not 16-byte aligned", who, ptrs[i].name);
      return DRIN_E_ALIGN;
    }
  }
  return DRIN_OK;
}
#define DRIN_CHECK_POINTERS(who, ...)                                                     \
  do {                                                                                    \
    const NamedPtr _ptrs[] = {__VA_ARGS__};                                               \
    DRIN_TRY(check_pointers(who, _ptrs, (int)(sizeof(_ptrs) / sizeof(_ptrs[0]))));        \
  } while (0)
int check_count(const char* who, const char* name, int64_t v, int64_t lo, int64_t hi) {
  if (v < lo || v > hi) {
    set_error("%s: %s = %lld is not in [%lld, %lld]", who, name, (long long)v, (long long)lo, (long long)hi);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}
int check_width4(const char* who, int E) {
  if (E <= 0 || E % 4) {
    set_error("%s: width %d must be a positive multiple of 4 (16-byte lane accesses)", who, E);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}
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

int drin_attention_train_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                             const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch, int32_t num_heads,
                             int32_t q_len, int32_t k_len, int32_t head_dim, void* stream) {
  return attention_train_fwd("drin_attention_train_fwd", q, ldq, k, ldk, v, ldv, key_mask, out, ldo, lse, batch, num_heads, q_len, k_len,
                             head_dim, stream, nullptr);
}

int drin_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const int64_t* key_mask,
                       const float* out, int64_t ldo, const float* lse, const float* dout, int64_t lddo, float* dq, int64_t lddq,
                       float* dk, int64_t lddk, float* dv, int64_t lddv, float* delta_scratch, int32_t batch, int32_t num_heads,
                       int32_t q_len, int32_t k_len, int32_t head_dim, void* stream) {
  return attention_bwd("drin_attention_bwd", q, ldq, k, ldk, v, ldv, key_mask, out, ldo, lse, dout, lddo, dq, lddq, dk, lddk, dv, lddv,
                       delta_scratch, batch, num_heads, q_len, k_len, head_dim, stream, nullptr);
}

int drin_attention_dropout_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                               const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch, int32_t num_heads,
                               int32_t q_len, int32_t k_len, int32_t head_dim, float p, uint64_t seed, uint64_t call, void* stream) {
  DropArgs drop;
  bool use;
  DRIN_TRY(dropout_args("drin_attention_dropout_fwd", p, seed, call, &drop, &use));
  return attention_train_fwd("drin_attention_dropout_fwd", q, ldq, k, ldk, v, ldv, key_mask, out, ldo, lse, batch, num_heads, q_len,
                             k_len, head_dim, stream, use ? &drop : nullptr);
}

int drin_attention_dropout_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                               const int64_t* key_mask, const float* out, int64_t ldo, const float* lse, const float* dout,
                               int64_t lddo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv,
                               float* delta_scratch, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim,
                               float p, uint64_t seed, uint64_t call, void* stream) {
  DropArgs drop;
  bool use;
  DRIN_TRY(dropout_args("drin_attention_dropout_bwd", p, seed, call, &drop, &use));
  return attention_bwd("drin_attention_dropout_bwd", q, ldq, k, ldk, v, ldv, key_mask, out, ldo, lse, dout, lddo, dq, lddq, dk, lddk, dv,
                       lddv, delta_scratch, batch, num_heads, q_len, k_len, head_dim, stream, use ? &drop : nullptr);
}

int drin_attention_dropout_keep(uint64_t seed, uint64_t call, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len, float p,
                                uint8_t* keep_host) {
  const char* who = "drin_attention_dropout_keep";
  DropArgs drop;
  bool use;
  DRIN_TRY(dropout_args(who, p, seed, call, &drop, &use));
  if (batch < 1 || num_heads < 1 || q_len < 1 || k_len < 1) {
    set_error("%s: batch, heads, q_len and k_len must be >= 1 (got %d, %d, %d, %d)", who, batch, num_heads, q_len, k_len);
    return DRIN_E_SHAPE;
  }
  if (!keep_host) {
    set_error("%s: keep_host is NULL", who);
    return DRIN_E_NULL;
  }
  const uint64_t n = (uint64_t)batch * num_heads * q_len * k_len;
  for (uint64_t e = 0; e < n; ++e) keep_host[e] = dropout_keep(seed, call, e, drop.threshold) ? 1 : 0;
  return DRIN_OK;
}

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
  DRIN_TRY(check_count(who, "batch", batch, 1, 65535));
  DRIN_TRY(check_count(who, "seq_len", seq_len, 1, INT32_MAX));
  DRIN_BIND_DEVICE(stream, out, who);
  return launch_seq_max(x, out, batch, seq_len, width, (hipStream_t)stream, idx);
}

int drin_seq_max_bwd(const float* dout, const int32_t* idx, float* dx, int32_t batch, int32_t seq_len, int32_t width, void* stream) {
  const char* who = "drin_seq_max_bwd";
  DRIN_CHECK_POINTERS(who, {"dout", dout, true}, {"idx", idx, true}, {"dx", dx, true});
  DRIN_TRY(check_width4(who, width));
  DRIN_TRY(check_count(who, "batch", batch, 1, 65535));
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
  DRIN_TRY(check_count(who, "num_candidates", num_candidates, 1, 65535));
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
  DRIN_TRY(check_count(who, "num_candidates", num_candidates, 1, 65535));
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

size_t drin_ghmfc_workspace_bytes(const drin_ghmfc_config* cfg) {
  if (validate_ghmfc_config(cfg) != DRIN_OK) return 0;
  GhmfcLayout W;
  W.build(*cfg);
  return W.total_floats * sizeof(float);
}

int drin_ghmfc_forward(const drin_ghmfc_config* cfg, const drin_ghmfc_batch* bt, const drin_ghmfc_params* p, void* workspace,
                       size_t workspace_bytes, float* scores, float* mention_repr, void* stream) {
  DRIN_TRY(validate_ghmfc_config(cfg));
  if (!bt || !p || !workspace || !scores) {
    set_error("drin_ghmfc_forward: batch / params / workspace / scores is NULL");
    return DRIN_E_NULL;
  }
  const drin_ghmfc_config& c = *cfg;
  if (!bt->mention_feature || !bt->mention_mask || !bt->mention_image || !bt->entity_feature || (c.entity_tokens > 0 && !bt->entity_mask)) {
    set_error("drin_ghmfc_forward: a batch tensor is NULL (entity_mask is read when entity_tokens > 0)");
    return DRIN_E_NULL;
  }
  static_assert(sizeof(drin_ghmfc_params) == 52 * sizeof(const float*), "the 52 state-dict tensors, nothing else");
  const float* const* tensors = reinterpret_cast<const float* const*>(p);
  for (int i = 0; i < 52; ++i) {
    if (!tensors[i]) {
      set_error("drin_ghmfc_forward: parameter %d (state-dict order) is NULL", i);
      return DRIN_E_NULL;
    }
    if (!aligned16(tensors[i])) {
      set_error("drin_ghmfc_forward: parameter %d (state-dict order) is not 16-byte aligned", i);
      return DRIN_E_ALIGN;
    }
  }
  GhmfcLayout W;
  W.build(c);
  if (workspace_bytes < W.total_floats * sizeof(float)) {
    set_error("drin_ghmfc_forward: workspace %zu bytes < %zu", workspace_bytes, W.total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  if (!aligned16(workspace) || !aligned16(bt->mention_feature) || !aligned16(bt->mention_image) || !aligned16(bt->entity_feature) ||
      (mention_repr && !aligned16(mention_repr))) {
    set_error("drin_ghmfc_forward: workspace, feature tensors and mention_repr must be 16-byte aligned");
    return DRIN_E_ALIGN;
  }
  DRIN_BIND_DEVICE(stream, scores, "drin_ghmfc_forward");
  RoctxRange range("drin_ghmfc_forward");
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const int N = c.num_candidates, D = c.embed_dim, R = c.image_dim, L = c.mention_tokens, P = c.image_regions, H = c.num_heads;
  const int T = c.entity_tokens, prec = c.precision;
  // rows are independent: the chunking changes no result
  for (int b0 = 0; b0 < c.batch; b0 += kChunk) {
    const int Bc = c.batch - b0 < kChunk ? c.batch - b0 : kChunk;
    const float* text = bt->mention_feature + (int64_t)b0 * L * D;
    const int64_t* tmask = bt->mention_mask + (int64_t)b0 * L;
    const float* image = bt->mention_image + (int64_t)b0 * P * R;
    // MultimodalFusion (ghmfc.py:141-149); the image mask is all ones: NULL
    DRIN_TRY(cross_attention_max(p->t2v, text, tmask, L, D, image, nullptr, P, R, Bc, H, ws + W.a, ws + W.b, ws + W.kv, ws + W.pool_t,
                                 prec, c.layer_norm_eps, st));
    DRIN_TRY(cross_attention_max(p->v2t, image, nullptr, P, R, text, tmask, L, D, Bc, H, ws + W.a, ws + W.b, ws + W.kv, ws + W.pool_v,
                                 prec, c.layer_norm_eps, st));
    DRIN_TRY(launch_gemm_nt(ws + W.pool_t, D, p->w_text_linear, D, p->b_text_linear, ws + W.tl, D, Bc, D, D, false, prec, st));
    DRIN_TRY(launch_gemm_nt(ws + W.pool_v, R, p->w_image_linear, R, p->b_image_linear, ws + W.vl, D, Bc, D, R, false, prec, st));
    float* men = mention_repr ? mention_repr + (int64_t)b0 * D : ws + W.men;
    DRIN_TRY(launch_gate_mix(ws + W.tl, ws + W.vl, p->w_score_linear, p->b_score_linear, men, Bc, D, st));
    // EntityEncoder (ghmfc.py:237-250) and the cosine (:297-298)
    const int64_t pairs = (int64_t)Bc * N;
    const float* ent_in = bt->entity_feature + (int64_t)b0 * N * D;
    if (T > 0) {
      DRIN_TRY(launch_entity_token_mean(bt->entity_feature + (int64_t)b0 * N * T * D, bt->entity_mask + (int64_t)b0 * N * T,
                                        ws + W.epool, pairs, T, D, st));
      ent_in = ws + W.epool;
    }
    DRIN_TRY(launch_gemm_nt(ent_in, D, p->w_entity, D, p->b_entity, ws + W.ent, D, pairs, D, D, false, prec, st));
    DRIN_TRY(launch_cosine_rows(men, ws + W.ent, D, scores + (int64_t)b0 * N, Bc, N, D, c.cosine_eps, 1.0f, st));
  }
  return DRIN_OK;
}
