// The MELHI baseline of the reference (baselines/melhi.py) on gfx950: its kernels and the entry points drin_melhi_*.
//
// What the reference computes reduces to:
//   - the image side: region mean, one Linear for the mention and the candidate images, the CLS / image cosines -> a 0/1 mask;
//   - the LSTM input X[b, t] = [mention_feature[b, t] | word[b] | mim[b]]: with W_ih = [W_tok | W_word | W_img'] the last two
//     blocks give ONE per-mention constant c[b] = W_word word + W_img' mim + b_ih + b_hh shared by every step;
//   - lstm_extract_last hands row i the TIME-0 output of the sequence one place ahead of it in torch's length order, and row
//     order[0] the last output of the sequence at sorted position c - 1 (c = number of sequences of the longest length): the
//     time-0 cells of all 2 B sequences (a zero state: no W_hh, no forget gate) plus at most ONE full recurrence per side.
// The two recurrences run side by side, one launch per step: k_lstm_step reads W_hh (4H x H fp32, 85 MB at the reference
// widths: Infinity-Cache resident) once for both lanes.  The backward pass runs the same structure in reverse, one
// k_lstm_step_bwd per step against W_hh^T, and forms dW_hh / dW_ih afterwards as GEMMs over the saved states.
// Every reduction is ordered: no atomics, the same bits every run.
#include <string.h>

#include <vector>

#include "device_utils.h"
#include "fused.h"
#include "internal.h"

namespace drin {
namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- image side -------------------------------------------------------------------------------------
// mask[b] = cos1[b] > t1 and cos2[b, n] > t2 for some n (strict: a NaN cosine is never above)
__global__ void __launch_bounds__(256) k_melhi_mask(const float* __restrict__ cos1, const float* __restrict__ cos2,
                                                    float* __restrict__ mask, int B, int N, float t1, float t2) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  bool any = false;
  for (int n = 0; n < N; ++n) any = any || cos2[(int64_t)b * N + n] > t2;
  mask[b] = (cos1[b] > t1 && any) ? 1.0f : 0.0f;
}

// x[r, :] *= mask[r / per]  (a product, as the reference's: NaN * 0 stays NaN).  grid (cdiv(D4, 256), <= 65535): rows strided
__global__ void __launch_bounds__(256) k_scale_rows(float* __restrict__ x, const float* __restrict__ mask, int64_t rows,
                                                    int per, int D4) {
  const int c4 = blockIdx.x * 256 + threadIdx.x;
  if (c4 >= D4) return;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    float* p = x + r * D4 * 4 + c4 * 4;
    st4(p, ld4(p) * mask[r / per]);
  }
}

__global__ void __launch_bounds__(256) k_bias_sum(const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// ---- time-0 inputs ------------------------------------------------------------------------------------
// Row q < B: the left sequence of mention q (first token 1, real iff start > 1); row B + b: the right one (first token
// end[b], real iff sum(mask[b]) > end[b]).  A placeholder is the reference's all-zero row: x = 0, ph = 1.  grid (2 B).
__global__ void __launch_bounds__(256) k_melhi_tok0(const float* __restrict__ mt, const int64_t* __restrict__ start,
                                                    const int64_t* __restrict__ end, const int64_t* __restrict__ mmask,
                                                    float* __restrict__ xtok0, int* __restrict__ ph, int B, int L, int D4) {
  const int q = blockIdx.x;
  const bool right = q >= B;
  const int b = right ? q - B : q;
  bool real;
  int64_t tok;
  if (!right) {
    real = start[b] > 1;
    tok = 1;
  } else {
    float cnt = 0.f;   // every wave sums the mask row itself (L int64 values, cache resident): no barrier
    for (int t = threadIdx.x & 63; t < L; t += 64) cnt += (float)mmask[(int64_t)b * L + t];
    cnt = wave_sum(cnt);
    tok = end[b];
    real = (int64_t)cnt > tok;
  }
  if (tok < 0) tok = 0;
  if (tok > L - 1) tok = L - 1;
  if (threadIdx.x == 0) ph[q] = real ? 0 : 1;
  const float* src = mt + ((int64_t)b * L + tok) * D4 * 4;
  float* dst = xtok0 + (int64_t)q * D4 * 4;
  for (int c4 = threadIdx.x; c4 < D4; c4 += 256) st4(dst + c4 * 4, real ? ld4(src + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f));
}

// the tokens of the (at most two) long recurrences: lane s, step t < T_s reads token (s == 0 ? 1 : end[j_s]) + t of mention
// j_s.  grid (cdiv(D4, 256), 2 L)
__global__ void __launch_bounds__(256) k_melhi_lane_tokens(const float* __restrict__ mt, const int64_t* __restrict__ end,
                                                           float* __restrict__ xlane, int L, int D4, int j0, int T0, int j1,
                                                           int T1) {
  const int c4 = blockIdx.x * 256 + threadIdx.x;
  const int s = blockIdx.y / L, t = blockIdx.y % L;
  if (c4 >= D4 || t >= (s ? T1 : T0)) return;
  const int j = s ? j1 : j0;
  int64_t tok = (s ? end[j] : 1) + t;
  if (tok < 0) tok = 0;
  if (tok > L - 1) tok = L - 1;
  st4(xlane + ((int64_t)s * L + t) * D4 * 4 + c4 * 4, ld4(mt + ((int64_t)j * L + tok) * D4 * 4 + c4 * 4));
}

// ---- LSTM cells (torch gate order i, f, g, o) ----------------------------------------------------------------
// time 0 of all 2 B sequences: gates = W_tok x0 (g0, in place) + (placeholder ? b_ih + b_hh : c[b]); zero state, so
// c = i g and h = o tanh(c).  Keeps the activated gates (in g0) and c for the backward pass.  grid (cdiv(H, 256), 2 B)
__global__ void __launch_bounds__(256) k_melhi_cell0(float* __restrict__ g0, const float* __restrict__ cst,
                                                     const float* __restrict__ bsum, const int* __restrict__ ph,
                                                     float* __restrict__ c0, float* __restrict__ h0, int B, int H) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= H) return;
  const int q = blockIdx.y;
  const int b = q >= B ? q - B : q;
  const int64_t G = 4 * (int64_t)H;
  const float* add = ph[q] ? bsum : cst + (int64_t)b * G;
  float* g = g0 + q * G;
  const float gi = sigmoidf_(g[k] + add[k]);
  const float gf = sigmoidf_(g[H + k] + add[H + k]);
  const float gg = tanhf(g[2 * H + k] + add[2 * H + k]);
  const float go = sigmoidf_(g[3 * H + k] + add[3 * H + k]);
  const float c = gi * gg;
  g[k] = gi, g[H + k] = gf, g[2 * H + k] = gg, g[3 * H + k] = go;
  c0[(int64_t)q * H + k] = c;
  h0[(int64_t)q * H + k] = go * tanhf(c);
}

// One step t of both long recurrences (lane s active while t < T_s).  Workgroup k owns hidden unit k: wave w forms gate row
// w H + k of W_hh h_{t-1} for both lanes (one read of the row serves both), the cell runs on two threads.  p holds the input
// projection W_tok x_t + c[j_s] and is overwritten with the activated gates.  grid (H), 256 threads.
__global__ void __launch_bounds__(256) k_lstm_step(const float* __restrict__ whh, float* __restrict__ p, float* __restrict__ cs,
                                                   float* __restrict__ hs, int H, int L, int t, int T0, int T1) {
  __shared__ float pre[4][2];
  const int k = blockIdx.x;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t G = 4 * (int64_t)H;
  float a0 = 0.f, a1 = 0.f;
  if (t > 0) {
    const float* wr = whh + ((int64_t)w * H + k) * H;
    const float* h0p = hs + ((int64_t)0 * L + t - 1) * H;
    const float* h1p = hs + ((int64_t)1 * L + t - 1) * H;
    const bool on0 = t < T0, on1 = t < T1;
    for (int c4 = lane; c4 < H / 4; c4 += 64) {
      const float4 wv = ld4(wr + c4 * 4);
      if (on0) a0 += dot4(wv, ld4(h0p + c4 * 4));
      if (on1) a1 += dot4(wv, ld4(h1p + c4 * 4));
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
  }
  if (lane == 0) pre[w][0] = a0, pre[w][1] = a1;
  __syncthreads();
  if (threadIdx.x >= 2) return;
  const int s = threadIdx.x;
  if (t >= (s ? T1 : T0)) return;
  float* g = p + ((int64_t)s * L + t) * G;
  const float gi = sigmoidf_(g[k] + pre[0][s]);
  const float gf = sigmoidf_(g[H + k] + pre[1][s]);
  const float gg = tanhf(g[2 * H + k] + pre[2][s]);
  const float go = sigmoidf_(g[3 * H + k] + pre[3][s]);
  const int64_t o = ((int64_t)s * L + t) * H + k;
  const float cprev = t > 0 ? cs[o - H] : 0.f;
  const float c = gf * cprev + gi * gg;
  g[k] = gi, g[H + k] = gf, g[2 * H + k] = gg, g[3 * H + k] = go;
  cs[o] = c;
  hs[o] = go * tanhf(c);
}

// men_in[b] = [left row | right row] by the extraction rule: src[s][b] >= 0 -> time-0 output of sequence src, else the last
// output of lane s.  grid (cdiv(H, 256), 2 B)
__global__ void __launch_bounds__(256) k_melhi_gather(const float* __restrict__ h0, const float* __restrict__ hs,
                                                      const int* __restrict__ src, float* __restrict__ men_in, int B, int H,
                                                      int L, int T0, int T1) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= H) return;
  const int q = blockIdx.y;
  const int s = q >= B ? 1 : 0, b = q - s * B;
  const int i = src[q];
  const float v = i >= 0 ? h0[((int64_t)s * B + i) * H + k] : hs[((int64_t)s * L + (s ? T1 : T0) - 1) * H + k];
  men_in[(int64_t)b * 2 * H + (int64_t)s * H + k] = v;
}

// ---- backward ------------------------------------------------------------------------------------------
// dh0[s][j] = dmen_in[recv[s][j]][s half] (the row that read sequence j's time-0 output; none for the last sorted
// position) + dmen_in[xsrc_s][s half] when j == xj_s (a side whose longest sequence has length 1: its "last output" is a
// time-0 output too).  grid (cdiv(H, 256), 2 B)
__global__ void __launch_bounds__(256) k_melhi_scatter_bwd(const float* __restrict__ dmen_in, const int* __restrict__ recv,
                                                           float* __restrict__ dh0, int B, int H, int xj0, int xsrc0, int xj1,
                                                           int xsrc1) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= H) return;
  const int q = blockIdx.y;
  const int s = q >= B ? 1 : 0, j = q - s * B;
  const int r = recv[q];
  float v = r >= 0 ? dmen_in[(int64_t)r * 2 * H + (int64_t)s * H + k] : 0.f;
  if (j == (s ? xj1 : xj0)) v += dmen_in[(int64_t)(s ? xsrc1 : xsrc0) * 2 * H + (int64_t)s * H + k];
  dh0[(int64_t)q * H + k] = v;
}

// pre-activation gradients of the time-0 cells (no forget-gate term: the previous cell state is zero).  grid (cdiv(H,256), 2B)
__global__ void __launch_bounds__(256) k_melhi_cell0_bwd(const float* __restrict__ dh0, const float* __restrict__ g0,
                                                         const float* __restrict__ c0, float* __restrict__ dg0, int H) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= H) return;
  const int64_t q = blockIdx.y, G = 4 * (int64_t)H;
  const float* g = g0 + q * G;
  const float gi = g[k], gg = g[2 * H + k], go = g[3 * H + k];
  const float dh = dh0[q * H + k];
  const float tc = tanhf(c0[q * H + k]);
  const float dc = dh * go * (1.f - tc * tc);
  float* d = dg0 + q * G;
  d[k] = dc * gg * gi * (1.f - gi);
  d[H + k] = 0.f;
  d[2 * H + k] = dc * gi * (1.f - gg * gg);
  d[3 * H + k] = dh * tc * go * (1.f - go);
}

// One step t of backpropagation through both long lanes: dh_t = W_hh^T dgates_{t+1} (+ the extracted row's gradient at the
// last step), then the cell.  dcc[s] carries dc_{t+1} f_{t+1}.  Wave w of workgroup x owns hidden unit 4 x + w and reads row
// k of W_hh^T once for both lanes.  grid (cdiv(H, 4)), 256 threads.
__global__ void __launch_bounds__(256) k_lstm_step_bwd(const float* __restrict__ whh_t, const float* __restrict__ gates,
                                                       const float* __restrict__ cs, float* __restrict__ dg,
                                                       const float* __restrict__ dlast0, const float* __restrict__ dlast1,
                                                       float* __restrict__ dcc, int H, int L, int t, int T0, int T1) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + w;
  if (k >= H) return;
  const int64_t G = 4 * (int64_t)H;
  const bool in0 = t + 1 < T0, in1 = t + 1 < T1;
  float a0 = 0.f, a1 = 0.f;
  if (in0 || in1) {
    const float* wr = whh_t + (int64_t)k * G;
    const float* d0 = dg + ((int64_t)0 * L + t + 1) * G;
    const float* d1 = dg + ((int64_t)1 * L + t + 1) * G;
    for (int c4 = lane; c4 < (int)(G / 4); c4 += 64) {
      const float4 wv = ld4(wr + c4 * 4);
      if (in0) a0 += dot4(wv, ld4(d0 + c4 * 4));
      if (in1) a1 += dot4(wv, ld4(d1 + c4 * 4));
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
  }
  if (lane >= 2) return;
  const int s = lane;
  const int T = s ? T1 : T0;
  if (t >= T) return;
  float dh = (t + 1 < T) ? (s ? a1 : a0) : 0.f;
  if (t == T - 1) dh += (s ? dlast1 : dlast0)[k];
  const float* g = gates + ((int64_t)s * L + t) * G;
  const float gi = g[k], gf = g[H + k], gg = g[2 * H + k], go = g[3 * H + k];
  const int64_t o = ((int64_t)s * L + t) * H + k;
  const float tc = tanhf(cs[o]);
  const float cprev = t > 0 ? cs[o - H] : 0.f;
  const float dc = dh * go * (1.f - tc * tc) + dcc[(int64_t)s * H + k];
  float* d = dg + ((int64_t)s * L + t) * G;
  d[k] = dc * gg * gi * (1.f - gi);
  d[H + k] = dc * cprev * gf * (1.f - gf);
  d[2 * H + k] = dc * gi * (1.f - gg * gg);
  d[3 * H + k] = dh * tc * go * (1.f - go);
  dcc[(int64_t)s * H + k] = dc * gf;
}

// gradient of the per-mention constant c[b]: the real time-0 rows of both sides plus, for the mention a long lane runs on,
// the sum over its steps (in step order).  grid (cdiv(G, 256), B)
__global__ void __launch_bounds__(256) k_melhi_dconst(const float* __restrict__ dg0, const int* __restrict__ ph,
                                                      const float* __restrict__ dgl, float* __restrict__ dcst, int B, int G,
                                                      int L, int j0, int T0, int j1, int T1) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= G) return;
  const int b = blockIdx.y;
  float v = 0.f;
  if (!ph[b]) v += dg0[(int64_t)b * G + r];
  if (!ph[B + b]) v += dg0[((int64_t)B + b) * G + r];
  if (b == j0)
    for (int t = 0; t < T0; ++t) v += dgl[((int64_t)0 * L + t) * G + r];
  if (b == j1)
    for (int t = 0; t < T1; ++t) v += dgl[((int64_t)1 * L + t) * G + r];
  dcst[(int64_t)b * G + r] = v;
}

inline dim3 row_grid(int64_t rows, int cols4) {
  return dim3((unsigned)cdiv(cols4, 256), (unsigned)(rows < kMaxGridY ? (rows > 0 ? rows : 1) : kMaxGridY));
}

// ---- host side ----------------------------------------------------------------------------------------------
constexpr int kTables = 4;   // int32 [2 B] each: src (forward gather), recv (backward scatter)

struct MelhiLayout {
  // offsets in floats into the workspace; forward (kept for backward) first, backward scratch after
  size_t mimg, mim, eim, cos1, cos2, mask, word, bsum, cst, xtok0, g0, c0, h0, xlane, p, cs, hs, men_in, men, ent, ph, src, recv;
  size_t dmen, dent, cscr, deim, dmen_in, dh0, dg0, whh_t, dgl, dcc, dcst, dmim, scratch;
  size_t scratch_floats, fwd_floats, total_floats;
  void build(const drin_melhi_config& c) {
    const size_t B = c.batch, N = c.num_candidates, D = c.embed_dim, R = c.image_dim, L = c.mention_tokens;
    const size_t H = 3 * D, G = 4 * H, BN = B * N;
    Arena A;
    mimg = A.take(B * R), mim = A.take(B * D), eim = A.take(BN * D), cos1 = A.take(B), cos2 = A.take(BN), mask = A.take(B);
    word = A.take(B * D), bsum = A.take(G), cst = A.take(B * G), xtok0 = A.take(2 * B * D), g0 = A.take(2 * B * G);
    c0 = A.take(2 * B * H), h0 = A.take(2 * B * H), xlane = A.take(2 * L * D), p = A.take(2 * L * G), cs = A.take(2 * L * H);
    hs = A.take(2 * L * H), men_in = A.take(B * 2 * H), men = A.take(B * D), ent = A.take(BN * D);
    ph = A.take(2 * B), src = A.take(2 * B), recv = A.take(2 * B);
    fwd_floats = A.total;
    dmen = A.take(B * D), dent = A.take(BN * D), cscr = A.take(3 * BN), deim = A.take(BN * D), dmen_in = A.take(B * 2 * H);
    dh0 = A.take(2 * B * H), dg0 = A.take(2 * B * G), whh_t = A.take(G * H), dgl = A.take(2 * L * G), dcc = A.take(2 * H);
    dcst = A.take(B * G), dmim = A.take(B * D);
    // slice scratch of the weight-gradient products (launch_gemm_tn deals its splits by what it is given: fixed per config)
    scratch_floats = 2 * G * H;
    scratch = A.take(scratch_floats);
    total_floats = A.total;
  }
};

int validate_melhi_config(const drin_melhi_config* c) {
  if (!c) {
    set_error("melhi config is NULL");
    return DRIN_E_NULL;
  }
  if (c->batch <= 0 || c->batch > 16384 || c->num_candidates <= 0 || c->embed_dim <= 0 || c->image_dim <= 0 ||
      c->mention_tokens < 2 || c->image_regions <= 0) {
    set_error("melhi config: batch in [1, 16384], num_candidates, embed_dim, image_dim, image_regions >= 1 and mention_tokens >= 2 "
              "(got B=%d N=%d D=%d R=%d L=%d P=%d)", c->batch, c->num_candidates, c->embed_dim, c->image_dim,
              c->mention_tokens, c->image_regions);
    return DRIN_E_SHAPE;
  }
  if (c->embed_dim % 4 || c->image_dim % 4) {
    set_error("melhi config: embed_dim=%d and image_dim=%d must be multiples of 4 (16-byte lane accesses)", c->embed_dim,
              c->image_dim);
    return DRIN_E_SHAPE;
  }
  if (c->embed_dim > 1024) {
    set_error("melhi config: embed_dim=%d > 1024 is not built (cosine backward keeps a row in registers)", c->embed_dim);
    return DRIN_E_UNSUPPORTED;
  }
  if ((int64_t)c->batch * c->num_candidates > (int64_t)1 << 30) {
    set_error("melhi config: batch * num_candidates too large for one call; split the batch");
    return DRIN_E_SHAPE;
  }
  if (c->precision != DRIN_PREC_F32 && c->precision != DRIN_PREC_BF16X3) {
    set_error("melhi config: precision %d is not DRIN_PREC_F32 / DRIN_PREC_BF16X3", c->precision);
    return DRIN_E_UNSUPPORTED;
  }
  return DRIN_OK;
}

// What the host derives from one side's order and lengths.
struct Side {
  int T;       // steps of the long recurrence: the longest length when >= 2, else 0 (its last output is a time-0 output)
  int jstar;   // the sequence at sorted position c - 1 (c = number of sequences of the longest length)
  int first;   // order[0]: the row that receives the last output
};

int melhi_sides(const drin_melhi_config& c, const int32_t* order, const int32_t* lengths, Side side[2], int32_t* tables) {
  if (!order || !lengths) {
    set_error("drin_melhi: order / lengths is NULL");
    return DRIN_E_NULL;
  }
  const int B = c.batch, L = c.mention_tokens;
  std::vector<int32_t> pos(B);
  for (int s = 0; s < 2; ++s) {
    const int32_t* o = order + (int64_t)s * B;
    const int32_t* len = lengths + (int64_t)s * B;
    const int max_len = s == 0 ? L - 1 : L;
    for (int b = 0; b < B; ++b) pos[b] = -1;
    for (int i = 0; i < B; ++i) {
      if (o[i] < 0 || o[i] >= B || pos[o[i]] >= 0) {
        set_error("drin_melhi: order[%d] is not a permutation of 0..%d (position %d: %d)", s, B - 1, i, o[i]);
        return DRIN_E_INDEX;
      }
      pos[o[i]] = i;
    }
    for (int b = 0; b < B; ++b)
      if (len[b] < 1 || len[b] > max_len) {
        set_error("drin_melhi: lengths[%d][%d] = %d outside [1, %d]", s, b, len[b], max_len);
        return DRIN_E_SHAPE;
      }
    for (int i = 1; i < B; ++i)
      if (len[o[i]] > len[o[i - 1]]) {
        set_error("drin_melhi: order[%d] is not sorted by descending length (position %d)", s, i);
        return DRIN_E_INDEX;
      }
    const int tmax = len[o[0]];
    int cnt = 0;
    while (cnt < B && len[o[cnt]] == tmax) ++cnt;
    side[s].T = tmax >= 2 ? tmax : 0;
    side[s].jstar = o[cnt - 1];
    side[s].first = o[0];
    if (tables) {
      int32_t* src = tables + (int64_t)s * B;
      int32_t* recv = tables + 2 * (int64_t)B + (int64_t)s * B;
      for (int b = 0; b < B; ++b) {
        src[b] = pos[b] > 0 ? o[pos[b] - 1] : (side[s].T ? -1 : side[s].jstar);
        recv[b] = pos[b] < B - 1 ? o[pos[b] + 1] : -1;
      }
    }
  }
  return DRIN_OK;
}

int check_ptrs(const drin_melhi_batch* bt, const drin_melhi_params* p) {
  if (!bt || !p) {
    set_error("drin_melhi: batch / params is NULL");
    return DRIN_E_NULL;
  }
  const void* need[] = {bt->mention_feature, bt->mention_mask, bt->start, bt->end, bt->mention_image, bt->entity_feature,
                        bt->entity_image, p->w_image_map_text, p->b_image_map_text, p->w_ih, p->w_hh, p->b_ih, p->b_hh,
                        p->w_mention_final_map, p->b_mention_final_map, p->w_entity_final_map, p->b_entity_final_map};
  for (const void* q : need)
    if (!q) {
      set_error("drin_melhi: a batch tensor or a parameter is NULL");
      return DRIN_E_NULL;
    }
  const void* f32[] = {bt->mention_feature, bt->mention_image, bt->entity_feature, bt->entity_image, p->w_image_map_text,
                       p->w_ih, p->w_hh, p->w_mention_final_map, p->w_entity_final_map};
  for (const void* q : f32)
    if (!aligned16(q)) {
      set_error("drin_melhi: feature and weight tensors must be 16-byte aligned");
      return DRIN_E_ALIGN;
    }
  return DRIN_OK;
}

}  // namespace

int melhi_layout_selfcheck(int batch, int n, int d, int r, int tokens) {
  drin_melhi_config c = {};
  c.batch = batch, c.num_candidates = n, c.embed_dim = d, c.image_dim = r, c.mention_tokens = tokens;
  const size_t B = batch, BN = B * n, D = d, R = r, L = tokens, H = 3 * D, G = 4 * H;
  MelhiLayout W;
  W.build(c);
  const Region fwd[] = {
      {"mimg", W.mimg, B * R}, {"mim", W.mim, B * D}, {"eim", W.eim, BN * D}, {"cos1", W.cos1, B}, {"cos2", W.cos2, BN}, {"mask", W.mask, B},
      {"word", W.word, B * D}, {"bsum", W.bsum, G}, {"cst", W.cst, B * G}, {"xtok0", W.xtok0, 2 * B * D}, {"g0", W.g0, 2 * B * G},
      {"c0", W.c0, 2 * B * H}, {"h0", W.h0, 2 * B * H}, {"xlane", W.xlane, 2 * L * D}, {"p", W.p, 2 * L * G}, {"cs", W.cs, 2 * L * H},
      {"hs", W.hs, 2 * L * H}, {"men_in", W.men_in, 2 * B * H}, {"men", W.men, B * D}, {"ent", W.ent, BN * D}, {"ph", W.ph, 2 * B},
      {"src", W.src, 2 * B}, {"recv", W.recv, 2 * B}};
  DRIN_TRY(regions_hold("MelhiLayout (forward)", fwd, (int)(sizeof(fwd) / sizeof(fwd[0])), W.fwd_floats));
  const Region bwd[] = {
      {"forward", 0, W.fwd_floats}, {"dmen", W.dmen, B * D}, {"dent", W.dent, BN * D}, {"cscr", W.cscr, 3 * BN}, {"deim", W.deim, BN * D},
      {"dmen_in", W.dmen_in, 2 * B * H}, {"dh0", W.dh0, 2 * B * H}, {"dg0", W.dg0, 2 * B * G}, {"whh_t", W.whh_t, G * H},
      {"dgl", W.dgl, 2 * L * G}, {"dcc", W.dcc, 2 * H}, {"dcst", W.dcst, B * G}, {"dmim", W.dmim, B * D}, {"scratch", W.scratch, W.scratch_floats}};
  return regions_hold("MelhiLayout", bwd, (int)(sizeof(bwd) / sizeof(bwd[0])), W.total_floats);
}

}  // namespace drin

using namespace drin;

size_t drin_melhi_workspace_bytes(const drin_melhi_config* cfg, int for_training) {
  if (validate_melhi_config(cfg) != DRIN_OK) return 0;
  MelhiLayout W;
  W.build(*cfg);
  return (for_training ? W.total_floats : W.fwd_floats) * sizeof(float);
}

int drin_melhi_forward(const drin_melhi_config* cfg, const drin_melhi_batch* bt, const drin_melhi_params* p,
                       const int32_t* order, const int32_t* lengths, void* workspace, size_t workspace_bytes, float* scores,
                       void* stream) {
  DRIN_TRY(validate_melhi_config(cfg));
  DRIN_TRY(check_ptrs(bt, p));
  if (!workspace || !scores) {
    set_error("drin_melhi_forward: workspace / scores is NULL");
    return DRIN_E_NULL;
  }
  const drin_melhi_config& c = *cfg;
  MelhiLayout W;
  W.build(c);
  if (workspace_bytes < W.fwd_floats * sizeof(float)) {
    set_error("drin_melhi_forward: workspace %zu bytes < %zu", workspace_bytes, W.fwd_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  if (!aligned16(workspace)) {
    set_error("drin_melhi_forward: workspace must be 16-byte aligned");
    return DRIN_E_ALIGN;
  }
  const int B = c.batch, N = c.num_candidates, D = c.embed_dim, R = c.image_dim, L = c.mention_tokens, P = c.image_regions;
  const int H = 3 * D, G = 4 * H, prec = c.precision;
  const int64_t BN = (int64_t)B * N;
  Side side[2];
  thread_local std::vector<int32_t> tables;
  tables.resize((size_t)kTables * B);
  DRIN_TRY(melhi_sides(c, order, lengths, side, tables.data()));
  DRIN_BIND_DEVICE(stream, scores, "drin_melhi_forward");
  RoctxRange range("drin_melhi_forward");
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  int* src = reinterpret_cast<int*>(ws + W.src);
  int* recv = reinterpret_cast<int*>(ws + W.recv);
  int* ph = reinterpret_cast<int*>(ws + W.ph);
  // the gather / scatter tables (pageable source: the runtime has consumed it when the call returns)
  hipError_t e = hipMemcpyAsync(src, tables.data(), sizeof(int32_t) * 2 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(recv, tables.data() + 2 * B, sizeof(int32_t) * 2 * B, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "drin_melhi_forward: hipMemcpyAsync(tables)");

  // image side: region mean, the image Linear on the mention and the candidates, the two cosines, the mask
  DRIN_TRY(launch_axis_mean(bt->mention_image, ws + W.mimg, B, P, R, st));
  DRIN_TRY(launch_gemm_nt({{ws + W.mimg, R}, {p->w_image_map_text, R}, p->b_image_map_text, ws + W.mim, D, B, D, R}, prec, st));
  DRIN_TRY(launch_gemm_nt({{bt->entity_image, R}, {p->w_image_map_text, R}, p->b_image_map_text, ws + W.eim, D, BN, D, R}, prec, st));
  DRIN_TRY(launch_cosine_rows(ws + W.mim, bt->mention_feature, (int64_t)L * D, ws + W.cos1, B, 1, D, c.cosine_eps, 1.0f, st));
  DRIN_TRY(launch_cosine_rows(ws + W.mimg, bt->entity_image, R, ws + W.cos2, B, N, R, c.cosine_eps, 1.0f, st));
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_mask", [&] {
    hipLaunchKernelGGL(k_melhi_mask, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, ws + W.cos1, ws + W.cos2, ws + W.mask, B, N,
                       c.thres_tmim, c.thres_imie);
  }));
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_scale_rows", [&] {
    hipLaunchKernelGGL(k_scale_rows, row_grid(B, D / 4), dim3(256), 0, st, ws + W.mim, ws + W.mask, (int64_t)B, 1, D / 4);
    hipLaunchKernelGGL(k_scale_rows, row_grid(BN, D / 4), dim3(256), 0, st, ws + W.eim, ws + W.mask, BN, N, D / 4);
  }));
  // the per-mention constant c[b] = W_word word + W_img' mim + b_ih + b_hh
  DRIN_TRY(launch_span_mean(bt->mention_feature, bt->start, bt->end, ws + W.word, B, L, D, st));
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_bias_sum", [&] {
    hipLaunchKernelGGL(k_bias_sum, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, st, p->b_ih, p->b_hh, ws + W.bsum, G);
  }));
  DRIN_TRY(launch_gemm_nt({{ws + W.word, D}, {p->w_ih + D, H}, ws + W.bsum, ws + W.cst, G, B, G, D}, prec, st));
  DRIN_TRY(launch_gemm_nt(NtProduct{{ws + W.mim, D}, {p->w_ih + 2 * D, H}, nullptr, ws + W.cst, G, B, G, D}.adding(), prec, st));
  // time-0 cells of all 2 B sequences
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_tok0", [&] {
    hipLaunchKernelGGL(k_melhi_tok0, dim3((unsigned)(2 * B)), dim3(256), 0, st, bt->mention_feature, bt->start, bt->end,
                       bt->mention_mask, ws + W.xtok0, ph, B, L, D / 4);
  }));
  DRIN_TRY(launch_gemm_nt({{ws + W.xtok0, D}, {p->w_ih, H}, nullptr, ws + W.g0, G, 2 * (int64_t)B, G, D}, prec, st));
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_cell0", [&] {
    hipLaunchKernelGGL(k_melhi_cell0, dim3((unsigned)cdiv(H, 256), (unsigned)(2 * B)), dim3(256), 0, st, ws + W.g0, ws + W.cst,
                       ws + W.bsum, ph, ws + W.c0, ws + W.h0, B, H);
  }));
  // the long recurrences: input projections in one GEMM per lane, then one launch per step for both lanes
  const int T0 = side[0].T, T1 = side[1].T;
  if (T0 || T1) {
    DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_lane_tokens", [&] {
      hipLaunchKernelGGL(k_melhi_lane_tokens, dim3((unsigned)cdiv(D / 4, 256), (unsigned)(2 * L)), dim3(256), 0, st,
                         bt->mention_feature, bt->end, ws + W.xlane, L, D / 4, side[0].jstar, T0, side[1].jstar, T1);
    }));
    for (int s = 0; s < 2; ++s)
      if (side[s].T)
        DRIN_TRY(launch_gemm_nt({{ws + W.xlane + (size_t)s * L * D, D}, {p->w_ih, H}, ws + W.cst + (size_t)side[s].jstar * G,
                                 ws + W.p + (size_t)s * L * G, G, side[s].T, G, D}, prec, st));
    const int steps = T0 > T1 ? T0 : T1;
    for (int t = 0; t < steps; ++t)
      DRIN_TRY(timed(DRIN_KC_LSTM, st, "k_lstm_step", [&] {
        hipLaunchKernelGGL(k_lstm_step, dim3((unsigned)H), dim3(256), 0, st, p->w_hh, ws + W.p, ws + W.cs, ws + W.hs, H, L, t, T0, T1);
      }));
  }
  // outputs: the extraction rule, the two final maps, the cosine head
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_gather", [&] {
    hipLaunchKernelGGL(k_melhi_gather, dim3((unsigned)cdiv(H, 256), (unsigned)(2 * B)), dim3(256), 0, st, ws + W.h0, ws + W.hs, src,
                       ws + W.men_in, B, H, L, T0, T1);
  }));
  DRIN_TRY(launch_gemm_nt({{ws + W.men_in, 2 * H}, {p->w_mention_final_map, 2 * H}, p->b_mention_final_map, ws + W.men, D, B, D, 2 * H}, prec, st));
  DRIN_TRY(launch_gemm_nt({{bt->entity_feature, D}, {p->w_entity_final_map, 2 * D}, p->b_entity_final_map, ws + W.ent, D, BN, D, D}, prec, st));
  DRIN_TRY(launch_gemm_nt(NtProduct{{ws + W.eim, D}, {p->w_entity_final_map + D, 2 * D}, nullptr, ws + W.ent, D, BN, D, D}.adding(), prec, st));
  DRIN_TRY(launch_cosine_rows(ws + W.men, ws + W.ent, D, scores, B, N, D, c.cosine_eps, 1.0f, st));
  return DRIN_OK;
}

int drin_melhi_backward(const drin_melhi_config* cfg, const drin_melhi_batch* bt, const drin_melhi_params* p,
                        const int32_t* order, const int32_t* lengths, void* workspace, size_t workspace_bytes,
                        const float* grad_scores, const drin_melhi_param_grads* gr, void* stream) {
  DRIN_TRY(validate_melhi_config(cfg));
  DRIN_TRY(check_ptrs(bt, p));
  if (!workspace || !grad_scores || !gr) {
    set_error("drin_melhi_backward: workspace / grad_scores / grads is NULL");
    return DRIN_E_NULL;
  }
  const drin_melhi_config& c = *cfg;
  MelhiLayout W;
  W.build(c);
  if (workspace_bytes < W.total_floats * sizeof(float)) {
    set_error("drin_melhi_backward: workspace %zu bytes < %zu (drin_melhi_workspace_bytes(cfg, 1))", workspace_bytes,
              W.total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  if (!aligned16(workspace)) {
    set_error("drin_melhi_backward: workspace must be 16-byte aligned");
    return DRIN_E_ALIGN;
  }
  float* const outs[] = {gr->w_image_map_text, gr->b_image_map_text, gr->w_ih, gr->w_hh, gr->b_ih, gr->b_hh,
                         gr->w_mention_final_map, gr->b_mention_final_map, gr->w_entity_final_map, gr->b_entity_final_map};
  for (float* q : outs)
    if (q && !aligned16(q)) {
      set_error("drin_melhi_backward: gradient buffers must be 16-byte aligned");
      return DRIN_E_ALIGN;
    }
  Side side[2];
  DRIN_TRY(melhi_sides(c, order, lengths, side, nullptr));
  DRIN_BIND_DEVICE(stream, grad_scores, "drin_melhi_backward");
  RoctxRange range("drin_melhi_backward");
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const int B = c.batch, N = c.num_candidates, D = c.embed_dim, R = c.image_dim, L = c.mention_tokens;
  const int H = 3 * D, G = 4 * H, prec = c.precision;
  const int64_t BN = (int64_t)B * N;
  const int T0 = side[0].T, T1 = side[1].T;
  const GemmScratch scr{ws + W.scratch, W.scratch_floats};
  const int* ph = reinterpret_cast<const int*>(ws + W.ph);
  const int* recv = reinterpret_cast<const int*>(ws + W.recv);
  auto colsum = [&](const float* x, float* out, int64_t rows, int C) {
    if (!out || rows <= 0) return (int)DRIN_OK;
    return launch_colsum(x, out, rows, C, st, scr.p, scr.floats);
  };

  // cosine head
  DRIN_TRY(launch_cosine_bwd(ws + W.men, ws + W.ent, grad_scores, ws + W.dmen, ws + W.dent, ws + W.cscr, B, N, D, c.cosine_eps, st));
  // entity_final_map over [entity_feature | eim]
  DRIN_TRY(launch_gemm_tn({{ws + W.dent, D}, {bt->entity_feature, D}, gr->w_entity_final_map, 2 * D, BN, D, D}, prec, st, scr));
  DRIN_TRY(launch_gemm_tn({{ws + W.dent, D}, {ws + W.eim, D}, gr->w_entity_final_map ? gr->w_entity_final_map + D : nullptr, 2 * D, BN, D, D}, prec, st, scr));
  DRIN_TRY(colsum(ws + W.dent, gr->b_entity_final_map, BN, D));
  const bool want_img = gr->w_image_map_text || gr->b_image_map_text;
  if (want_img) {
    DRIN_TRY(launch_gemm_nn({{ws + W.dent, D}, {p->w_entity_final_map + D, 2 * D}, ws + W.deim, D, BN, D, D}, prec, st));
    DRIN_TRY(timed(DRIN_KC_CELL, st, "k_scale_rows", [&] {
      hipLaunchKernelGGL(k_scale_rows, row_grid(BN, D / 4), dim3(256), 0, st, ws + W.deim, ws + W.mask, BN, N, D / 4);
    }));
    DRIN_TRY(launch_gemm_tn({{ws + W.deim, D}, {bt->entity_image, R}, gr->w_image_map_text, R, BN, D, R}, prec, st, scr));
    DRIN_TRY(colsum(ws + W.deim, gr->b_image_map_text, BN, D));
  }
  // mention_final_map over [left | right]
  DRIN_TRY(launch_gemm_tn({{ws + W.dmen, D}, {ws + W.men_in, 2 * H}, gr->w_mention_final_map, 2 * H, B, D, 2 * H}, prec, st, scr));
  DRIN_TRY(colsum(ws + W.dmen, gr->b_mention_final_map, B, D));
  const bool want_lstm = gr->w_ih || gr->w_hh || gr->b_ih || gr->b_hh || want_img;
  if (!want_lstm) return DRIN_OK;
  DRIN_TRY(launch_gemm_nn({{ws + W.dmen, D}, {p->w_mention_final_map, 2 * H}, ws + W.dmen_in, 2 * H, B, 2 * H, D}, prec, st));
  // the extraction rule backwards, then the time-0 cells
  const int xj0 = T0 ? -1 : side[0].jstar, xj1 = T1 ? -1 : side[1].jstar;
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_scatter_bwd", [&] {
    hipLaunchKernelGGL(k_melhi_scatter_bwd, dim3((unsigned)cdiv(H, 256), (unsigned)(2 * B)), dim3(256), 0, st, ws + W.dmen_in, recv,
                       ws + W.dh0, B, H, xj0, side[0].first, xj1, side[1].first);
  }));
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_cell0_bwd", [&] {
    hipLaunchKernelGGL(k_melhi_cell0_bwd, dim3((unsigned)cdiv(H, 256), (unsigned)(2 * B)), dim3(256), 0, st, ws + W.dh0, ws + W.g0,
                       ws + W.c0, ws + W.dg0, H);
  }));
  // backpropagation through time over the long lanes
  if (T0 || T1) {
    DRIN_TRY(launch_transpose(p->w_hh, ws + W.whh_t, G, H, st));
    hipError_t e = hipMemsetAsync(ws + W.dcc, 0, sizeof(float) * 2 * H, st);
    if (e != hipSuccess) return hip_fail(e, "drin_melhi_backward: hipMemsetAsync");
    const float* dlast0 = ws + W.dmen_in + (size_t)side[0].first * 2 * H;
    const float* dlast1 = ws + W.dmen_in + (size_t)side[1].first * 2 * H + H;
    const int steps = T0 > T1 ? T0 : T1;
    for (int t = steps - 1; t >= 0; --t)
      DRIN_TRY(timed(DRIN_KC_LSTM, st, "k_lstm_step_bwd", [&] {
        hipLaunchKernelGGL(k_lstm_step_bwd, dim3((unsigned)cdiv(H, 4)), dim3(256), 0, st, ws + W.whh_t, ws + W.p, ws + W.cs,
                           ws + W.dgl, dlast0, dlast1, ws + W.dcc, H, L, t, T0, T1);
      }));
  }
  // weight gradients over the saved states
  for (int s = 0; s < 2; ++s)
    if (side[s].T >= 2)
      DRIN_TRY(launch_gemm_tn({{ws + W.dgl + ((size_t)s * L + 1) * G, G}, {ws + W.hs + (size_t)s * L * H, H}, gr->w_hh, H, side[s].T - 1, G, H},
                              prec, st, scr));
  DRIN_TRY(launch_gemm_tn({{ws + W.dg0, G}, {ws + W.xtok0, D}, gr->w_ih, H, 2 * (int64_t)B, G, D}, prec, st, scr));
  for (int s = 0; s < 2; ++s)
    if (side[s].T)
      DRIN_TRY(launch_gemm_tn({{ws + W.dgl + (size_t)s * L * G, G}, {ws + W.xlane + (size_t)s * L * D, D}, gr->w_ih, H, side[s].T, G, D}, prec, st, scr));
  DRIN_TRY(timed(DRIN_KC_CELL, st, "k_melhi_dconst", [&] {
    hipLaunchKernelGGL(k_melhi_dconst, dim3((unsigned)cdiv(G, 256), (unsigned)B), dim3(256), 0, st, ws + W.dg0, ph, ws + W.dgl,
                       ws + W.dcst, B, G, L, side[0].jstar, T0, side[1].jstar, T1);
  }));
  if (gr->w_ih) {
    DRIN_TRY(launch_gemm_tn({{ws + W.dcst, G}, {ws + W.word, D}, gr->w_ih + D, H, B, G, D}, prec, st, scr));
    DRIN_TRY(launch_gemm_tn({{ws + W.dcst, G}, {ws + W.mim, D}, gr->w_ih + 2 * D, H, B, G, D}, prec, st, scr));
  }
  float* const dbias[2] = {gr->b_ih, gr->b_hh};   // both biases enter every gate sum once
  for (float* db : dbias) {
    DRIN_TRY(colsum(ws + W.dg0, db, 2 * (int64_t)B, G));
    for (int s = 0; s < 2; ++s)
      if (side[s].T) DRIN_TRY(colsum(ws + W.dgl + (size_t)s * L * G, db, side[s].T, G));
  }
  if (want_img) {
    // mim enters the constant through W_img' (and the mask, which carries no gradient)
    DRIN_TRY(launch_gemm_nn({{ws + W.dcst, G}, {p->w_ih + 2 * D, H}, ws + W.dmim, D, B, D, G}, prec, st));
    DRIN_TRY(timed(DRIN_KC_CELL, st, "k_scale_rows", [&] {
      hipLaunchKernelGGL(k_scale_rows, row_grid(B, D / 4), dim3(256), 0, st, ws + W.dmim, ws + W.mask, (int64_t)B, 1, D / 4);
    }));
    DRIN_TRY(launch_gemm_tn({{ws + W.dmim, D}, {ws + W.mimg, R}, gr->w_image_map_text, R, B, D, R}, prec, st, scr));
    DRIN_TRY(colsum(ws + W.dmim, gr->b_image_map_text, B, D));
  }
  return DRIN_OK;
}
