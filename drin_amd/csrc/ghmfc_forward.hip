// The GHMFC baseline of the reference (baselines/ghmfc.py, model_type "ghmfc"), eval-mode scoring in one call: the workspace
// layout, the configuration check and drin_ghmfc_forward.  What the reference computes and how the launches are laid out:
// DESIGN.md section 15.  Every x W^T + b goes through launch_gemm_nt (the GEMM module picks the kernel); attention is the FMA
// core (attention_fma.hip), the row kernels are ghmfc_rows.hip's.  Host code only.
#include "attention_common.h"

namespace drin {
namespace {

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
// launch_attention checks nothing, and need not here: validate_ghmfc_config has Bc in [1, kChunk], H >= 1 dividing Ea <=
// kLnMaxWidth (so H <= 65535 and dh = Ea / H >= 1), dh <= kAttnMaxDh, La and Lb in [1, kAttnMaxLk] (mention_tokens,
// image_regions), and the row strides below are Ea and 2 Ea >= H dh = Ea.
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
  DRIN_TRY(launch_attention(AttnCall{A, Ea, KV, 2 * (int64_t)Ea, KV + Ea, 2 * (int64_t)Ea, mb, Bf, Ea, nullptr, Bc, H, La, Lb, dh}, nullptr, st));
  DRIN_TRY(gemm(Bf, Ea, W.a2b_wo, W.a2b_bo, A, Ea, Ma, Ea, Ea));
  DRIN_TRY(launch_layernorm_res(A, nullptr, W.ln0_w, W.ln0_b, A, Ma, Ea, eps, st));
  DRIN_TRY(gemm(A, Ea, W.a2b_ffn_w, W.a2b_ffn_b, Bf, Ea, Ma, Ea, Ea));
  DRIN_TRY(launch_layernorm_res(Bf, A, W.ln1_w, W.ln1_b, A, Ma, Ea, eps, st));
  // the result attends to a: packed in_proj_weight [3 Ea, Ea]; K | V of seq_a are its rows Ea .. 3 Ea, ONE product
  DRIN_TRY(gemm(A, Ea, W.b2a_in_w, W.b2a_in_bias, Bf, Ea, Ma, Ea, Ea));
  DRIN_TRY(gemm(sa, Ea, W.b2a_in_w + (int64_t)Ea * Ea, W.b2a_in_bias + Ea, KV, 2 * (int64_t)Ea, Ma, 2 * Ea, Ea));
  DRIN_TRY(launch_attention(AttnCall{Bf, Ea, KV, 2 * (int64_t)Ea, KV + Ea, 2 * (int64_t)Ea, ma, A, Ea, nullptr, Bc, H, La, La, dh}, nullptr, st));
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
