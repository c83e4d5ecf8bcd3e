// The GHMFC baseline of the reference (baselines/ghmfc.py, model_type "ghmfc"), eval-mode scoring in one call: the workspace
// layout, the configuration check and drin_ghmfc_forward.  What the reference computes and how the launches are laid out:
// DESIGN.md section 15.  Every x W^T + b goes through launch_gemm_nt (the GEMM module picks the kernel); attention is the FMA
// core (attention_fma.hip), the row kernels are ghmfc_rows.hip's.  The table form (drin_ghmfc_forward_table,
// drin_ghmfc_entity_rows) shares the mention half and reads the entity side through candidate rows of a
// device-resident table (row kernels: ghmfc_table.hip).  Host code only.
#include "attention_common.h"
#include "row_checks.h"

namespace drin {
namespace {

constexpr int kChunk = 256;   // mentions per pass over the workspace

struct GhmfcLayout {
  size_t a, b, kv, pool_t, pool_v, tl, vl, men, epool, ent, total_floats;   // offsets in floats
  // form: the gathered batch of drin_ghmfc_forward | drin_ghmfc_forward_table, whose epool also takes the gathered rows of a
  // pooled table | the same scoring from per-entity rows: no entity regions
  enum Form { GATHERED, TABLE, TABLE_ROWS };
  void build(const drin_ghmfc_config& c, Form form = GATHERED) {
    const size_t Bc = c.batch < kChunk ? c.batch : kChunk, N = c.num_candidates, D = c.embed_dim, R = c.image_dim;
    const size_t L = c.mention_tokens, P = c.image_regions;
    Arena A;
    auto mx = [](size_t x, size_t y) { return x > y ? x : y; };
    const size_t rows = mx(L * D, P * R);
    a = A.take(Bc * rows), b = A.take(Bc * rows);
    kv = A.take(Bc * 2 * mx(mx(L, P) * D, mx(L, P) * R));
    pool_t = A.take(Bc * D), pool_v = A.take(Bc * R), tl = A.take(Bc * D), vl = A.take(Bc * D), men = A.take(Bc * D);
    epool = A.take(form == TABLE || (form == GATHERED && c.entity_tokens > 0) ? Bc * N * D : 0);
    ent = A.take(form != TABLE_ROWS ? Bc * N * D : 0);
    total_floats = A.total;
  }
};

int validate_ghmfc_config(const drin_ghmfc_config* c) {
  if (!c) {
    set_error("ghmfc config is NULL");
    return DRIN_E_NULL;
  }
  if (c->batch <= 0 || c->batch > (1 << 20) || c->num_candidates <= 0 || c->num_candidates > kMaxGridY || c->embed_dim <= 0 ||
      c->image_dim <= 0 || c->mention_tokens <= 0 || c->image_regions <= 0 || c->num_heads <= 0 || c->entity_tokens < 0) {
    set_error("ghmfc config: batch in [1, 2^20], num_candidates in [1, %d], widths, token counts and heads >= 1, entity_tokens >= 0 "
              "(got B=%d N=%d D=%d R=%d L=%d P=%d H=%d T=%d)", kMaxGridY, c->batch, c->num_candidates, c->embed_dim, c->image_dim,
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
  // a attends to b: separate q / k / v weights (kdim = vdim = Eb), one in_proj_bias [3 Ea]; K | V side by side
  DRIN_TRY(launch_gemm_nt({{sa, Ea}, {W.a2b_wq, Ea}, W.a2b_in_bias, A, Ea, Ma, Ea, Ea}, prec, st));
  DRIN_TRY(launch_gemm_nt({{sb, Eb}, {W.a2b_wk, Eb}, W.a2b_in_bias + Ea, KV, 2 * (int64_t)Ea, Mb, Ea, Eb}, prec, st));
  DRIN_TRY(launch_gemm_nt({{sb, Eb}, {W.a2b_wv, Eb}, W.a2b_in_bias + 2 * Ea, KV + Ea, 2 * (int64_t)Ea, Mb, Ea, Eb}, prec, st));
  DRIN_TRY(launch_attention(AttnCall{A, Ea, KV, 2 * (int64_t)Ea, KV + Ea, 2 * (int64_t)Ea, mb, Bf, Ea, nullptr, Bc, H, La, Lb, dh}, nullptr, st));
  DRIN_TRY(launch_gemm_nt({{Bf, Ea}, {W.a2b_wo, Ea}, W.a2b_bo, A, Ea, Ma, Ea, Ea}, prec, st));
  DRIN_TRY(launch_layernorm_res(A, nullptr, W.ln0_w, W.ln0_b, A, Ma, Ea, eps, st));
  DRIN_TRY(launch_gemm_nt({{A, Ea}, {W.a2b_ffn_w, Ea}, W.a2b_ffn_b, Bf, Ea, Ma, Ea, Ea}, prec, st));
  DRIN_TRY(launch_layernorm_res(Bf, A, W.ln1_w, W.ln1_b, A, Ma, Ea, eps, st));
  // the result attends to a: packed in_proj_weight [3 Ea, Ea]; K | V of seq_a are its rows Ea .. 3 Ea, ONE product
  DRIN_TRY(launch_gemm_nt({{A, Ea}, {W.b2a_in_w, Ea}, W.b2a_in_bias, Bf, Ea, Ma, Ea, Ea}, prec, st));
  DRIN_TRY(launch_gemm_nt({{sa, Ea}, {W.b2a_in_w + (int64_t)Ea * Ea, Ea}, W.b2a_in_bias + Ea, KV, 2 * (int64_t)Ea, Ma, 2 * Ea, Ea}, prec, st));
  DRIN_TRY(launch_attention(AttnCall{Bf, Ea, KV, 2 * (int64_t)Ea, KV + Ea, 2 * (int64_t)Ea, ma, A, Ea, nullptr, Bc, H, La, La, dh}, nullptr, st));
  DRIN_TRY(launch_gemm_nt({{A, Ea}, {W.b2a_wo, Ea}, W.b2a_bo, Bf, Ea, Ma, Ea, Ea}, prec, st));
  DRIN_TRY(launch_layernorm_res(Bf, nullptr, W.ln2_w, W.ln2_b, Bf, Ma, Ea, eps, st));
  DRIN_TRY(launch_gemm_nt({{Bf, Ea}, {W.b2a_ffn_w, Ea}, W.b2a_ffn_b, A, Ea, Ma, Ea, Ea}, prec, st));
  DRIN_TRY(launch_layernorm_res(A, Bf, W.ln3_w, W.ln3_b, A, Ma, Ea, eps, st));
  return launch_seq_max(A, pooled, Bc, La, Ea, st);
}

// the 52 state-dict tensors: none NULL, all 16-byte aligned
int check_ghmfc_params(const char* who, const drin_ghmfc_params* p) {
  static_assert(sizeof(drin_ghmfc_params) == 52 * sizeof(const float*), "the 52 state-dict tensors, nothing else");
  const float* const* tensors = reinterpret_cast<const float* const*>(p);
  for (int i = 0; i < 52; ++i) {
    if (!tensors[i]) {
      set_error("%s: parameter %d (state-dict order) is NULL", who, i);
      return DRIN_E_NULL;
    }
    if (!aligned16(tensors[i])) {
      set_error("%s: parameter %d (state-dict order) is not 16-byte aligned", who, i);
      return DRIN_E_ALIGN;
    }
  }
  return DRIN_OK;
}

// MultimodalFusion (ghmfc.py:141-149) of the Bc mentions from b0 on: men [Bc, D].  The mention half of drin_ghmfc_forward and
// drin_ghmfc_forward_table: one function, the same launches.  The image mask is all ones: NULL.
int mention_half(const drin_ghmfc_config& c, const drin_ghmfc_batch* bt, const drin_ghmfc_params* p, const GhmfcLayout& W, float* ws,
                 int b0, int Bc, float* men, hipStream_t st) {
  const int D = c.embed_dim, R = c.image_dim, L = c.mention_tokens, P = c.image_regions, H = c.num_heads, prec = c.precision;
  const float* text = bt->mention_feature + (int64_t)b0 * L * D;
  const int64_t* tmask = bt->mention_mask + (int64_t)b0 * L;
  const float* image = bt->mention_image + (int64_t)b0 * P * R;
  DRIN_TRY(cross_attention_max(p->t2v, text, tmask, L, D, image, nullptr, P, R, Bc, H, ws + W.a, ws + W.b, ws + W.kv, ws + W.pool_t,
                               prec, c.layer_norm_eps, st));
  DRIN_TRY(cross_attention_max(p->v2t, image, nullptr, P, R, text, tmask, L, D, Bc, H, ws + W.a, ws + W.b, ws + W.kv, ws + W.pool_v,
                               prec, c.layer_norm_eps, st));
  DRIN_TRY(launch_gemm_nt({{ws + W.pool_t, D}, {p->w_text_linear, D}, p->b_text_linear, ws + W.tl, D, Bc, D, D}, prec, st));
  DRIN_TRY(launch_gemm_nt({{ws + W.pool_v, R}, {p->w_image_linear, R}, p->b_image_linear, ws + W.vl, D, Bc, D, R}, prec, st));
  return launch_gate_mix(ws + W.tl, ws + W.vl, p->w_score_linear, p->b_score_linear, men, Bc, D, st);
}

// ---- the table form ---------------------------------------------------------------------------
constexpr int64_t kRowsChunk = 65536;   // entities per pass of drin_ghmfc_entity_rows

int check_ghmfc_table(const char* who, const drin_ghmfc_table* t, int D) {
  if (!t) {
    set_error("%s: table is NULL", who);
    return DRIN_E_NULL;
  }
  if (t->size != sizeof(drin_ghmfc_table)) {
    set_error("%s: table.size = %zu is not sizeof(drin_ghmfc_table) = %zu", who, t->size, sizeof(drin_ghmfc_table));
    return DRIN_E_SHAPE;
  }
  if (t->num_entities < 1 || t->num_entities > INT64_MAX / 4096 / D) {
    set_error("%s: table.num_entities = %lld is not in [1, %lld]", who, (long long)t->num_entities, (long long)(INT64_MAX / 4096 / D));
    return DRIN_E_SHAPE;
  }
  if (t->entity_tokens < 0 || t->entity_tokens > kAttnMaxLk) {
    set_error("%s: table.entity_tokens = %d is not in [0, %d]", who, t->entity_tokens, kAttnMaxLk);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

// the configuration the layout is built from: the call's, with the table's token count
drin_ghmfc_config table_config(const drin_ghmfc_config& cfg, const drin_ghmfc_table& t) {
  drin_ghmfc_config c = cfg;
  c.entity_tokens = t.entity_tokens;
  return c;
}

struct EntityRowsLayout {
  size_t pool, total_floats;
  void build(int64_t E, int T, int D) {
    Arena A;
    pool = A.take(T > 0 ? (size_t)(E < kRowsChunk ? E : kRowsChunk) * D : 0);
    total_floats = A.total;
  }
};

int check_entity_rows_shape(const char* who, int64_t E, int T, int D) {
  DRIN_TRY(check_width4(who, D));
  DRIN_TRY(check_count(who, "num_entities", E, 1, INT64_MAX / 4096 / D));
  return check_count(who, "entity_tokens", T, 0, kAttnMaxLk);
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

int ghmfc_table_layout_selfcheck(int batch, int n, int d, int r, int tokens, int regions, int entity_tokens, bool from_rows, int64_t E) {
  drin_ghmfc_config c = {};
  c.batch = batch, c.num_candidates = n, c.embed_dim = d, c.image_dim = r, c.mention_tokens = tokens, c.image_regions = regions;
  c.entity_tokens = entity_tokens;
  const size_t Bc = batch < kChunk ? batch : kChunk, N = n, D = d, R = r, L = tokens, P = regions;
  const size_t rows = L * D > P * R ? L * D : P * R, longest = L > P ? L : P, widest = D > R ? D : R;
  GhmfcLayout W;
  W.build(c, from_rows ? GhmfcLayout::TABLE_ROWS : GhmfcLayout::TABLE);
  // what the launches index: the mention half as above; the gathered (or pooled) rows and their products unless from_rows
  const Region ws[] = {
      {"a", W.a, Bc * rows}, {"b", W.b, Bc * rows}, {"kv", W.kv, Bc * 2 * longest * widest}, {"pool_t", W.pool_t, Bc * D},
      {"pool_v", W.pool_v, Bc * R}, {"tl", W.tl, Bc * D}, {"vl", W.vl, Bc * D}, {"men", W.men, Bc * D},
      {"epool", W.epool, from_rows ? 0 : Bc * N * D}, {"ent", W.ent, from_rows ? 0 : Bc * N * D}};
  DRIN_TRY(regions_hold("GhmfcLayout (table)", ws, (int)(sizeof(ws) / sizeof(ws[0])), W.total_floats));
  EntityRowsLayout Q;
  Q.build(E, entity_tokens, d);
  const Region qs[] = {{"pool", Q.pool, entity_tokens > 0 ? (size_t)(E < kRowsChunk ? E : kRowsChunk) * D : 0}};
  return regions_hold("EntityRowsLayout", qs, 1, Q.total_floats);
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
  DRIN_TRY(check_ghmfc_params("drin_ghmfc_forward", p));
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
  const int N = c.num_candidates, D = c.embed_dim, T = c.entity_tokens, prec = c.precision;
  // rows are independent: the chunking changes no result
  for (int b0 = 0; b0 < c.batch; b0 += kChunk) {
    const int Bc = c.batch - b0 < kChunk ? c.batch - b0 : kChunk;
    float* men = mention_repr ? mention_repr + (int64_t)b0 * D : ws + W.men;
    DRIN_TRY(mention_half(c, bt, p, W, ws, b0, Bc, men, st));
    // EntityEncoder (ghmfc.py:237-250) and the cosine (:297-298)
    const int64_t pairs = (int64_t)Bc * N;
    const float* ent_in = bt->entity_feature + (int64_t)b0 * N * D;
    if (T > 0) {
      DRIN_TRY(launch_entity_token_mean(bt->entity_feature + (int64_t)b0 * N * T * D, bt->entity_mask + (int64_t)b0 * N * T,
                                        ws + W.epool, pairs, T, D, st));
      ent_in = ws + W.epool;
    }
    DRIN_TRY(launch_gemm_nt({{ent_in, D}, {p->w_entity, D}, p->b_entity, ws + W.ent, D, pairs, D, D}, prec, st));
    DRIN_TRY(launch_cosine_rows(men, ws + W.ent, D, scores + (int64_t)b0 * N, Bc, N, D, c.cosine_eps, 1.0f, st));
  }
  return DRIN_OK;
}

// the configuration of the mention half alone: the candidate side is not the caller's to state (TABLE_ROWS: no entity regions)
static int mention_config(const drin_ghmfc_config* cfg, drin_ghmfc_config* out) {
  if (!cfg) return validate_ghmfc_config(cfg);
  *out = *cfg;
  out->num_candidates = 1, out->entity_tokens = 0;
  return validate_ghmfc_config(out);
}

size_t drin_ghmfc_mention_forward_workspace_bytes(const drin_ghmfc_config* cfg) {
  drin_ghmfc_config c;
  if (mention_config(cfg, &c) != DRIN_OK) return 0;
  GhmfcLayout W;
  W.build(c, GhmfcLayout::TABLE_ROWS);
  return W.total_floats * sizeof(float);
}

int drin_ghmfc_mention_forward(const drin_ghmfc_config* cfg, const drin_ghmfc_batch* bt, const drin_ghmfc_params* p, void* workspace,
                               size_t workspace_bytes, float* mention_repr, void* stream) {
  const char* who = "drin_ghmfc_mention_forward";
  drin_ghmfc_config c;
  DRIN_TRY(mention_config(cfg, &c));
  if (!bt || !p || !workspace || !mention_repr) {
    set_error("%s: batch / params / workspace / mention_repr is NULL", who);
    return DRIN_E_NULL;
  }
  if (!bt->mention_feature || !bt->mention_mask || !bt->mention_image) {
    set_error("%s: a mention tensor of the batch is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_ghmfc_params(who, p));
  GhmfcLayout W;
  W.build(c, GhmfcLayout::TABLE_ROWS);
  if (workspace_bytes < W.total_floats * sizeof(float)) {
    set_error("%s: workspace %zu bytes < %zu", who, workspace_bytes, W.total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  if (!aligned16(workspace) || !aligned16(bt->mention_feature) || !aligned16(bt->mention_image) || !aligned16(mention_repr)) {
    set_error("%s: workspace, feature tensors and mention_repr must be 16-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  DRIN_BIND_DEVICE(stream, mention_repr, who);
  RoctxRange range(who);
  float* ws = static_cast<float*>(workspace);
  // drin_ghmfc_forward's chunks, so every launch has that call's shape
  for (int b0 = 0; b0 < c.batch; b0 += kChunk) {
    const int Bc = c.batch - b0 < kChunk ? c.batch - b0 : kChunk;
    DRIN_TRY(mention_half(c, bt, p, W, ws, b0, Bc, mention_repr + (int64_t)b0 * c.embed_dim, (hipStream_t)stream));
  }
  return DRIN_OK;
}

size_t drin_ghmfc_table_workspace_bytes(const drin_ghmfc_config* cfg, const drin_ghmfc_table* table) {
  if (validate_ghmfc_config(cfg) != DRIN_OK || check_ghmfc_table("drin_ghmfc_table_workspace_bytes", table, cfg->embed_dim) != DRIN_OK)
    return 0;
  GhmfcLayout W;
  W.build(table_config(*cfg, *table), table->rows ? GhmfcLayout::TABLE_ROWS : GhmfcLayout::TABLE);
  return W.total_floats * sizeof(float);
}

int drin_ghmfc_forward_table(const drin_ghmfc_config* cfg, const drin_ghmfc_batch* bt, const drin_ghmfc_params* p,
                             const drin_ghmfc_table* table, void* workspace, size_t workspace_bytes, float* scores, float* mention_repr,
                             void* stream) {
  const char* who = "drin_ghmfc_forward_table";
  DRIN_TRY(validate_ghmfc_config(cfg));
  if (!bt || !p || !workspace || !scores) {
    set_error("%s: batch / params / workspace / scores is NULL", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_ghmfc_table(who, table, cfg->embed_dim));
  const drin_ghmfc_table& t = *table;
  const drin_ghmfc_config c = table_config(*cfg, t);
  if (!bt->mention_feature || !bt->mention_mask || !bt->mention_image || !t.candidates ||
      (!t.rows && (!t.text || (t.entity_tokens > 0 && !t.mask)))) {
    set_error("%s: a mention tensor, table.candidates or - without table.rows - table.text / table.mask (read when entity_tokens > 0) is NULL",
              who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_ghmfc_params(who, p));
  GhmfcLayout W;
  W.build(c, t.rows ? GhmfcLayout::TABLE_ROWS : GhmfcLayout::TABLE);
  if (workspace_bytes < W.total_floats * sizeof(float)) {
    set_error("%s: workspace %zu bytes < %zu", who, workspace_bytes, W.total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  if (!aligned16(workspace) || !aligned16(bt->mention_feature) || !aligned16(bt->mention_image) || (mention_repr && !aligned16(mention_repr)) ||
      (t.rows ? !aligned16(t.rows) : !aligned16(t.text)) || (reinterpret_cast<uintptr_t>(t.candidates) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(t.index_status) & 3u) != 0) {
    set_error("%s: workspace, feature tensors, table.text / table.rows and mention_repr must be 16-byte aligned, table.candidates 8-byte, "
              "table.index_status 4-byte", who);
    return DRIN_E_ALIGN;
  }
  DRIN_BIND_DEVICE(stream, scores, who);
  RoctxRange range(who);
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const int N = c.num_candidates, D = c.embed_dim, T = c.entity_tokens, prec = c.precision;
  for (int b0 = 0; b0 < c.batch; b0 += kChunk) {
    const int Bc = c.batch - b0 < kChunk ? c.batch - b0 : kChunk;
    float* men = mention_repr ? mention_repr + (int64_t)b0 * D : ws + W.men;
    DRIN_TRY(mention_half(c, bt, p, W, ws, b0, Bc, men, st));
    const int64_t pairs = (int64_t)Bc * N, p0 = (int64_t)b0 * N;
    const int64_t* cand = t.candidates + p0;
    if (t.rows) {   // per-entity rows (drin_ghmfc_entity_rows): the entity half is one cosine against gathered rows
      DRIN_TRY(launch_cosine_gather(men, t.rows, DRIN_FEAT_F32, cand, t.num_entities, scores + p0, Bc, N, D, c.cosine_eps, t.index_status, p0, st));
      continue;
    }
    // EntityEncoder (ghmfc.py:237-250) on the rows data.py's qid2idx gather would have delivered, and the cosine (:297-298): the
    // operands of the product and of k_cosine_rows are drin_ghmfc_forward's values in its shapes
    if (T > 0)
      DRIN_TRY(launch_entity_token_mean_indexed(t.text, t.mask, cand, t.num_entities, ws + W.epool, pairs, T, D, t.index_status, p0, st));
    else
      DRIN_TRY(launch_gather_rows(t.text, cand, t.num_entities, ws + W.epool, pairs, D, t.index_status, p0, st));
    DRIN_TRY(launch_gemm_nt({{ws + W.epool, D}, {p->w_entity, D}, p->b_entity, ws + W.ent, D, pairs, D, D}, prec, st));
    DRIN_TRY(launch_cosine_rows(men, ws + W.ent, D, scores + p0, Bc, N, D, c.cosine_eps, 1.0f, st));
  }
  return DRIN_OK;
}

size_t drin_ghmfc_entity_rows_workspace_bytes(int64_t num_entities, int32_t entity_tokens, int32_t width) {
  if (check_entity_rows_shape("drin_ghmfc_entity_rows_workspace_bytes", num_entities, entity_tokens, width) != DRIN_OK) return 0;
  EntityRowsLayout Q;
  Q.build(num_entities, entity_tokens, width);
  return Q.total_floats * sizeof(float);
}

// drin_ghmfc_entity_rows and _ex: `identity` = final_layer is nn.Identity (entity_final_layer_name "none": no weights, no product)
static int entity_rows(const char* who, const float* text, const int64_t* mask, int64_t num_entities, int32_t entity_tokens,
                       int32_t width, int32_t pooling, const float* w_entity, const float* b_entity, bool identity, int32_t precision,
                       float* rows, void* workspace, size_t workspace_bytes, void* stream) {
  const bool pooled_in_ws = entity_tokens > 0 && !identity;
  if (!text || (!identity && (!w_entity || !b_entity)) || !rows || (entity_tokens > 0 && !mask) || (pooled_in_ws && !workspace)) {
    set_error("%s: text / w_entity / b_entity / rows is NULL (mask and the workspace are read when entity_tokens > 0)", who);
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_entity_rows_shape(who, num_entities, entity_tokens, width));
  DRIN_TRY(check_entity_pooling(who, pooling));
  if (precision != DRIN_PREC_F32 && precision != DRIN_PREC_BF16X3) {
    set_error("%s: precision %d is not DRIN_PREC_F32 / DRIN_PREC_BF16X3", who, precision);
    return DRIN_E_UNSUPPORTED;
  }
  if (!aligned16(text) || !aligned16(w_entity) || !aligned16(b_entity) || !aligned16(rows) || !aligned16(workspace)) {
    set_error("%s: text, w_entity, b_entity, rows and the workspace must be 16-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  EntityRowsLayout Q;
  Q.build(num_entities, entity_tokens, width);
  if (pooled_in_ws && workspace_bytes < Q.total_floats * sizeof(float)) {
    set_error("%s: workspace %zu bytes < %zu", who, workspace_bytes, Q.total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  DRIN_BIND_DEVICE(stream, rows, who);
  RoctxRange range(who);
  hipStream_t st = (hipStream_t)stream;
  const int T = entity_tokens, D = width;
  // final_layer(pool(text[e])) (ghmfc.py:245-250) once per ENTITY instead of once per pair; entities are independent
  for (int64_t e0 = 0; e0 < num_entities; e0 += kRowsChunk) {
    const int64_t n = num_entities - e0 < kRowsChunk ? num_entities - e0 : kRowsChunk;
    const float* in = text + e0 * D;
    if (T > 0) {
      float* pool = identity ? rows + e0 * D : static_cast<float*>(workspace) + Q.pool;
      DRIN_TRY(launch_entity_token_pool(text + e0 * T * D, mask + e0 * T, pool, n, T, D, pooling, st));
      in = pool;
    }
    if (!identity) {
      DRIN_TRY(launch_gemm_nt({{in, D}, {w_entity, D}, b_entity, rows + e0 * D, D, n, D, D}, precision, st));
    } else if (T == 0 && rows != text) {   // Identity over a pooled table: the rows are the table's
      hipError_t e = hipMemcpyAsync(rows + e0 * D, in, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return hip_fail(e, "drin_ghmfc_entity_rows_ex: hipMemcpyAsync(rows)");
    }
  }
  return DRIN_OK;
}

int drin_ghmfc_entity_rows(const float* text, const int64_t* mask, int64_t num_entities, int32_t entity_tokens, int32_t width,
                           const float* w_entity, const float* b_entity, int32_t precision, float* rows, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return entity_rows("drin_ghmfc_entity_rows", text, mask, num_entities, entity_tokens, width, DRIN_POOL_AVG, w_entity, b_entity, false,
                     precision, rows, workspace, workspace_bytes, stream);
}

int drin_ghmfc_entity_rows_ex(const float* text, const int64_t* mask, int64_t num_entities, int32_t entity_tokens, int32_t width,
                              int32_t pooling, const float* w_entity, const float* b_entity, int32_t precision, float* rows,
                              void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "drin_ghmfc_entity_rows_ex";
  if (!w_entity != !b_entity) {
    set_error("%s: exactly one of w_entity / b_entity is NULL (both NULL: final_layer = Identity)", who);
    return DRIN_E_NULL;
  }
  return entity_rows(who, text, mask, num_entities, entity_tokens, width, pooling, w_entity, b_entity, !w_entity, precision, rows,
                     workspace, workspace_bytes, stream);
}
