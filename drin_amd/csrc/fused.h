// Argument blocks and launch wrappers of the fused two-layer inference pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/drin_hip.h"
#include "gemm.h"
#include "layout.h"

namespace drin {

// Layout of the caller-owned buffer drin_prepare fills (weight-only products, offsets in floats).
struct Prepared {  // offsets in floats
  size_t wcat1, bcat1, ecat, etmp, k_t, k_i, c_txt, c_img, cb_t, cb_i, total;
  size_t p_ctxt, p_cimg, p_wh2;  // bf16 (hi, lo) planes of the three pair-sized GEMM weights; lo follows hi
  size_t p_wmt, p_wmi, p_wcat1, p_ecat, p_wet, p_wei, p_wh1;  // the same for the mention-sized GEMM weights
  size_t p_cimg_f16;             // W_h1 W_ei as ONE fp16 plane [D, R] under one power-of-two scale (DRIN_PREC_BF16X3_IF16)
  size_t cimg_f16_scale;         // [2]: that scale, and the scratch word of its reduction
  void build(const drin_config& c) {
    const size_t D = c.embed_dim, R = c.image_dim;
    Arena A;
    wcat1 = A.take(2 * D * D);      // [W_h1; W_u1]           [2D, D]
    bcat1 = A.take(2 * D);          // [0; b_u1]
    ecat = A.take(D * (D + R));     // ([W_v1 W_et | W_v1 W_ei])^T  [D + R, D]  (nn.Linear layout: q = fu ecat^T)
    etmp = A.take(D * (D + R));     // scratch of drin_prepare: the un-transposed product
    k_t = A.take(D);                // W_v1 b_et + b_v1
    k_i = A.take(D);                // W_v1 b_ei + b_v1
    c_txt = A.take(D * D);          // W_h1 W_et              [D, D]
    c_img = A.take(D * R);          // W_h1 W_ei              [D, R]
    cb_t = A.take(D);               // W_h1 b_et + b_h1
    cb_i = A.take(D);               // W_h1 b_ei + b_h1
    p_ctxt = A.take(D * D);         // hi plane D*D bf16 (= D*D/2 floats) then lo plane
    p_cimg = A.take(D * R);
    p_wh2 = A.take(D * D);
    p_wmt = A.take(D * D);          // W_mt
    p_wmi = A.take(D * R);          // W_mi
    p_wcat1 = A.take(2 * D * D);    // [W_h1; W_u1]
    p_ecat = A.take(D * (D + R));   // ([W_v1 W_et | W_v1 W_ei])^T
    p_wet = A.take(D * D);          // W_et
    p_wei = A.take(D * R);          // W_ei
    p_wh1 = A.take(D * D);          // W_h1
    p_cimg_f16 = A.take(D * R / 2 + 2);   // D R halves
    cimg_f16_scale = A.take(2);
    total = A.total;
  }
};

// DRIN_OK when `c` can take the folded two-layer pipelines (fused_forward.hip, entity_cache.hip)
int fused_supported(const drin_config* c);
// split-bf16 widths of every product of the folded paths (DRIN_PREC_BF16X3_IF16 differs in the image contraction's passes only)
inline int folded_precision(const drin_config* c) { return c->precision == DRIN_PREC_BF16X3_IF16 ? (int)DRIN_PREC_BF16X3 : c->precision; }
// "the pair-sized contractions of the folded paths run on bf16 planes", as far as the precision says: what the two layouts size
// their plane regions by.  A call uses them where the widths allow it too (nt_planes_width) and refuses or falls back otherwise.
inline bool folded_planes(const drin_config& c) { return split_bf16(folded_precision(&c)); }
// workgroups (candidate chunks) per mention of the per-entity-cache path's kernels for this call (entity_cache.hip)
int cached_chunks_per_mention(const drin_config& c);

struct StreamArgs {
  // batch (entity side) - device pointers into the caller's tensors
  const void* entity_text;           // TOKENS: [M, T, D]   else [M, D]     (fp32, or bf16 when bf16_features)
  const int64_t* entity_mask;        // TOKENS: [M, T]
  const void* entity_image;          // [M, R]
  const void* entity_object;         // [M, Ke, R]
  const float* entity_object_score;  // [M, Ke]
  const int64_t* entity_index;       // optional [M]: entity_* above are tables, pair p reads row entity_index[p]
  int64_t num_entities;
  int32_t* index_status;             // optional int32[4]: where a clamped entity_index is reported (drin_batch.index_status)
  const float* miet;                 // [M]
  const float* mtei;                 // [M]
  // mention side
  const float* span_mean;            // [B, D]
  const void* mobj;                  // [B, Km, R]   (fp32 / bf16 like the entity features)
  const float* mscore;               // [B, Km]
  const float* fu;                   // rows b and B + b, row stride ldfu: W_u(mt0), W_u(mi0)  (dynamic edges only)
  const float* q;                    // [2 B][ldq]  fu * [W_v W_et | W_v W_ei]     (dynamic edges only)
  const float* k_t;                  // [D]  W_v b_et + b_v
  const float* k_i;                  // [D]  W_v b_ei + b_v
  // outputs
  float* xt_out;                     // TOKENS: pooled entity text [M, D] (NULL when only the planes are wanted)
  void* xt_hi;                       // optional bf16 hi / lo planes of the entity text GEMM operand [M, D]
  void* xt_lo;
  void* xi_hi;                       // optional bf16 hi / lo planes of the entity image rows [M, R]
  void* xi_lo;
  float* xi_scale;                   // optional [M]: 2^ceil(log2 max |image row|) per pair (1 for an all-zero row) - DRIN_PREC_BF16X3_IF16 -
  void* xi_f16;                      //   and with it [M, R] fp16: the image row divided by that scale (the one plane of its contraction)
  float* e0m;                        // [4][M] layer-1 edges (already multiplied by the edge switch)
  float* e1m;                        // [4][M] layer-2 edges (ditto)
  float* s_part;                     // [B][chunks][2 D + 2 R + 4]
  float* s_text;                     // chunks == 1 only: [2][B][D] (S_tt, S_it), [2][B][R] (S_ti, S_ii), [4][B] edge sums,
  float* s_img;                      //   written directly in the layout k_reduce_stream_partials would produce
  float* sig;
  int B, N, D4, R4, T, Km, Ke, chunks, ldq, ldfu, dynamic, bf16_features;
  int act_e;                         // drin_activation of the edges, resolved (DRIN_ACT_SIGMOID by default)
  float mask[4];
  float cos_eps, miei_eps, clip;
};

struct PairArgs {
  const float* h_text;   // [M, D]  X_t (W_h W_et)^T
  const float* h_image;  // [M, D]  X_i (W_h W_ei)^T
  const float* hm;       // rows b and B + b, row stride ldhm: W_h mt0, W_h mi0 (no bias)
  const float* c_t;      // [D]  W_h b_et + b_h
  const float* c_i;      // [D]  W_h b_ei + b_h
  const float* gamma;
  const float* beta;
  const float* e0m;
  const float* e1m;
  float* et1;            // [M, D]  (NULL when only the planes are wanted)
  void* et1_hi;          // optional bf16 hi / lo planes of et1
  void* et1_lo;
  float* s2_part;        // [B][chunks][2 D]
  int B, N, D4, chunks, ldhm;
  int act_v;             // drin_activation of the vertices, resolved (DRIN_ACT_GELU by default)
  float ln_eps;
};

struct FinalArgs {
  const float* h2;       // [M, D]  et1 W_h2^T
  const float* hm2;      // [2][B][D]  W_h2 mt1, W_h2 mi1 (no bias)
  const float* b_h2;
  const float* gamma;
  const float* beta;
  const float* e1m;
  const float* mt2;      // [B, D]
  float* scores;         // [M]
  int B, N, D4, chunks;
  int act_v;             // drin_activation of the vertices, resolved
  float ln_eps, cos_eps;
};

// ---- which width band a family's launcher takes (drin_width_class) ----------------------------------------------------------------
// Every width-templated kernel of the folded and cached paths is built in three forms: `tiny` (one float4 per lane in every slot the
// family has), `exact` (D = 768 and, where the family reads image rows, R = 2048: every lane of every slot full, widths compile-time
// constants) and `guarded` (the exact form's register slots with `c4 < D4` guards: part of the lanes, or whole slots, hold nothing).
// Each family's choice is made HERE, once: its launcher switches on the result and drin_width_class exports it, so a test asks the
// dispatch which form a shape takes instead of restating the gates (the argument of the GEMM route record, gemm.h) - a pure
// function of the widths is enough, no per-thread record.  D4 / R4: widths in float4 quads.
constexpr int kTinyQuads = 64;                        // one quad per lane of a wave
constexpr int kExactTextQuads = 192, kExactImageQuads = 512;   // D = 768 (three slots), R = 2048 (eight)
// k_entity_stream<1,1> / <3,8,EXACT> / <3,8,false>; also what fused_supported accepts
inline int stream_width_band(int D4, int R4) {
  if (D4 <= kTinyQuads && R4 <= kTinyQuads) return DRIN_WIDTH_TINY;
  if (D4 == kExactTextQuads && R4 == kExactImageQuads) return DRIN_WIDTH_EXACT;
  if (D4 <= kExactTextQuads && R4 <= kExactImageQuads) return DRIN_WIDTH_GUARDED;
  return DRIN_WIDTH_NOT_BUILT;
}
// k_pair_layer1 / k_pair_final <1> / <3,true> / <3,false>: text rows only.  A non-default vertex activation has the GENERIC_ACT
// twins of the tiny and the guarded form; at D = 768 it runs the guarded one
inline int pair_width_band(int D4, bool generic_act) {
  if (D4 <= kTinyQuads) return DRIN_WIDTH_TINY;
  if (D4 == kExactTextQuads && !generic_act) return DRIN_WIDTH_EXACT;
  if (D4 <= kExactTextQuads) return DRIN_WIDTH_GUARDED;
  return DRIN_WIDTH_NOT_BUILT;
}
// k_entity_cache_rows<1,1> / <3,8>: one guarded instantiation serves the exact width too (`exact` then says every lane is full)
inline int cache_rows_width_band(int D4, int R4) { return stream_width_band(D4, R4); }
// k_cache_pack_mixed<1> / <3>: text-width fields only; the same remark
inline int cache_pack_width_band(int D4) { return pair_width_band(D4, false); }
// k_cached_pairs: fp32 rows <1,1> / <3,8,EXACT> / <3,8,false>; DRIN_CACHE_MIXED_F16 rows read the object row in the pair layout,
// an even number of image slots: <1,2> up to R = 512.  GENERIC_ACT twins as for the pair kernels
inline int cached_pairs_width_band(int D4, int R4, bool mixed, bool generic_act) {
  if (D4 <= kTinyQuads && R4 <= (mixed ? 2 * kTinyQuads : kTinyQuads)) return DRIN_WIDTH_TINY;
  if (D4 == kExactTextQuads && R4 == kExactImageQuads && !generic_act) return DRIN_WIDTH_EXACT;
  if (D4 <= kExactTextQuads && R4 <= kExactImageQuads) return DRIN_WIDTH_GUARDED;
  return DRIN_WIDTH_NOT_BUILT;
}

// An argument block starts zeroed; the fields that restate the configuration are derived here and nowhere else (shape: every
// block; vertex fields: PairArgs, FinalArgs, CachedArgs; edge fields: StreamArgs, CachedArgs); the rest is the call site's.
template <class Args>
Args shaped_args(const drin_config& c) {
  Args a;
  memset(&a, 0, sizeof(a));
  a.B = c.batch, a.N = c.num_candidates, a.D4 = c.embed_dim / 4;
  return a;
}
template <class Args>
void set_vertex_fields(Args& a, const drin_config& c) {
  a.ln_eps = c.layer_norm_eps, a.act_v = vertex_act(&c);
}
template <class Args>
void set_edge_fields(Args& a, const drin_config& c) {
  a.R4 = c.image_dim / 4;
  a.Km = c.mention_objects;
  a.dynamic = c.dynamic_edges != 0;
  a.act_e = edge_act(&c);
  for (int k = 0; k < 4; ++k) a.mask[k] = c.edge_enabled[k];
  a.cos_eps = c.cosine_eps, a.miei_eps = c.miei_eps, a.clip = c.clip_scale;
}

size_t entity_stream_lds_bytes(const StreamArgs& a);
int launch_entity_stream(const StreamArgs& a, hipStream_t st);
int launch_reduce_stream_partials(const float* part, float* s_text, float* s_img, float* sig, int B, int D, int R,
                                  int chunks, hipStream_t st);
int launch_mention_input1(const float* T, const float* T2, const float* sig, const float* b_et, const float* b_ei,
                          const float* v0, float* out, int B, int D, int N, hipStream_t st);
int launch_pair_layer1(const PairArgs& a, hipStream_t st);
int launch_mention_input2(const float* part, const float* mt1, float* out, int B, int D, int N, int chunks,
                          hipStream_t st);
int launch_pair_final(const FinalArgs& a, hipStream_t st);

// ---- what drin_forward_prepared and drin_forward_cached share (fused_forward.hip) ----------------------------------------------
// The two are one folded model around two ways of getting a pair's layer-1 entity quantities: run_folded_head, the path's own
// middle with run_folded_mention_finish inside, run_folded_tail.  `weight_planes` (the mention-sized products read the prepared bf16
// planes of their weights) and the scratch a path hands over select kernels inside the GEMM module, hence bits: passed on as given.
// Mention-side pooling (ghmfc.py:54-60, model.py:41; fp32 or bf16 features by cfg->feature_dtype), the two vertex-encoder Linears
// -> vm0 = [mt0; mi0], then hmfu = [hm | fu] = vm0 [W_h1; W_u1]^T + [0; b_u1].
int run_folded_head(const drin_config* cfg, const drin_batch* b, const drin_params* params, const float* prepared, const Prepared& P,
                    bool weight_planes, float* span_mean, float* mimg, float* vm0, float* hmfu, GemmScratch mention_sk, hipStream_t st,
                    const drin_mention_head* head = nullptr);   // a rows head: k_mention_rows and the mention-image product alone
// Layer-1 mention vertices from their W_h1 output (LayerNorm + activation in place), then hm2 = vm1 W_h2^T.
int run_folded_mention_finish(const drin_config* cfg, const drin_params* params, const float* prepared, const Prepared& P,
                              bool weight_planes, float* vm1, float* hm2, GemmScratch mention_sk, hipStream_t st);
// Layer 2: the mention-text vertex mt2 (through agg2), the contraction h2 = et1 W_h2^T - on et1's bf16 planes (hi at et1_hi, lo
// behind it; the LDS-DMA kernel, pair_sk its scratch) or, et1_hi == NULL, on fp32 et1 - then k_pair_final's vertex and score.
int run_folded_tail(const drin_config* cfg, const drin_params* params, const float* prepared, const Prepared& P, int chunks,
                    const float* s2_part, const float* vm1, float* agg2, float* mt2, const float* hm2, const float* e1m, float* h2,
                    const float* et1, const void* et1_hi, bool weight_planes, GemmScratch mention_sk, GemmScratch pair_sk,
                    float* scores, hipStream_t st);
}  // namespace drin
