// Fused two-layer inference pipeline: drin_prepare / drin_forward_prepared.
//
// The reference evaluates, per (mention, candidate) pair, six D x D and one D x R contractions
// (10.2 MFLOP after dead-code elimination).  For inference most of them are linear maps applied to
// linear maps, so they fold (fp32 re-association only; parity is pinned by the same golden tests):
//
//   layer-1 entity vertices (model.py:128,146):   W_h(e_a mt + e_b mi + W_et x + b_et) + b_h
//        = x (W_h W_et)^T + e_a (W_h mt) + e_b (W_h mi) + (W_h b_et + b_h)        -> C_t, hm, c_t
//   layer-1 dynamic edges (model.py:148-153):     mean_d(W_u(u) * (W_v(W_et x + b_et) + b_v))
//        = ((W_v W_et)^T W_u(u)) . x / D + W_u(u) . (W_v b_et + b_v) / D           -> q, kappa
//   layer-1 mention vertices (model.py:143-144):  mean_n(e W_et x + e b_et)
//        = W_et (sum_n e x) / N + b_et (sum_n e) / N                               -> S, sigma
//   layer-2 (last): only mt'' and et'' reach the score (model.py:207-209); its edge update, mi'', ei''
//   are dead, and  W_h2(e_a mt' + e_b mi' + et') = et' W_h2^T + e_a (W_h2 mt') + e_b (W_h2 mi').
//
// Per pair this leaves three contractions - x_t C_t^T (D x D), x_i C_i^T (D x R), et' W_h2^T (D x D):
// 5.5 MFLOP - plus ONE streaming pass over the entity bytes (k_entity_stream) and two row kernels.
// The folded matrices depend only on the weights: drin_prepare computes them once per weight version
// into a caller-owned buffer.
#include <string.h>

#include "fused.h"
#include "internal.h"
#include "layout.h"

namespace drin {

// DRIN_PREC_BF16X3_IF16: the shortest candidate list whose mean averages the one-pass image contraction's noise far enough
constexpr int kMixedMinCandidates = 64;

// The side schedule's grid.  G, f and the least tile count: profiles/image_overlap_ab.txt - G in {32, 48, 64, 96} x f in 0.1 .. 0.9 on one
// resident headline batch: the side part may outlast the stream pass (it goes on under the layer-1 mention chain and x_t C_t^T), so
// the step falls with f until the side part ends at the join: G = 64, f = 0.9 (headline 16.00 -> 14.60 ms over fresh processes).  Fewer
// workgroups cannot finish in time, 96 cost the stream pass and x_t C_t^T more than they save.  Below ~1 200 tiles (B = 1 024 at N = 101)
// the gain sinks into the noise, so smaller calls keep the one launch.  (The three macros exist for probe builds of that file's grid.)
#ifndef DRIN_SIDE_WGS
#define DRIN_SIDE_WGS 64          // G
#endif
#ifndef DRIN_SIDE_PERMILLE
#define DRIN_SIDE_PERMILLE 900    // f, in thousandths of the row tiles
#endif
#ifndef DRIN_SIDE_MIN_TILES
#define DRIN_SIDE_MIN_TILES 1200
#endif
#ifdef DRIN_SIDE_PROBE   // probe builds only (tools/probes/image_overlap_ab.py): G and f set between calls of one process
static int g_probe_wgs = DRIN_SIDE_WGS, g_probe_permille = DRIN_SIDE_PERMILLE;
extern "C" __attribute__((visibility("default"))) void drin_probe_side_plan(int wgs, int permille) { g_probe_wgs = wgs, g_probe_permille = permille; }
#endif

// How a call runs x_i C_i^T.  The rows are read in place wherever they can be: writing 8 KB/pair of planes from the stream kernel costs
// it more (measured twice on one box: +1.0 ms at B = 4096) than the LDS-DMA kernel gains on that GEMM (-0.35 ms).
enum class ImageForm {
  kGeneric,        // launch_gemm_nt at the call's precision: exact fp32 - or, at widths that keep a split-bf16 call off the planes, its own choice
  kSplitRows,      // fp32 rows read in place, split on the fly: 3 passes
  kBf16Rows,       // bf16 rows read in place, their own (only) plane: 2 passes
  kStreamPlanes,   // the table form, which has to gather the rows anyway: the stream pass writes them as planes (hi, lo; bf16 rows: hi alone)
  // DRIN_PREC_BF16X3_IF16: ONE pass of the fp16 matrix instruction on single planes.  k_entity_stream, which holds every image row in
  // registers anyway, writes it as fp16(x / 2^ceil(log2 max|x|)) with the scale beside it; the folded weight is one fp16 plane under one
  // scale (drin_prepare); the epilogue multiplies both back (bf16-STORED rows measured a wash and keep their two passes)
  kF16Plane,
};
enum class Refusal { kNone, kIndexWithoutTable, kTableOffPlanes, kBf16OffPlanes };

// The plan of one folded forward: which operands travel as bf16 planes and how x_i C_i^T runs - a pure function of the configuration
// and of `indexed` (entity_index given): no HIP call, no pointer.  FusedLayout sizes its regions from it, the call launches by it (after
// demoting it by what only the run knows), the drin_image_contraction_* queries answer its fields, fused_layout_selfcheck checks it.
struct FoldedPlan {
  bool plane_regions;   // the precision asks for planes: the regions exist (whichever way `indexed` falls, so do the sizes below)
  bool planes;          // ... and the widths allow them: the three pair-sized contractions run on the LDS-DMA kernel of gemm_x3_planes.hip
  bool xt_lo;           // x_t has a lo plane (pooled entity text stored as bf16 is exact in its hi plane: two MFMAs per tile pair)
  ImageForm form;
  int passes;           // what drin_image_contraction_passes answers
  size_t plane_floats, p_xi_floats, xi_scale_floats, splitk_floats;   // p_xt and p_et1 each, p_xi, xi_scale, splitk
  // The eager side schedule: row tiles [0, S) as G persistent workgroups on the library's side stream, under the entity stream
  // pass, the rest at full grid behind it.  {0, 0}: one launch on the caller's stream.
  int64_t S;
  int G;
  Refusal refusal;
};
static FoldedPlan folded_plan(const drin_config& c, bool indexed) {
  FoldedPlan p = {};
  const int D = c.embed_dim, R = c.image_dim;
  const int64_t M = (int64_t)c.batch * c.num_candidates;
  const size_t B = c.batch, MD = (size_t)M * D, MR = (size_t)M * R;
  const bool bf16_rows = c.feature_dtype == DRIN_FEAT_BF16, if16 = c.precision == DRIN_PREC_BF16X3_IF16;
  p.plane_regions = folded_planes(c);
  p.planes = p.plane_regions && nt_planes_width(D) && nt_planes_width(R);
  p.xt_lo = !(bf16_rows && c.entity_tokens <= 0);
  // The one fp16 pass (what is left of its gate - 16-byte alignment of workspace slots - holds by the workspace contract): per-pair
  // fp32-stored rows, the exact widths the stream kernel's fp16 hand-over is instantiated for, at least half a round of 256 x 256
  // tiles, a list long enough to average the pass's rounding (on TRAINED weights 1.2e-4 at N = 11, outside the bar, 2e-5 at N = 101:
  // profiles/r4_precision_on_trained_weights.txt).  Everything else: three passes, bit for bit.
  const bool f16 = if16 && !indexed && !bf16_rows && c.num_candidates >= kMixedMinCandidates && D == 768 && R == 2048 &&
                   cdiv(M, 256) * cdiv(D, 256) >= 128;
  p.form = !p.planes ? ImageForm::kGeneric : indexed ? ImageForm::kStreamPlanes : f16 ? ImageForm::kF16Plane : bf16_rows ? ImageForm::kBf16Rows : ImageForm::kSplitRows;
  // (kGeneric in a split-bf16 precision: launch_gemm_nt splits fp32 rows itself from 256 pairs up, and bf16 rows are refused)
  p.passes = p.form == ImageForm::kGeneric && !p.plane_regions ? 0 : p.form == ImageForm::kF16Plane ? 1 : bf16_rows ? 2 : 3;
  p.refusal = indexed && c.num_entities <= 0 ? Refusal::kIndexWithoutTable : indexed && !p.planes ? Refusal::kTableOffPlanes
              : bf16_rows && !p.planes ? Refusal::kBf16OffPlanes : Refusal::kNone;
  // The regions, sized by use as far as the configuration alone says it: tables (cfg.num_entities > 0, indexed in this call
  // or not) M R floats of image planes; DRIN_PREC_BF16X3_IF16 the fp16 plane, M R / 2, and a scale per pair; else nothing (-3.4 GB at the headline)
  p.plane_floats = p.plane_regions ? MD : 0;   // hi plane (M*D bf16) then lo plane
  p.p_xi_floats = !p.plane_regions ? 0 : c.num_entities > 0 ? MR : if16 ? MR / 2 : 0;
  p.xi_scale_floats = if16 ? (size_t)M : 0;
  // split-K partials of the mention-sized exact-fp32 products (small batches: the call is a chain of ~25 launches)
  // (the widest: q [2 B][D + R]; in split-bf16 precision at least tail_split_floor_floats(), so that a partly filled last round of
  //  tiles of the larger products can split K over the idle CUs - gemm_bf16x3.hip)
  p.splitk_floats = 2 * B <= (size_t)kSmallSplitkMaxRows ? small_splitk_floats(2 * B, (size_t)D + R) : 0;
  if (p.plane_regions && p.splitk_floats < tail_split_floor_floats()) p.splitk_floats = tail_split_floor_floats();
  // The side schedule: only where both kernels' four-phase contract holds (rows read in place on the planes' widths, at least
  // DRIN_SIDE_MIN_TILES tiles) and S row tiles lie outside the product's tail split.
  int wgs = DRIN_SIDE_WGS, permille = DRIN_SIDE_PERMILLE;
#ifdef DRIN_SIDE_PROBE
  wgs = g_probe_wgs, permille = g_probe_permille;
#endif
  const int64_t nx = cdiv(D, 256), row_tiles = cdiv(M, 256), tiles = row_tiles * nx;
  // (192: below it the fp32-row product leaves the 256 x 256 kernel - launch_gemm_nt_bf16x3; the bf16-row one from 129 up)
  const bool in_place = p.form == ImageForm::kSplitRows || p.form == ImageForm::kBf16Rows;
  if (!in_place || wgs <= 0 || permille <= 0 || tiles < 192 || tiles < DRIN_SIDE_MIN_TILES || tiles > ((int64_t)1 << 28)) return p;
  const int64_t whole_rows = gemm_p4_whole_tiles(tiles, R, p.splitk_floats > 0, p.splitk_floats) / nx;
  int64_t S = (row_tiles * permille + 500) / 1000;
  S = S < whole_rows ? S : whole_rows;
  S = S < row_tiles - 1 ? S : row_tiles - 1;   // the plain launch behind the join keeps the last row tile (and the tail split)
  if (S > 0) p.S = S, p.G = (int)(wgs < S * nx ? wgs : S * nx);
  return p;
}
static int refuse(Refusal r, const drin_config* cfg) {
  if (r == Refusal::kNone) return DRIN_OK;
  if (r == Refusal::kIndexWithoutTable)
    set_error("drin_forward_prepared: entity_index given but cfg.num_entities = %d", cfg->num_entities);
  else if (r == Refusal::kTableOffPlanes)   // the fp32 contractions read the entity rows in place; with a table they need gathered copies
    set_error("drin_forward_prepared: entity_index needs the split-bf16 precision (the stream kernel gathers the "
              "GEMM operands as planes); gather on the caller side for DRIN_PREC_F32");
  else
    set_error("drin_forward_prepared: bf16 features need the split-bf16 precision (DRIN_PREC_BF16X3) and D, R multiples of 32");
  return r == Refusal::kIndexWithoutTable ? DRIN_E_SHAPE : DRIN_E_UNSUPPORTED;
}

struct FusedLayout {  // workspace offsets in floats
  size_t span_mean, mimg, vm0, hmfu, q, e0m, e1m, xt, s_part, s_text, s_img, sig, tm, tm2, agg1, vm1, hm2, h_text, h_image,
      et1, s2_part, agg2, mt2, p_xt, p_xi, p_et1, xi_scale, splitk, splitk_floats, pair_splitk, pair_splitk_floats, total;
  int chunks;
  void build(const drin_config& c, const FoldedPlan& plan) {
    const size_t B = c.batch, N = c.num_candidates, D = c.embed_dim, R = c.image_dim, M = B * N;
    // a workgroup owns 16 consecutive candidates of one mention (4 per wave) - or, from 2 048 mentions up, where the mentions
    // alone fill the chip eight times over, up to 128 of them (WikiMEL: the whole list): one prologue of mention-side vectors
    // and one cross-wave reduction per mention instead of seven, no partial sums to write and reduce (same box, three
    // alternating runs: k_reduce_stream_partials' 0.15 ms gone, the stream kernel itself unchanged, step -0.19 ms;
    // profiles/r3_stream_chunk_ab.txt).  The grouping of the per-mention sums therefore depends on the size of the call: a
    // mention's scores in a small and in a large call differ by fp32 re-association (as through the tile choices of the
    // mention-sized products), within one call size they are the same bits every run.
    chunks = (int)(B >= 2048 ? (N + 127) / 128 : B >= 1024 ? (N + 47) / 48 : (N + 15) / 16);   // (1 024 mentions: 48 candidates, 4.56 -> 4.49 ms)
    Arena A;
    span_mean = A.take(B * D);
    mimg = A.take(B * R);
    vm0 = A.take(2 * B * D);
    hmfu = A.take(2 * B * 2 * D);
    q = A.take(2 * B * (D + R));
    e0m = A.take(4 * M);
    e1m = A.take(4 * M);
    xt = A.take(c.entity_tokens > 0 ? M * D : 0);
    s_part = A.take(B * chunks * (2 * D + 2 * R + 4));
    s_text = A.take(2 * B * D);
    s_img = A.take(2 * B * R);
    sig = A.take(4 * B);
    tm = A.take(2 * B * D);
    tm2 = A.take(2 * B * D);
    agg1 = A.take(2 * B * D);
    vm1 = A.take(2 * B * D);
    hm2 = A.take(2 * B * D);
    h_text = A.take(M * D);   // re-used for et1 W_h2^T once layer 1 is done
    h_image = A.take(M * D);
    et1 = A.take(M * D);
    s2_part = A.take(B * chunks * 2 * D);
    agg2 = A.take(B * D);
    mt2 = A.take(B * D);
    p_xt = A.take(plan.plane_floats);
    p_xi = A.take(plan.p_xi_floats);
    p_et1 = A.take(plan.plane_floats);
    xi_scale = A.take(plan.xi_scale_floats);
    splitk = A.take(splitk_floats = plan.splitk_floats);
    // split-K partials of the pair-sized split-bf16 products when the whole batch is less than half a round of 256 x 256 tiles
    pair_splitk_floats = plan.plane_regions ? drin::pair_splitk_floats(M, D) : 0;
    pair_splitk = A.take(pair_splitk_floats);
    total = A.total;
  }
};

// The regions with the floats the kernels index - of p_xi and xi_scale per form, not read off the plan's sizes - and, over both ways
// `indexed` can fall, the plan against itself: form <-> passes, and a side schedule only on rows read in place, inside the row tiles.
int fused_layout_selfcheck(const drin_config& c) {
  const size_t B = c.batch, M = B * c.num_candidates, D = c.embed_dim, R = c.image_dim;
  const int64_t nx = cdiv((int64_t)D, 256), row_tiles = cdiv((int64_t)M, 256);
  const bool bf16_rows = c.feature_dtype == DRIN_FEAT_BF16;
  size_t xi = 0, scale = 0, planes = 0;
  for (int indexed = 0; indexed < 2; ++indexed) {
    const FoldedPlan p = folded_plan(c, indexed != 0);
    if (p.refusal != Refusal::kNone) continue;
    const bool in_place = p.form == ImageForm::kSplitRows || p.form == ImageForm::kBf16Rows;
    static_assert((int)ImageForm::kF16Plane == 4, "by form, in ImageForm's order");   // p_xi: M R bf16 per plane the stream pass writes, M R halves (with M scales)
    const int passes[] = {c.precision == DRIN_PREC_F32 ? 0 : 3, 3, 2, bf16_rows ? 2 : 3, 1};
    const size_t need[] = {0, 0, 0, bf16_rows ? M * R / 2 : M * R, M * R / 2};
    if (p.form == ImageForm::kF16Plane) scale = M;
    if (p.passes != passes[(int)p.form] || p.S < 0 || (p.S > 0 ? !(in_place && p.S < row_tiles && p.G >= 1 && p.G <= p.S * nx) : p.G != 0)) {
      set_error("selftest: FoldedPlan(indexed = %d): form %d with %d passes, side schedule {%lld, %d} of %lld row tiles", indexed, (int)p.form,
                p.passes, (long long)p.S, p.G, (long long)row_tiles);
      return DRIN_E_WORKSPACE;
    }
    xi = need[(int)p.form] > xi ? need[(int)p.form] : xi, planes |= p.planes;
  }
  FusedLayout L;
  L.build(c, folded_plan(c, false));
  const size_t ch = (size_t)L.chunks;
  const Region ws[] = {
      {"span_mean", L.span_mean, B * D}, {"mimg", L.mimg, B * R}, {"vm0", L.vm0, 2 * B * D}, {"hmfu", L.hmfu, 4 * B * D},
      {"q", L.q, 2 * B * (D + R)}, {"e0m", L.e0m, 4 * M}, {"e1m", L.e1m, 4 * M}, {"xt", L.xt, c.entity_tokens > 0 ? M * D : 0},
      {"s_part", L.s_part, B * ch * (2 * D + 2 * R + 4)}, {"s_text", L.s_text, 2 * B * D}, {"s_img", L.s_img, 2 * B * R},
      {"sig", L.sig, 4 * B}, {"tm", L.tm, 2 * B * D}, {"tm2", L.tm2, 2 * B * D}, {"agg1", L.agg1, 2 * B * D}, {"vm1", L.vm1, 2 * B * D},
      {"hm2", L.hm2, 2 * B * D}, {"h_text", L.h_text, M * D}, {"h_image", L.h_image, M * D}, {"et1", L.et1, M * D},
      {"s2_part", L.s2_part, B * ch * 2 * D}, {"agg2", L.agg2, B * D}, {"mt2", L.mt2, B * D}, {"p_xt", L.p_xt, planes * M * D},
      {"p_xi", L.p_xi, xi}, {"p_et1", L.p_et1, planes * M * D}, {"xi_scale", L.xi_scale, scale},
      {"splitk", L.splitk, L.splitk_floats}, {"pair_splitk", L.pair_splitk, L.pair_splitk_floats}};
  DRIN_TRY(regions_hold("FusedLayout", ws, (int)(sizeof(ws) / sizeof(ws[0])), L.total));
  Prepared P;
  P.build(c);
  const Region pr[] = {
      {"wcat1", P.wcat1, 2 * D * D}, {"bcat1", P.bcat1, 2 * D}, {"ecat", P.ecat, D * (D + R)}, {"etmp", P.etmp, D * (D + R)},
      {"k_t", P.k_t, D}, {"k_i", P.k_i, D}, {"c_txt", P.c_txt, D * D}, {"c_img", P.c_img, D * R}, {"cb_t", P.cb_t, D}, {"cb_i", P.cb_i, D},
      {"p_ctxt", P.p_ctxt, D * D}, {"p_cimg", P.p_cimg, D * R}, {"p_wh2", P.p_wh2, D * D}, {"p_wmt", P.p_wmt, D * D},
      {"p_wmi", P.p_wmi, D * R}, {"p_wcat1", P.p_wcat1, 2 * D * D}, {"p_ecat", P.p_ecat, D * (D + R)}, {"p_wet", P.p_wet, D * D},
      {"p_wei", P.p_wei, D * R}, {"p_wh1", P.p_wh1, D * D}, {"p_cimg_f16", P.p_cimg_f16, D * R / 2}, {"cimg_f16_scale", P.cimg_f16_scale, 2}};
  return regions_hold("Prepared", pr, (int)(sizeof(pr) / sizeof(pr[0])), P.total);
}

// The caller's stream joins the side stream when the call leaves, whatever way it leaves
struct SideJoin {
  SideLane* lane = nullptr;
  hipStream_t st = nullptr;
  int join() {
    if (!lane) return DRIN_OK;
    const hipError_t e = hipStreamWaitEvent(st, lane->join, 0);
    lane = nullptr;
    return e == hipSuccess ? DRIN_OK : hip_fail(e, "hipStreamWaitEvent(side stream)");
  }
  ~SideJoin() { (void)join(); }
};

int fused_supported(const drin_config* c) {
  if (c->num_layers != 2) {
    set_error("fused path: built for num_layers == 2 (got %d); use drin_forward", c->num_layers);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->vector_edges) {
    set_error("fused path: vector edge features (model.py:112-116) run on the layer-by-layer path; use drin_forward");
    return DRIN_E_UNSUPPORTED;
  }
  if (c->mention_object_inner > 1 || c->entity_object_inner > 1 || c->entity_image_inner > 1) {
    set_error("fused path: inner feature dims > 1 need the pooled path of drin_forward");
    return DRIN_E_UNSUPPORTED;
  }
  if (stream_width_band(c->embed_dim / 4, c->image_dim / 4) == DRIN_WIDTH_NOT_BUILT) {   // every family is built where this one is
    set_error("fused path: D=%d R=%d outside the built instantiations", c->embed_dim, c->image_dim);
    return DRIN_E_UNSUPPORTED;
  }
  return DRIN_OK;
}

}  // namespace drin

using namespace drin;

extern "C" {

int drin_split_planes(const float* x, void* hi, void* lo, int64_t n, void* stream) {
  DRIN_BIND_DEVICE(stream, x, "drin_split_planes");
  if (!x || !hi || !lo) {
    set_error("drin_split_planes: NULL argument");
    return DRIN_E_NULL;
  }
  return launch_split_planes(x, hi, lo, n, (hipStream_t)stream);
}

int drin_linear_planes_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias,
                           float* y, int64_t rows, int32_t n_out, int32_t k, void* stream) {
  DRIN_BIND_DEVICE(stream, y, "drin_linear_planes_fwd");
  if (!x_hi || !w_hi || !w_lo || !y) {
    set_error("drin_linear_planes_fwd: NULL argument");
    return DRIN_E_NULL;
  }
  return launch_gemm_x3_planes(x_hi, x_lo, k, w_hi, w_lo, k, bias, y, n_out, rows, n_out, k, (hipStream_t)stream);
}

int drin_fused_supported(const drin_config* cfg) {
  DRIN_TRY(validate_config(cfg));
  return fused_supported(cfg);
}

int drin_width_class(const drin_config* cfg, int family) {
  DRIN_TRY(validate_config(cfg));
  if (family < DRIN_WIDTH_FAMILY_ENTITY_STREAM || family > DRIN_WIDTH_FAMILY_LN_BACKWARD) {
    set_error("drin_width_class: family %d is not a drin_width_family", family);
    return DRIN_E_SHAPE;
  }
  if (family == DRIN_WIDTH_FAMILY_LN_BACKWARD) return ln_bwd_slots(cfg->embed_dim);   // the layer-by-layer path: any validated width
  if (fused_supported(cfg) != DRIN_OK) return DRIN_WIDTH_NOT_BUILT;
  const int D4 = cfg->embed_dim / 4, R4 = cfg->image_dim / 4;
  const bool gen = vertex_act(cfg) != DRIN_ACT_GELU, mixed = cfg->cache_format == DRIN_CACHE_MIXED_F16;
  const bool mixed_rows_fit = cfg->embed_dim % 8 == 0 && cfg->image_dim % 8 == 0;   // (cache_supported, entity_cache.hip)
  switch (family) {
    case DRIN_WIDTH_FAMILY_ENTITY_STREAM:
      return stream_width_band(D4, R4);
    case DRIN_WIDTH_FAMILY_PAIR_ROWS:
      return pair_width_band(D4, gen);
    case DRIN_WIDTH_FAMILY_CACHE_ROWS:
      return mixed && !mixed_rows_fit ? DRIN_WIDTH_NOT_BUILT : cache_rows_width_band(D4, R4);
    case DRIN_WIDTH_FAMILY_CACHE_PACK:   // runs for DRIN_CACHE_MIXED_F16 rows only
      return mixed && mixed_rows_fit ? cache_pack_width_band(D4) : DRIN_WIDTH_NOT_BUILT;
    default:
      return mixed && !mixed_rows_fit ? DRIN_WIDTH_NOT_BUILT : cached_pairs_width_band(D4, R4, mixed, gen);
  }
}

size_t drin_prepared_bytes(const drin_config* cfg) {
  if (validate_config(cfg) != DRIN_OK || fused_supported(cfg) != DRIN_OK) return 0;
  Prepared P;
  P.build(*cfg);
  return P.total * sizeof(float);
}

int drin_prepare(const drin_config* cfg, const drin_params* params, void* prepared, size_t prepared_bytes,
                 void* stream) {
  DRIN_BIND_DEVICE(stream, prepared, "drin_prepare");
  RoctxRange range("drin_prepare");
  DRIN_TRY(validate_config(cfg));
  DRIN_TRY(fused_supported(cfg));
  if (!params || !prepared) {
    set_error("drin_prepare: NULL argument");
    return DRIN_E_NULL;
  }
  {   // every weight the folds read; w_mention_text alone may be NULL (a DRIN_MENTION_ROWS model: its plane is skipped below)
    const void* need[] = {params->w_entity_text, params->b_entity_text, params->w_mention_image, params->w_entity_image,
                          params->b_entity_image, params->layer[0].w_h, params->layer[0].b_h, params->layer[0].w_u, params->layer[0].b_u,
                          params->layer[0].w_v, params->layer[0].b_v, params->layer[1].w_h};
    for (const void* q : need)
      if (!q) {
        set_error("drin_prepare: a weight the folds read is NULL (only w_mention_text may be, for a DRIN_MENTION_ROWS model)");
        return DRIN_E_NULL;
      }
  }
  Prepared P;
  P.build(*cfg);
  if (prepared_bytes < P.total * sizeof(float) || !aligned16(prepared)) {
    set_error("drin_prepare: buffer has %zu bytes (needs %zu) or is not 16-byte aligned", prepared_bytes,
              P.total * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* pb = (float*)prepared;
  const int D = cfg->embed_dim, R = cfg->image_dim;
  const drin_layer_params& L1 = params->layer[0];
  const int F32 = DRIN_PREC_F32;  // the folds are computed once, in exact fp32
  auto copy = [&](float* dst, const float* src, size_t n) -> int {
    hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? DRIN_OK : hip_fail(e, "hipMemcpyAsync(prepare)");
  };
  DRIN_TRY(copy(pb + P.wcat1, L1.w_h, (size_t)D * D));
  DRIN_TRY(copy(pb + P.wcat1 + (size_t)D * D, L1.w_u, (size_t)D * D));
  {
    hipError_t e = hipMemsetAsync(pb + P.bcat1, 0, D * sizeof(float), st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(prepare)");
  }
  DRIN_TRY(copy(pb + P.bcat1 + D, L1.b_u, D));
  // E = W_v1 [W_et | W_ei]   (y[m, n] = sum_k x[m, k] w[k, n])
  DRIN_TRY(launch_gemm_nn({{L1.w_v, D}, {params->w_entity_text, D}, pb + P.etmp, D + R, D, D, D}, F32, st));
  DRIN_TRY(launch_gemm_nn({{L1.w_v, D}, {params->w_entity_image, R}, pb + P.etmp + D, D + R, D, R, D}, F32, st));
  DRIN_TRY(launch_transpose(pb + P.etmp, pb + P.ecat, D, D + R, st));
  // k = b_e W_v1^T + b_v1 as row vectors
  DRIN_TRY(launch_gemm_nt({{params->b_entity_text, D}, {L1.w_v, D}, L1.b_v, pb + P.k_t, D, 1, D, D}, F32, st));
  DRIN_TRY(launch_gemm_nt({{params->b_entity_image, D}, {L1.w_v, D}, L1.b_v, pb + P.k_i, D, 1, D, D}, F32, st));
  // C = W_h1 [W_et | W_ei],  cb = b_e W_h1^T + b_h1
  DRIN_TRY(launch_gemm_nn({{L1.w_h, D}, {params->w_entity_text, D}, pb + P.c_txt, D, D, D, D}, F32, st));
  DRIN_TRY(launch_gemm_nn({{L1.w_h, D}, {params->w_entity_image, R}, pb + P.c_img, R, D, R, D}, F32, st));
  DRIN_TRY(launch_gemm_nt({{params->b_entity_text, D}, {L1.w_h, D}, L1.b_h, pb + P.cb_t, D, 1, D, D}, F32, st));
  DRIN_TRY(launch_gemm_nt({{params->b_entity_image, D}, {L1.w_h, D}, L1.b_h, pb + P.cb_i, D, 1, D, D}, F32, st));
  // bf16 hi / lo planes of the pair-sized GEMM weights (split-bf16 precision)
  {
    const size_t dd = (size_t)D * D, dr = (size_t)D * R;
    __bf16* q = reinterpret_cast<__bf16*>(pb + P.p_ctxt);
    DRIN_TRY(launch_split_planes(pb + P.c_txt, q, q + dd, dd, st));
    q = reinterpret_cast<__bf16*>(pb + P.p_cimg);
    DRIN_TRY(launch_split_planes(pb + P.c_img, q, q + dr, dr, st));
    // DRIN_PREC_BF16X3_IF16: one fp16 plane under one power-of-two scale (weights of any magnitude stay inside fp16's range)
    DRIN_TRY(launch_to_f16_scaled(pb + P.c_img, pb + P.p_cimg_f16, (int64_t)dr, pb + P.cimg_f16_scale, st));
    q = reinterpret_cast<__bf16*>(pb + P.p_wh2);
    DRIN_TRY(launch_split_planes(params->layer[1].w_h, q, q + dd, dd, st));
    // mention-sized GEMM weights (they matter for short candidate lists: at N = 11 the mention side is a third
    // of the contraction work)
    struct { size_t off; const float* w; size_t n; } extra[] = {
        {P.p_wmt, params->w_mention_text, dd},  {P.p_wmi, params->w_mention_image, dr},
        {P.p_wcat1, pb + P.wcat1, 2 * dd},      {P.p_ecat, pb + P.ecat, dd + dr},
        {P.p_wet, params->w_entity_text, dd},   {P.p_wei, params->w_entity_image, dr},
        {P.p_wh1, L1.w_h, dd}};
    for (const auto& e : extra) {
      // w_mention_text NULL: a model whose mention head is DRIN_MENTION_ROWS has no such Linear; its plane is zeroed, so a later call
      // without a rows head on this buffer reads zeros, never uninitialised memory (drin_hip.h: drin_forward_prepared_head)
      if (e.off == P.p_wmt && e.w == nullptr) {
        const hipError_t me = hipMemsetAsync(pb + e.off, 0, e.n * sizeof(float), st);
        if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync(prepare)");
        continue;
      }
      q = reinterpret_cast<__bf16*>(pb + e.off);
      DRIN_TRY(launch_split_planes(e.w, q, q + e.n, e.n, st));
    }
  }
  return DRIN_OK;
}

}  // extern "C"

namespace drin {

int run_folded_head(const drin_config* cfg, const drin_batch* b, const drin_params* params, const float* pb, const Prepared& P,
                    bool weight_planes, float* span_mean, float* mimg, float* vm0, float* hmfu, GemmScratch sk, hipStream_t st,
                    const drin_mention_head* head) {
  const int B = cfg->batch, D = cfg->embed_dim, R = cfg->image_dim, prec = folded_precision(cfg);
  auto wp = [&](size_t plane_off) -> const float* { return weight_planes ? pb + plane_off : nullptr; };
  const bool bf16 = cfg->feature_dtype == DRIN_FEAT_BF16;
  const bool rows = rows_head(head);
  if (rows) {
    // the edge row where the span mean lives (the stream pass reads it there), the vertex row straight into vm0; no Linear
    int32_t *ie, *iv;
    head_positions(cfg, head, &ie, &iv);
    DRIN_TRY(launch_mention_rows(b->mention_text, bf16, head->encoded, b->mention_start, b->mention_end, head->representation, span_mean,
                                 vm0, ie, iv, B, cfg->mention_tokens, D, st));
  } else if (bf16) {
    DRIN_TRY(launch_span_mean_bf16(b->mention_text, b->mention_start, b->mention_end, span_mean, B, cfg->mention_tokens, D, st));
  } else {
    DRIN_TRY(launch_span_mean(b->mention_text, b->mention_start, b->mention_end, span_mean, B, cfg->mention_tokens, D, st));
  }
  if (bf16)
    DRIN_TRY(launch_axis_mean_bf16(b->mention_image, mimg, B, cfg->image_regions, R, st));
  else
    DRIN_TRY(launch_axis_mean(b->mention_image, mimg, B, cfg->image_regions, R, st));
  const NtProduct enc_mi =
      NtProduct{{mimg, R}, {params->w_mention_image, R}, params->b_mention_image, vm0 + (size_t)B * D, D, B, D, R}.with_planes(wp(P.p_wmi));
  if (rows)   // the mention-text vertex is in vm0 already: the mention-image product alone
    DRIN_TRY(launch_gemm_nt(enc_mi, prec, st, sk));
  else
    DRIN_TRY(launch_gemm_nt_pair(NtProduct{{span_mean, D}, {params->w_mention_text, D}, params->b_mention_text, vm0, D, B, D, D}.with_planes(wp(P.p_wmt)),
                                 enc_mi, prec, st, sk));
  return launch_gemm_nt(NtProduct{{vm0, D}, {pb + P.wcat1, D}, pb + P.bcat1, hmfu, 2 * D, 2 * (int64_t)B, 2 * D, D}.with_planes(wp(P.p_wcat1)), prec, st, sk);
}

int run_folded_mention_finish(const drin_config* cfg, const drin_params* params, const float* pb, const Prepared& P,
                              bool weight_planes, float* vm1, float* hm2, GemmScratch sk, hipStream_t st) {
  const int B = cfg->batch, D = cfg->embed_dim;
  const drin_layer_params& L1 = params->layer[0];
  DRIN_TRY(launch_layernorm_gelu(vm1, L1.ln_weight, L1.ln_bias, vm1, nullptr, nullptr, 2 * (int64_t)B, D, cfg->layer_norm_eps, st,
                                 vertex_act(cfg)));
  const NtProduct wh2 = {{vm1, D}, {params->layer[1].w_h, D}, nullptr, hm2, D, 2 * (int64_t)B, D, D};
  return launch_gemm_nt(wh2.with_planes(weight_planes ? pb + P.p_wh2 : nullptr), folded_precision(cfg), st, sk);
}

int run_folded_tail(const drin_config* cfg, const drin_params* params, const float* pb, const Prepared& P, int chunks,
                    const float* s2_part, const float* vm1, float* agg2, float* mt2, const float* hm2, const float* e1m, float* h2,
                    const float* et1, const void* et1_hi, bool weight_planes, GemmScratch sk, GemmScratch pair_sk, float* scores,
                    hipStream_t st) {
  const int B = cfg->batch, N = cfg->num_candidates, D = cfg->embed_dim, prec = folded_precision(cfg);
  const int64_t M = (int64_t)B * N;
  const drin_layer_params& L2 = params->layer[1];
  // layer-2 mention-text vertex
  DRIN_TRY(launch_mention_input2(s2_part, vm1, agg2, B, D, N, chunks, st));
  DRIN_TRY(launch_gemm_nt(NtProduct{{agg2, D}, {L2.w_h, D}, L2.b_h, mt2, D, B, D, D}.with_planes(weight_planes ? pb + P.p_wh2 : nullptr), prec, st, sk));
  DRIN_TRY(launch_layernorm_gelu(mt2, L2.ln_weight, L2.ln_bias, mt2, nullptr, nullptr, B, D, cfg->layer_norm_eps, st, vertex_act(cfg)));
  // layer-2 entity-text contraction, vertex and score
  // (Round 6, built and dropped - profiles/r6_full_row_ab.txt, tools/probes/r6_full_row/, commit 8a5bc6b: this contraction and k_pair_final's
  //  arithmetic in ONE launch on 96-row x 768-column tiles, so that h2 never goes to HBM.  Correct, and slower: a full-row tile needs all
  //  768 weight rows per K-step for 96 activation rows - 1.56 x the LDS-DMA instructions per MFMA of the 256 x 256 tile - and its K-loop
  //  alone took what the 256 x 256 kernel takes including its store (1.20 against 1.15 ms); the epilogue's vector work came on top.)
  if (et1_hi) {
    const __bf16* e1 = static_cast<const __bf16*>(et1_hi);
    const __bf16* w2 = reinterpret_cast<const __bf16*>(pb + P.p_wh2);
    DRIN_TRY(launch_gemm_x3_planes(e1, e1 + (size_t)M * D, D, w2, w2 + (size_t)D * D, D, nullptr, h2, D, M, D, D, st, pair_sk));
  } else {
    DRIN_TRY(launch_gemm_nt({{et1, D}, {L2.w_h, D}, nullptr, h2, D, M, D, D}, prec, st));
  }
  FinalArgs fa = shaped_args<FinalArgs>(*cfg);
  set_vertex_fields(fa, *cfg);
  fa.h2 = h2;
  fa.hm2 = hm2;
  fa.b_h2 = L2.b_h;
  fa.gamma = L2.ln_weight;
  fa.beta = L2.ln_bias;
  fa.e1m = e1m;
  fa.mt2 = mt2;
  fa.scores = scores;
  fa.chunks = chunks;
  fa.cos_eps = cfg->cosine_eps;
  return launch_pair_final(fa, st);
}

// The whole forward on the caller's stream: the one pass over the entity bytes (HBM-bound), then the contractions and row kernels
// behind it (MFMA-bound).  (Running the two halves of consecutive mention chunks side by side - two streams, forced co-residency,
// disjoint CU masks - was built in round 3 and measured slower every time; removed in round 5: profiles/r3_pipeline_probe.txt.)
// One product leaves the caller's stream where the plan has a side schedule: the first S row tiles of x_i C_i^T, which depend on nothing
// the call computes, run on the library's side stream from the START of the call (fork event first: the previous call's readers of
// h_image are in front of it; the workgroups are resident before the stream pass is dispatched) and the caller's stream waits for them
// before it launches the other row tiles.  Same kernel code and the same tail split per tile as the one launch: the same bits.
static int forward_prepared_on_stream(const drin_config* cfg, const drin_batch* b, const drin_params* params, const void* prepared,
                                      void* workspace, float* scores, hipStream_t st, const drin_mention_head* head, FoldedPlan plan,
                                      const FusedLayout& L) {
  Prepared P;
  P.build(*cfg);
  float* ws = (float*)workspace;
  const float* pb = (const float*)prepared;
  const int B = cfg->batch, N = cfg->num_candidates, D = cfg->embed_dim, R = cfg->image_dim;
  const int64_t M = (int64_t)B * N;
  if (B == 0) return DRIN_OK;
  if (b->entity_text_cls) {
    set_error("drin_forward_prepared: entity_text_cls (text pooled ahead of time) is a form of the training entry points");
    return DRIN_E_UNSUPPORTED;
  }
  DRIN_TRY(refuse(plan.refusal, cfg));
  // What only the run knows, and all of it: each fact demotes the plan, nothing below asks again.  The fp16 kernel's own fit failing:
  // three passes.  A stream under capture (no parallel branches in a graph) or one that cannot say, misaligned image rows or h_image,
  // no rows at all (the plain launch reports those): the one launch.
  if (plan.form == ImageForm::kF16Plane && !gemm_f16_planes_fits(ws + L.p_xi, R, pb + P.p_cimg_f16, R, ws + L.h_image, D, M, D, R))
    plan.form = ImageForm::kSplitRows;
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (plan.S > 0 && hipStreamIsCapturing(st, &capture) != hipSuccess) {
    (void)hipGetLastError();
    capture = hipStreamCaptureStatusActive;
  }
  if (capture != hipStreamCaptureStatusNone || !aligned16(b->entity_image) || !aligned16(ws + L.h_image) || !b->entity_image) plan.S = plan.G = 0;
  const int prec = folded_precision(cfg);
  const bool dyn = cfg->dynamic_edges != 0, tokens = cfg->entity_tokens > 0, planes = plan.planes, bf16_feat = cfg->feature_dtype == DRIN_FEAT_BF16;
  __bf16* xt_hi = reinterpret_cast<__bf16*>(ws + L.p_xt);
  __bf16* xi_hi = reinterpret_cast<__bf16*>(ws + L.p_xi);
  __bf16* e1_hi = reinterpret_cast<__bf16*>(ws + L.p_et1);
  const size_t MD = (size_t)M * D, MR = (size_t)M * R;
  const drin_layer_params& L1 = params->layer[0];

  // Mention-sized contractions: launch_gemm_nt / launch_gemm_nt_pair choose the kernel; the split-bf16 ones read the prepared
  // weight planes when this path has them (`planes` also asks R % 32, which those cannot see)
  auto wp = [&](size_t plane_off) -> const float* { return planes ? pb + plane_off : nullptr; };
  const GemmScratch msk = scratch_at(ws, L.splitk, L.splitk_floats);
  float* vm0 = ws + L.vm0;
  float* hmfu = ws + L.hmfu;
  // split-K scratch of the pair-sized products: the whole-product split when the batch is a few tiles, else the tail-split scratch
  const GemmScratch psk = L.pair_splitk_floats ? GemmScratch{ws + L.pair_splitk, L.pair_splitk_floats} : msk;
  // x_i C_i^T on rows read in place (fp32: split on the fly; bf16: the rows are the one plane), whole or a slice of its row tiles
  const NtProduct xi_ci = NtProduct{{(const float*)b->entity_image, R}, {pb + P.c_img, R}, nullptr, ws + L.h_image, D, M, D, R}.with_planes(pb + P.p_cimg);
  auto image_rows_product = [&](hipStream_t on, RowTiles rows) -> int {
    if (bf16_feat)
      return launch_gemm_x3_planes(b->entity_image, nullptr, R, xi_ci.w_hi, xi_ci.w_lo, R, nullptr, ws + L.h_image, D, M, D, R, on, psk, rows);
    if (plan.S == 0) return launch_gemm_nt_bf16x3(xi_ci, on, psk);   // whole: the launcher chooses the kernel (a small product leaves the 256 x 256 one)
    return launch_gemm_nt_bf16x3_p4(xi_ci, on, aligned16(psk.p) ? psk : GemmScratch{}, rows);
  };
  SideJoin side_join;
  if (plan.S > 0) {
    SideLane* lane = nullptr;
    DRIN_TRY(side_lane(&lane));
    std::lock_guard<std::mutex> order(lane->order);
    hipError_t e = hipEventRecord(lane->fork, st);
    if (e == hipSuccess) e = hipStreamWaitEvent(lane->stream, lane->fork, 0);
    if (e != hipSuccess) return hip_fail(e, "fork to the side stream");
    const int rc = image_rows_product(lane->stream, RowTiles{0, plan.S, plan.G});
    e = hipEventRecord(lane->join, lane->stream);
    side_join.lane = lane, side_join.st = st;
    if (rc != DRIN_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord(side stream)");
  }
  // (1) mention-side pooling and vertex-encoder Linears, [hm | fu]; (2) q = fu [W_v1 W_et | W_v1 W_ei]
  DRIN_TRY(run_folded_head(cfg, b, params, pb, P, planes, ws + L.span_mean, ws + L.mimg, vm0, hmfu, msk, st, head));
  if (dyn)
    DRIN_TRY(launch_gemm_nt(NtProduct{{hmfu + D, 2 * D}, {pb + P.ecat, D}, nullptr, ws + L.q, D + R, 2 * (int64_t)B, D + R, D}.with_planes(wp(P.p_ecat)),
                            prec, st, msk));
  // (3) one pass over the entity-side bytes
  StreamArgs sa = shaped_args<StreamArgs>(*cfg);
  set_edge_fields(sa, *cfg);
  sa.entity_text = b->entity_text;
  sa.entity_mask = b->entity_text_mask;
  sa.entity_image = b->entity_image;
  sa.entity_object = b->entity_object;
  sa.entity_object_score = b->entity_object_score;
  sa.entity_index = b->entity_index;
  sa.num_entities = cfg->num_entities;
  sa.index_status = b->index_status;
  sa.miet = b->miet_similarity;
  sa.mtei = b->mtei_similarity;
  sa.span_mean = ws + L.span_mean;
  sa.mobj = b->mention_object;
  sa.mscore = b->mention_object_score;
  sa.fu = hmfu + D;
  sa.ldfu = 2 * D;
  sa.q = ws + L.q;
  sa.ldq = D + R;  // q row = [q_text (D) | q_image (R)]
  sa.k_t = pb + P.k_t;
  sa.k_i = pb + P.k_i;
  if (planes) sa.xt_hi = xt_hi, sa.xt_lo = plan.xt_lo ? xt_hi + MD : nullptr;
  else sa.xt_out = ws + L.xt;
  switch (plan.form) {   // the image outputs: only the forms whose A operand comes from this pass have any
    case ImageForm::kStreamPlanes: sa.xi_hi = xi_hi, sa.xi_lo = bf16_feat ? nullptr : xi_hi + MR; break;   // (bf16 rows are their own hi plane)
    case ImageForm::kF16Plane: sa.xi_scale = ws + L.xi_scale, sa.xi_f16 = xi_hi; break;
    default: break;
  }
  sa.e0m = ws + L.e0m;
  sa.e1m = ws + L.e1m;
  sa.s_part = ws + L.s_part;
  sa.T = cfg->entity_tokens;
  sa.Ke = cfg->entity_objects;
  sa.chunks = L.chunks;
  sa.bf16_features = bf16_feat ? 1 : 0;
  sa.s_text = ws + L.s_text;
  sa.s_img = ws + L.s_img;
  sa.sig = ws + L.sig;
  DRIN_TRY(launch_entity_stream(sa, st));
  if (L.chunks > 1)
    DRIN_TRY(launch_reduce_stream_partials(ws + L.s_part, ws + L.s_text, ws + L.s_img, ws + L.sig, B, D, R, L.chunks, st));
  // (4) layer-1 mention vertices: T = S_text W_et^T + S_img W_ei^T, then the W_h input, W_h, LN, GELU
  DRIN_TRY(launch_gemm_nt_pair(NtProduct{{ws + L.s_text, D}, {params->w_entity_text, D}, nullptr, ws + L.tm, D, 2 * (int64_t)B, D, D}.with_planes(wp(P.p_wet)),
                               NtProduct{{ws + L.s_img, R}, {params->w_entity_image, R}, nullptr, ws + L.tm2, D, 2 * (int64_t)B, D, R}.with_planes(wp(P.p_wei)),
                               prec, st, msk));
  DRIN_TRY(launch_mention_input1(ws + L.tm, ws + L.tm2, ws + L.sig, params->b_entity_text, params->b_entity_image, vm0, ws + L.agg1, B, D, N, st));
  float* vm1 = ws + L.vm1;
  DRIN_TRY(launch_gemm_nt(NtProduct{{ws + L.agg1, D}, {L1.w_h, D}, L1.b_h, vm1, D, 2 * (int64_t)B, D, D}.with_planes(wp(P.p_wh1)), prec, st, msk));
  DRIN_TRY(run_folded_mention_finish(cfg, params, pb, P, planes, vm1, ws + L.hm2, msk, st));
  // (5) the two pair-sized layer-1 contractions on the folded weights
  const __bf16* ct = reinterpret_cast<const __bf16*>(pb + P.p_ctxt);
  if (planes)
    DRIN_TRY(launch_gemm_x3_planes(xt_hi, sa.xt_lo, D, ct, ct + (size_t)D * D, D, nullptr, ws + L.h_text, D, M, D, D, st, psk));
  else
    DRIN_TRY(launch_gemm_nt({{tokens ? ws + L.xt : (const float*)b->entity_text, D}, {pb + P.c_txt, D}, nullptr, ws + L.h_text, D, M, D, D}, prec, st));
  switch (plan.form) {
    case ImageForm::kGeneric:
      DRIN_TRY(launch_gemm_nt({{(const float*)b->entity_image, R}, {pb + P.c_img, R}, nullptr, ws + L.h_image, D, M, D, R}, prec, st));
      break;
    case ImageForm::kF16Plane:   // on the plane the stream kernel wrote
      DRIN_TRY(launch_gemm_f16_planes(xi_hi, R, pb + P.p_cimg_f16, R, ws + L.xi_scale, pb + P.cimg_f16_scale, ws + L.h_image, D, M, D, R,
                                      st, psk));
      break;
    case ImageForm::kStreamPlanes:
      DRIN_TRY(launch_gemm_x3_planes(xi_hi, sa.xi_lo, R, xi_ci.w_hi, xi_ci.w_lo, R, nullptr, ws + L.h_image, D, M, D, R, st, psk));
      break;
    case ImageForm::kBf16Rows:
    case ImageForm::kSplitRows:   // whole, or the row tiles the side stream did not take, once it is done with its own
      DRIN_TRY(side_join.join());
      DRIN_TRY(image_rows_product(st, RowTiles{plan.S, -1, 0}));
      break;
  }
  // The two pair kernels walk the same candidate chunks as the stream kernel (FusedLayout::chunks: whole mentions from 2 048
  // mentions up - their share of that change: row kernels 1.385 -> 1.27 ms at 4 096 mentions; 64 mentions with whole-mention
  // workgroups 0.55 -> 0.63 ms, which is why small calls keep 16 candidates).
  // (6) layer-1 entity vertices + layer-2 mention aggregates
  PairArgs pa = shaped_args<PairArgs>(*cfg);
  set_vertex_fields(pa, *cfg);
  pa.h_text = ws + L.h_text;
  pa.h_image = ws + L.h_image;
  pa.hm = hmfu;
  pa.ldhm = 2 * D;
  pa.c_t = pb + P.cb_t;
  pa.c_i = pb + P.cb_i;
  pa.gamma = L1.ln_weight;
  pa.beta = L1.ln_bias;
  pa.e0m = ws + L.e0m;
  pa.e1m = ws + L.e1m;
  if (planes) pa.et1_hi = e1_hi, pa.et1_lo = e1_hi + MD;
  else pa.et1 = ws + L.et1;
  pa.s2_part = ws + L.s2_part;
  pa.chunks = L.chunks;
  DRIN_TRY(launch_pair_layer1(pa, st));
  // (7), (8) layer 2; its contraction writes over h_text
  return run_folded_tail(cfg, params, pb, P, L.chunks, ws + L.s2_part, vm1, ws + L.agg2, ws + L.mt2, ws + L.hm2, ws + L.e1m, ws + L.h_text,
                         planes ? nullptr : ws + L.et1, planes ? e1_hi : nullptr, planes, msk, psk, scores, st);
}

}  // namespace drin

extern "C" {

int32_t drin_workgroups_per_mention(const drin_config* cfg, int32_t cached) {
  if (validate_config(cfg) != DRIN_OK || fused_supported(cfg) != DRIN_OK) return 0;
  if (cached) return cached_chunks_per_mention(*cfg);
  FusedLayout L;
  L.build(*cfg, folded_plan(*cfg, false));
  return L.chunks;
}

int32_t drin_image_contraction_side_tiles(const drin_config* cfg, int32_t indexed) {
  if (validate_config(cfg) != DRIN_OK || fused_supported(cfg) != DRIN_OK) return 0;
  return (int32_t)folded_plan(*cfg, indexed != 0).S;
}

int32_t drin_image_contraction_passes(const drin_config* cfg, int32_t indexed) {
  if (validate_config(cfg) != DRIN_OK || fused_supported(cfg) != DRIN_OK) return 0;
  return folded_plan(*cfg, indexed != 0).passes;
}

int drin_index_status(int32_t* index_status, void* stream) {
  if (!index_status) {
    set_error("drin_index_status: NULL argument");
    return DRIN_E_NULL;
  }
  DRIN_BIND_DEVICE(stream, index_status, "drin_index_status");
  int32_t w[4] = {0, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(w, index_status, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "drin_index_status");
  if (w[0] == 0) return DRIN_OK;
  e = hipMemsetAsync(index_status, 0, sizeof(w), (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "drin_index_status(reset)");
  const long long value = (long long)(((uint64_t)(uint32_t)w[3] << 32) | (uint32_t)w[2]);
  set_error("entity_index out of range: candidate row %lld at pair %d (b * N + n) is outside the entity tables - the row was clamped "
            "and a WRONG entity scored; drin/data.py:87-93 raises IndexError here", value, (int)w[1]);
  return DRIN_E_INDEX;
}

size_t drin_fused_workspace_bytes(const drin_config* cfg) {
  if (validate_config(cfg) != DRIN_OK || fused_supported(cfg) != DRIN_OK) return 0;
  FusedLayout L;
  L.build(*cfg, folded_plan(*cfg, false));
  return L.total * sizeof(float);
}

int drin_forward_prepared(const drin_config* cfg, const drin_batch* b, const drin_params* params, const void* prepared,
                          void* workspace, size_t workspace_bytes, float* scores, void* stream) {
  return drin_forward_prepared_head(cfg, b, params, prepared, workspace, workspace_bytes, scores, nullptr, stream);
}

int drin_forward_prepared_head(const drin_config* cfg, const drin_batch* b, const drin_params* params, const void* prepared,
                               void* workspace, size_t workspace_bytes, float* scores, const drin_mention_head* head, void* stream) {
  DRIN_BIND_DEVICE(stream, workspace, head ? "drin_forward_prepared_head" : "drin_forward_prepared");
  RoctxRange range("drin_forward_prepared");
  DRIN_TRY(validate_config(cfg));
  DRIN_TRY(validate_head(head, "drin_forward_prepared_head"));
  DRIN_TRY(fused_supported(cfg));
  // (launch_entity_stream's own limit, asked before the first launch: the image product, the folded head and the q product run
  //  ahead of the stream pass and would have written the workspace by the time it refused)
  if (!entity_stream_fits(cfg->batch)) {
    set_error("drin_forward_prepared: batch = %d: the entity stream pass is built for at most %d mentions per call; split the batch",
              cfg->batch, kMaxGridY);
    return DRIN_E_SHAPE;
  }
  if (!b || !params || !prepared || !workspace || !scores) {
    set_error("drin_forward_prepared: NULL argument");
    return DRIN_E_NULL;
  }
  const FoldedPlan plan = folded_plan(*cfg, b->entity_index != nullptr);
  FusedLayout L;
  L.build(*cfg, plan);
  if (workspace_bytes < L.total * sizeof(float) || !aligned16(workspace)) {
    set_error("drin_forward_prepared: workspace has %zu bytes (needs %zu) or is not 16-byte aligned", workspace_bytes,
              L.total * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  return forward_prepared_on_stream(cfg, b, params, prepared, workspace, scores, (hipStream_t)stream, head, plan, L);
}

}  // extern "C"
