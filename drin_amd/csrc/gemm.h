// The GEMM module's host interface: one description per product kind (NT, TN, NN), the launchers and groups that take them,
// the ordered slice sums they land through, the route records the probes read, and the weight-gradient pass built on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/drin_hip.h"
#include "scratch_sizes.h"

namespace drin {

// ---- ordered slice sums (gemm_f32.hip) -----------------------------------------------------------
// y[r, c] += sum over the destination's segments (in the order they were added), over each segment's slices (in order), of
// partial[slice][r][c].  Every split reduction of the backward pass - the weight-gradient products split over the B N pairs,
// their bias sums, the column sums - stores its slices plainly and lands in its destination through this ONE kernel: no
// fp32 atomics anywhere, the same bits every run.  Two products that add to the same destination (dW_h takes the mention
// and the entity rows) become two segments of one entry, summed by one thread in a fixed order.
struct SliceSum {
  static constexpr int MAX_DST = 32, MAX_SEG = 40;
  struct Dst {
    float* y;
    int64_t ldy;
    int rows, c4;          // the destination is rows x 4 c4 floats
    unsigned first_block;
    int seg_head, seg_tail;
  } dst[MAX_DST];
  struct Seg {
    const float* partial;  // [slices][rows][4 c4], contiguous
    int slices, next;
  } seg[MAX_SEG];
  int n = 0, n_seg = 0;
  // DRIN_E_ALIGN / DRIN_E_SHAPE outside the contract (cols % 4, 16-byte alignment of y / partial, ldy % 4 unless rows == 1,
  // the same y with another shape, more than MAX_DST destinations / MAX_SEG segments)
  int add(float* y, int64_t ldy, int rows, int cols, const float* partial, int slices);
};
int launch_slice_sum(SliceSum& s, hipStream_t st);   // no-op for an empty one

// ---- which NT GEMM form ran (drin_gemm_probe) -----------------------------------------------------
// This thread's record of the last NT product's GEMM kernel, written by the dispatch code next to the launch itself (a handful of
// host stores): tests assert it instead of restating the size gates, so a gate that moves cannot leave a form silently untested.
drin_gemm_route& gemm_route();
struct RouteNote {
  int family, bm, bn;
  bool w_planes = false, a_lo = true, f16 = false, persist = false, indexed = false, accumulate = false;
  int ksplit = 1, splits = 1;
  int64_t tiles = 0, whole_tiles = 0, tile0 = 0, work_items = 0;
};
inline void note_route(const RouteNote& n) {
  drin_gemm_route& r = gemm_route();
  r.launches += 1;
  r.family = n.family, r.bm = n.bm, r.bn = n.bn;
  r.w_planes = n.w_planes, r.a_lo = n.a_lo, r.f16 = n.f16, r.persist = n.persist, r.indexed = n.indexed, r.accumulate = n.accumulate;
  r.ksplit = n.ksplit, r.splits = n.splits;
  r.tiles = n.tiles, r.whole_tiles = n.whole_tiles, r.tile0 = n.tile0, r.work_items = n.work_items;
}

// ---- what the backward products did (drin_wgrad_probe) ----------------------------------------------
// This thread's record of the weight-gradient, bias-gradient and dX launches, written by the dispatch code next to each launch like
// the NT record above.  The probe names its products here while it runs; a launcher that carries one of them (the same dy, x and dw)
// notes what it chose for it.  The record is written ONLY while the probe runs on this thread (wgrad_route() is NULL otherwise):
// a product call stores nothing and counts nothing, so no counter grows over the life of a training process.
struct WgradTrace {
  drin_wgrad_route route;
  const drin_wgrad_product* product;
  int n;
};
WgradTrace& wgrad_trace();
inline drin_wgrad_route* wgrad_route() {   // the record while drin_wgrad_probe runs on this thread, else NULL
  WgradTrace& t = wgrad_trace();
  return t.product != nullptr ? &t.route : nullptr;
}
inline void note_wgrad_product(const float* dy, const float* x, const float* dw, int kernel, int slices, int64_t rows_per_slice, bool in_place,
                               bool db_rode, int launch = 0) {   // launch: -1 when noted after its note_wgrad_gemm_launch
  WgradTrace& t = wgrad_trace();
  for (int i = 0; i < t.n; ++i) {
    const drin_wgrad_product& p = t.product[i];
    if (p.dy != dy || p.x != x || p.dw != dw) continue;
    drin_wgrad_product_route& r = t.route.product[i];
    r.kernel = kernel, r.slices = slices, r.rows_per_slice = rows_per_slice, r.in_place = in_place, r.db_rode = db_rode;
    r.launch = t.route.gemm_launches + launch;
  }
}
inline void note_wgrad_gemm_launch(int64_t workgroups) {   // after the note_wgrad_product calls of the products it carries
  drin_wgrad_route* r = wgrad_route();
  if (r == nullptr) return;
  if (r->gemm_launches >= 0 && r->gemm_launches < DRIN_WGRAD_ROUTE_LAUNCHES) r->grid[r->gemm_launches] = workgroups;
  r->gemm_launches += 1;
}
inline void note_wgrad_colsum(const float* dy, const float* db, int row_slices) {
  WgradTrace& t = wgrad_trace();
  for (int i = 0; i < t.n; ++i)
    if (t.product[i].dy == dy && t.product[i].db == db) t.route.product[i].db_slices = row_slices;
}

// ---- what a linear product is: one description per kind, taken by every launcher of that kind --------------------------
// After the description a launcher's arguments come in one order: precision (where it has one), stream, scratch.
struct GemmScratch {  // split-K / tail-split / slice partials of a product; none: {}
  float* p = nullptr;
  size_t floats = 0;
};
// `floats` floats at base + off (a Layout's offset and size, or a caller's buffer with off = 0); none when either is missing
inline GemmScratch scratch_at(float* base, size_t off, size_t floats) {
  return base != nullptr && floats ? GemmScratch{base + off, floats} : GemmScratch{};
}
struct Mat {  // an fp32 operand: the pointer never travels without its row stride
  const float* p = nullptr;
  int64_t ld = 0;
};
// y[rows, n_out] (+)= x[rows, k_red] w[n_out, k_red]^T + bias[n_out]
struct NtProduct {
  Mat x, w;
  const float* bias = nullptr;
  float* y = nullptr;
  int64_t ldy = 0, rows = 0;
  int n_out = 0, k_red = 0;
  const void *w_hi = nullptr, *w_lo = nullptr;   // optional pre-split bf16 planes of w (launch_split_planes_batch), row stride w.ld
  bool accumulate = false;                       // y += ... instead of y = ...
  const int64_t* x_index = nullptr;              // row m of x is row x_index[m] of a table (split-bf16 kernels only)
  // The row-side operand STORED as bf16 (a bf16 entity table, read in place): x_bf16 addresses [rows][x.ld]
  // bf16 and x.p is NULL.  launch_gemm_nt takes one of two routes (nt_bf16_rows_as_planes, scratch_sizes.h).  PLANES: split-bf16
  // precision, k_red % 32 == 0, x.ld % 8 == 0, 16-byte aligned, w_hi / w_lo given - the rows ARE the hi plane of
  // launch_gemm_x3_planes with no lo plane (exact in bf16: two MFMAs per tile pair), their bytes read once, as stored.  WIDEN:
  // anything else - the rows are widened exactly into x_widen (rows k_red floats; DRIN_E_WORKSPACE without it) and the product
  // runs on them as it would on fp32 rows: the same kernel on the same values.  No bias, no accumulate, no x_index.
  const void* x_bf16 = nullptr;
  GemmScratch x_widen;
  // the same product on the planes a workspace holds: n_out k_red bf16 of hi, then as many of lo (NULL: none)
  NtProduct with_planes(const float* hi_then_lo) const {
    NtProduct q = *this;
    q.w_hi = hi_then_lo;
    q.w_lo = hi_then_lo ? reinterpret_cast<const uint16_t*>(hi_then_lo) + (int64_t)n_out * k_red : nullptr;
    return q;
  }
  NtProduct adding() const {   // the same product as y += ...
    NtProduct q = *this;
    q.accumulate = true;
    return q;
  }
};
// dw[n_out, k_red] += dy[rows, n_out]^T x[rows, k_red], split over the rows
struct TnProduct {
  Mat dy, x;
  float* dw = nullptr;
  int64_t lddw = 0, rows = 0;
  int n_out = 0, k_red = 0;
  const int64_t* x_index = nullptr;   // reduction row m of x is row x_index[m] of a table - the gathered form never materialised
  float* db = nullptr;                // optional [n_out], += the column sums of dy: taken by TnGroup::add and WeightGradPass::add only
};
// dx[rows, n_out] (+)= dy[rows, k_red] w[k_red, n_out]
struct NnProduct {
  Mat dy, w;
  float* dx = nullptr;
  int64_t lddx = 0, rows = 0;
  int n_out = 0, k_red = 0;
  bool accumulate = false;
};

// ---- GEMM (gemm_f32.hip) ------------------------------------------------------------------------
// (splitk: optional scratch; mention-sized exact-fp32 products with a long reduction (scratch_sizes.h: small_splitk_shape)
//  then split K over workgroups into it and reduce in order - deterministic - instead of walking K serially in 24 tiles)
// (w_hi / w_lo: taken when the product runs split-bf16, w contiguous and k_red a multiple of 32)
int launch_gemm_nt(const NtProduct& p, int precision, hipStream_t st, GemmScratch splitk = {});
// same contraction, operands split into bf16 hi + lo, three bf16 MFMAs, fp32 accumulate (gemm_bf16x3.hip)
// (w_hi, w_lo: then w itself is not read and the weights stream by LDS-DMA)
// (tail: optional scratch; a partly filled last round of 256 x 256 tiles is then split along K over the idle CUs)
int launch_gemm_nt_bf16x3(const NtProduct& p, hipStream_t st, GemmScratch tail = {});
// one fp16 plane of x under ONE power-of-two scale: out = fp16(x / s), s -> scale[0] (scale: two floats, [1] is scratch); n % 4 == 0
int launch_to_f16_scaled(const float* x, void* out, int64_t n, float* scale, hipStream_t st);
// weight-gradient contraction dw[n, k] += sum_m dy[m, n] x[m, k] in split-bf16 (gemm_tn_bf16x3.hip)
bool gemm_tn_bf16x3_fits(const TnProduct& p);
// (scratch: [slices][N][K] floats, at least N K of them, 16-byte aligned - the slices store plainly and are added to dw in
//  order: DRIN_E_WORKSPACE without it)
int launch_gemm_tn_bf16x3(const TnProduct& p, hipStream_t st, GemmScratch scratch);
// what launch_gemm_tn_bf16x3 / launch_gemm_tn_group need of dw and the scratch besides gemm_tn_bf16x3_fits
bool gemm_tn_bf16x3_scratch_ok(const TnProduct& p, GemmScratch scratch);
// up to kTnGroupMax such products in ONE launch (+ one for the slice reduction): the chip's workgroups are dealt over all of
// them (scratch for a whole pass: tn_group_floats)
struct TnGroup {
  static constexpr int MAX = kTnGroupMax;
  TnProduct item[MAX];
  int n = 0;
  // no-op for dw == NULL; DRIN_E_SHAPE outside gemm_tn_bf16x3_fits or past MAX
  // (db: the bias gradient that belongs to dW = dY^T X, from the rows the product stages anyway)
  int add(const TnProduct& p);
};
// (defer: the slice sums are appended to it instead of being launched - the caller launches it, after which the scratch
//  may be reused; NULL: launched here)
int launch_gemm_tn_group(const TnGroup& g, hipStream_t st, GemmScratch scratch, SliceSum* defer = nullptr);
// same, operands pre-split into bf16 hi / lo planes (gemm_x3_planes.hip); K % 32 == 0
// (a_lo NULL: A exact in bf16, two MFMAs per tile pair)
// RowTiles: a slice of a product on the four-phase 256 x 256 kernels - row tiles [begin, end) (end < 0: to the last one).  wgs > 0:
// that many PERSISTENT workgroups walk the slice's tiles (tile_walk.h) instead of one workgroup per tile; such a slice holds whole
// tiles only.  The product's tail split (K-slices of a partly filled last round + tail add) goes with the plain launch that ends at
// the last row tile.  Every tile is computed by the same code with the same split whichever slice covers it: slices that
// partition the row tiles write, bit for bit, what one launch of the whole product writes.
struct RowTiles {
  int64_t begin = 0, end = -1;
  int wgs = 0;
};
// how many tiles of a `tiles`-tile product (reduction length K, this tail scratch) are computed whole, i.e. outside the tail split
int64_t gemm_p4_whole_tiles(int64_t tiles, int K, bool tail_scratch, size_t tail_floats);
int launch_gemm_x3_planes(const void* a_hi, const void* a_lo, int64_t lda, const void* b_hi, const void* b_lo,
                          int64_t ldb, const float* bias, float* y, int64_t ldy, int64_t M, int N, int K,
                          hipStream_t st, GemmScratch splitk = {}, RowTiles rows = RowTiles());
// y = a b^T in ONE fp16 MFMA pass on single fp16 planes (DRIN_PREC_BF16X3_IF16; gemm_x3_planes.hip): a_f16 [M][K] holds row m of the
// activation divided by row_scale[m], b_f16 [N][K] the weight divided by *b_scale (powers of two: exact); output row m is multiplied
// by row_scale[m] * *b_scale.  Whole 256 x 256 tiles, K % 64 == 0, 16-byte aligned: gemm_f16_planes_fits, DRIN_E_UNSUPPORTED otherwise.
bool gemm_f16_planes_fits(const void* a_f16, int64_t lda, const void* b_f16, int64_t ldb, const float* y, int64_t ldy, int64_t M, int N, int K);
int launch_gemm_f16_planes(const void* a_f16, int64_t lda, const void* b_f16, int64_t ldb, const float* row_scale, const float* b_scale,
                           float* y, int64_t ldy, int64_t M, int N, int K, hipStream_t st, GemmScratch tail = {});
// the four-phase pipeline (gemm_x3_planes.hip) on an fp32 x against pre-split weight planes (w_hi, w_lo): whole 256 x 256 tiles
int launch_gemm_nt_bf16x3_p4(const NtProduct& p, hipStream_t st, GemmScratch tail = {}, RowTiles rows = RowTiles());
// y[tail tile] += its ksplit - 1 partial 256 x 256 tiles, in order (tail split of the two split-bf16 NT kernels)
int launch_tail_add_256(const float* tail, float* y, int64_t ldy, int64_t M, int N, unsigned col_tiles, unsigned full,
                        unsigned tail_tiles, int ksplit, hipStream_t st);
// y[m, n] (+)= bias[n] + sum_z partial[z][m][n] in order (the reduction step of every split-K product; gemm_f32.hip)
int launch_splitk_reduce(const float* partial, int splits, int64_t part_stride, const float* bias, float* y, int64_t ldy,
                         int64_t M, int N, bool accumulate, hipStream_t st);
// fp32 -> bf16 hi / lo planes (n % 4 == 0)
int launch_split_planes(const float* x, void* hi, void* lo, int64_t n, hipStream_t st);
// up to 32 tensors split in ONE launch; planes_out holds numel bf16 of hi followed by numel bf16 of lo (= numel floats).
// launch_transpose_split_batch: the same for the TRANSPOSES of equally shaped [rows][cols] matrices.
struct SplitBatch {
  const float* src[32];
  float* planes[32];
  int64_t n4[32];
  int n = 0;
  int add(const float* w, float* planes_out, int64_t numel);   // no-op for w == NULL
};
int launch_split_planes_batch(const SplitBatch& b, hipStream_t st);
int launch_transpose_split_batch(const SplitBatch& b, int rows, int cols, hipStream_t st);
// out [cols][rows] = in [rows][cols]^T, fp32 (fused_kernels.hip)
int launch_transpose(const float* in, float* out, int rows, int cols, hipStream_t st);
// dx[m, n] (+)= sum_k dy[m, k] * w[k, n]        (used by backward: dX = dY * W)
// Pair-sized products in split-bf16 precision (gemm_nn_takes_bf16x3) run on the split-bf16 NT kernel against w^T when the
// caller supplies it in one of the forms below; everything else takes the exact fp32 NN kernel (splitk: as launch_gemm_nt's).
struct WtForms {
  const float* planes = nullptr;   // bf16 hi / lo planes of w^T [N][K], already written (a caller that writes them asks the predicate)
  GemmScratch scratch;             // else: room for an fp32 w^T, transposed here; taken with w contiguous and N K floats of it
  GemmScratch tail;                // the NT kernel's tail-split scratch (launch_gemm_nt_bf16x3)
};
bool gemm_nn_takes_bf16x3(int precision, int64_t M, int N, int K);
int launch_gemm_nn(const NnProduct& p, int precision, hipStream_t st, GemmScratch splitk = {}, const WtForms& wt = WtForms());
// up to 8 MENTION-sized (at most kMentionSizedMaxRows rows) exact-fp32 products of ONE kind in one launch: weight gradients
// (item[], add_tn) or y = x w^T + bias (nt[], add_nt)
struct F32GemmGroup {
  static constexpr int MAX = 8;
  TnProduct item[MAX];
  NtProduct nt[MAX];
  int n = 0;
  int add_tn(const TnProduct& p);
  // only for products that passed gemm_nt_f32_group_fits - the ones launch_gemm_nt would run as the exact-fp32 split-K kernel +
  // slice reduction
  int add_nt(const NtProduct& p);
};
// (a product alone on its destination with one slice adds to it in place; any other stores its slices to the scratch and
//  goes through the slice sum - defer as for launch_gemm_tn_group; floats needed: small_tn_scratch_floats per item)
int launch_gemm_tn_f32_group(const F32GemmGroup& g, hipStream_t st, GemmScratch scratch, SliceSum* defer = nullptr);
bool gemm_nt_f32_group_fits(const NtProduct& p, int precision);
int launch_gemm_nt_f32_group(const F32GemmGroup& g, hipStream_t st, GemmScratch scratch);
// Two NT products that do not depend on each other.  When both would run as the exact-fp32 split-K kernel + slice reduction
// (a few hundred rows: 6-9 us + 5 us each, nearly all fill and drain) the two kernels share a launch and so do the two
// reductions - same slices, same order, same bits; otherwise two launch_gemm_nt calls.
int launch_gemm_nt_pair(const NtProduct& a, const NtProduct& b, int precision, hipStream_t st, GemmScratch splitk);
// dw[n, k] += sum_m dy[m, n] * x[m, k]          (used by backward: dW = dY^T * X), split over m; no-op for dw == NULL
int launch_gemm_tn(const TnProduct& p, int precision, hipStream_t st, GemmScratch scratch = {});
// the kernel such a product takes, decided here only: split-bf16 MFMA (gemm_tn_bf16x3_fits, gemm_tn_bf16x3_scratch_ok) |
// exact fp32, mention-sized (rows <= kMentionSizedMaxRows): 64 x 64 tiles, small_tn_slices(rows) slices | exact fp32, 128 x 128 tiles
enum TnKernel { TN_BF16X3, TN_F32_SMALL, TN_F32_LARGE };
TnKernel gemm_tn_kernel(const TnProduct& p, int precision, GemmScratch scratch);


// ---- bias-gradient column sums (backward_kernels.hip) --------------------------------------------------
// out[c] += sum_rows x[row, c].  The rows are dealt over up to kColsumMaxSlices workgroups per 256 columns, whose sums go to
// the scratch ([slices][C] floats) and from there to out in order (SliceSum); without scratch one workgroup per 256 columns
// walks all rows and adds to out itself - slower, the same kind of result: no atomics either way.
int launch_colsum(const float* x, float* out, int64_t rows, int C, hipStream_t st, float* scratch = nullptr,
                  size_t scratch_floats = 0);
// up to kColsumBatchMax such column sums in ONE launch
struct ColsumBatch {
  const float* x[kColsumBatchMax];
  float* out[kColsumBatchMax];
  int64_t rows[kColsumBatchMax];
  int64_t ld[kColsumBatchMax];
  int c4[kColsumBatchMax];
  int by[kColsumBatchMax];
  int n = 0;
  // no-op for dst == NULL or nrows <= 0; ld_src: the row stride of src in floats (0: C, contiguous rows)
  int add(const float* src, float* dst, int64_t nrows, int C, int64_t ld_src = 0);
};
// (scratch: sum over the entries of by * C floats <= colsum_batch_floats(C); defer as for launch_gemm_tn_group)
int launch_colsum_batch(const ColsumBatch& b, hipStream_t st, float* scratch, size_t scratch_floats, SliceSum* defer = nullptr);

// ---- the weight and bias gradients of one backward pass (gemm_f32.hip) -----------------------------------------------
// dW (+)= dY^T X, db (+)= column sums of dY.  The pair-sized products of the whole pass (dW_h, dW_v of every layer, the two entity
// encoders) run as ONE launch at the end: alone, each deals its ~15-stage slices over the chip between a pipeline fill and a partial
// tile per workgroup; together the workgroups walk ~4x longer slices.  The mention-sized ones (exact fp32) and the bias column sums:
// one launch each as well; a full group (deeper than three layers) goes in instalments.  Vector edges: products run where they arise.
struct WeightGradPass {
  const int prec;       // DRIN_PREC_F32 or a split-bf16 one
  const bool vec;       // vector edges
  const hipStream_t st;
  const GemmScratch tn, small, colsum;   // Layout::tn_part (it holds a slice of every product), small_part, colsum_part
  // no-op for dw == NULL.  db: the bias gradient that goes with the product = the column
  // sums of dy; the split-bf16 group takes them from the rows it stages, any other product's join the batch of column sums
  int add(const TnProduct& p);
  SliceSum ln_sums;        // launch_layernorm_gelu_bwd2's deferred second level: lands with (the first part of) finish
  int flush_bias_sums() { const int rc = launch_colsum_batch(bias_sums, st, colsum.p, colsum.floats); bias_sums = ColsumBatch(); return rc; }
  // what was added up to here lands in the GCN layers' gradients, what follows in the vertex encoders'
  void layers_done() { layer_sums = bias_sums.n, layer_small = dw_small.n, layer_group = dw_group.n; }
  int finish(void* layers_ready_event);   // NULL: everything lands in one part; else the layers' part, the hipEvent_t, the encoders'
  ColsumBatch bias_sums;
  F32GemmGroup dw_small;
  TnGroup dw_group;
  int layer_sums = 0, layer_small = 0, layer_group = 0;   // entries of each that belong to the GCN layers (an instalment takes them all: 0 remain)
};
size_t small_group_worst_case_floats(const drin_config& c, size_t tn_part_floats);   // of dw_small at once (drin_host_selftest)

}  // namespace drin
