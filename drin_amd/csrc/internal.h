// Host-side internals of libdrin_hip.so: error and device plumbing, the launch wrappers of the row kernels, workspace self-checks
// (the GEMM module's interface: gemm.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

#include "../../include/drin_hip.h"
#include "gemm.h"
#include "scratch_sizes.h"

namespace drin {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define DRIN_CHECK_LAUNCH(what)                                  \
  do {                                                           \
    hipError_t _e = hipGetLastError();                           \
    if (_e != hipSuccess) return ::drin::hip_fail(_e, what);     \
  } while (0)

#define DRIN_TRY(expr)              \
  do {                              \
    int _s = (expr);                \
    if (_s != DRIN_OK) return _s;   \
  } while (0)

// Brackets the launches issued during its lifetime with hipEvents when a profile is open on this
// thread (drin_profile_begin); otherwise free.
struct KernelTimer {
  KernelTimer(int kernel_class, hipStream_t st);
  ~KernelTimer();
  int slot;
  hipStream_t stream;
};
// the launches of `launch` under a KernelTimer of class `cls`, then the launch check
template <typename F>
int timed(int cls, hipStream_t st, const char* what, F&& launch) {
  KernelTimer timer(cls, st);
  launch();
  DRIN_CHECK_LAUNCH(what);
  return DRIN_OK;
}

// The device a call runs on is the device of the caller's STREAM, not whatever device happens to be current on the calling
// thread: every entry point that launches opens a DeviceScope first.  It asks the stream (hipStreamGetDevice) - or, for the NULL
// stream, the device that owns `device_pointer` (hipPointerGetAttributes; the NULL stream of THAT device is then used) - makes that
// device current for the duration of the call and restores the previous one on the way out.  A process whose current device is 0
// may therefore score tensors that live on device 1 through a stream of device 1: kernel attributes, launches, events and memsets
// all land on device 1.  Scopes nest (an entry point calling another one); the innermost one answers call_device().
struct DeviceScope {
  DeviceScope(void* stream, const void* device_pointer, const char* entry_point);
  ~DeviceScope();
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  int status;        // DRIN_OK, or DRIN_E_HIP with the message set
  int prev, dev, outer;
  bool switched;
};
// device of the innermost DeviceScope of this thread (outside any scope: the current device)
int call_device();
#define DRIN_BIND_DEVICE(stream, device_pointer, entry_point)               \
  ::drin::DeviceScope _device_scope((stream), (device_pointer), (entry_point)); \
  if (_device_scope.status != DRIN_OK) return _device_scope.status

// One side stream and a fork / join event pair per device, owned by the library for the life of the process: work of a call that
// does not depend on what the caller's stream is doing (fused_forward.hip: the first row tiles of x_i C_i^T) runs there between
// `fork` (recorded on the caller's stream) and `join` (recorded on the side stream, waited for by the caller's).  Non-blocking
// stream, events without timing; created by the first call that needs them - never inside a stream capture, whose calls do not
// ask for it.  `order` serialises the record + wait pairs of calls from different threads, which share the pair of events.
struct SideLane {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  std::mutex order;
  std::atomic<bool> ready{false};
};
int side_lane(SideLane** out);   // the lane of call_device()

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: one high-water mark per (call site,
// device), so a process that runs on cuda:0 and later on cuda:1 opts in on both, and a later call that needs more LDS
// than the first one raises it.  The device is the CALL's (DeviceScope), which the entry point has made current.
// Atomics: the caller's thread and autograd's may race here harmlessly (idempotent call).
struct DynLdsOptIn {
  std::atomic<int> bytes[64] = {};
};
inline int ensure_dynamic_lds(DynLdsOptIn& s, const void* kernel, int bytes, const char* what) {
  const int dev = call_device();
  std::atomic<int>& mark = s.bytes[dev & 63];
  if (mark.load(std::memory_order_relaxed) >= bytes) return DRIN_OK;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return hip_fail(e, what);
  mark.store(bytes, std::memory_order_relaxed);
  return DRIN_OK;
}

// roctx range over one entry point (rocprofv3 --marker-trace shows the calls of the path as named ranges above their
// kernels).  Inert unless DRIN_ROCTX is set in the environment when the first entry point runs; the roctx library is
// dlopen'ed then (librocprofiler-sdk-roctx.so, else libroctx64.so) - the library has no link-time dependency on it.
struct RoctxRange {
  explicit RoctxRange(const char* name);
  ~RoctxRange();
  bool pushed;
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// grid of the one-wave-per-pair kernels (device_utils.h: wave_pair)
inline dim3 pair_grid(int B, int N) {
  return (B > 1 && B <= kMaxGridY) ? dim3((unsigned)cdiv(N, 4), (unsigned)B) : dim3((unsigned)cdiv((int64_t)B * N, 4));
}
// [0, count) in slices of at most kMaxGridY (scratch_sizes.h), in order: launch(first, n) per slice, none for count <= 0; the
// first status that is not DRIN_OK ends the walk and is returned.  The launch loop of every (column quads, mention, ...) grid:
// the body moves each pointer by `first` mentions and takes n as grid.y
template <typename F>
int for_grid_slices(int64_t count, F&& launch) {
  for (int64_t first = 0; first < count; first += kMaxGridY) {
    const int64_t left = count - first;
    DRIN_TRY(launch(first, (int)(left < kMaxGridY ? left : kMaxGridY)));
  }
  return DRIN_OK;
}
// workgroups of the one-wave-per-row grid-stride launchers (launch_layernorm_res, launch_gather_rows, launch_row_inv_norms):
// four rows each, past the cap a wave walks several rows
constexpr int64_t kMaxRowBlocks = (int64_t)kMaxGridY * 16;
inline int64_t row_blocks(int64_t rows) { return cdiv(rows, 4) < kMaxRowBlocks ? cdiv(rows, 4) : kMaxRowBlocks; }
// A launcher with a (column quads, mention, ...) grid that does not slice refuses past kMaxGridY mentions, and the entry points
// that reach it ask the same predicate among their argument checks (api.hip: layers_call_fits): a size is refused before the
// first launch of a call or not at all
inline bool edge_pre_vec_bwd_fits(int B) { return B <= kMaxGridY; }   // k_edge_pre_vec_bwd_fu (vector_kernels.hip)
inline bool entity_stream_fits(int B) { return B <= kMaxGridY; }      // k_entity_stream (fused_kernels.hip); drin_forward_prepared asks

// ---- pooling and static edges of the layer-by-layer entry points (api.hip; Layout, Pooled: layout.h) -------------------
struct Layout;
struct Pooled;
int run_pooling(const drin_config* c, const drin_batch* b, const Layout& L, float* ws, Pooled* out, hipStream_t st,
                const drin_mention_head* head = nullptr);
int run_static_edges(const drin_config* c, const drin_batch* b, const Pooled& P, float* edges, hipStream_t st);

// ---- streaming / pooling kernels (stream_kernels.hip) -------------------------------------------
// out[g, c] = mean_s in[g, s, c]
int launch_axis_mean(const float* in, float* out, int64_t groups, int inner, int cols, hipStream_t st);
// Avg.avg (ghmfc.py:54-60): out[b, :] = mean(seq[b, start[b]:end[b], :])
int launch_span_mean(const float* seq, const int64_t* start, const int64_t* end, float* out, int B, int L, int D,
                     hipStream_t st);
// the same two for features stored as bf16 (drin_config.feature_dtype = DRIN_FEAT_BF16)
int launch_axis_mean_bf16(const void* in, float* out, int64_t groups, int inner, int cols, hipStream_t st);
int launch_span_mean_bf16(const void* seq, const int64_t* start, const int64_t* end, float* out, int B, int L, int D,
                          hipStream_t st);
// ghmfc.py:245-249: out[p, :] = mean(feat[p, 1:ntok-1, :]), ntok = sum(mask[p, :])
int launch_entity_token_mean(const float* feat, const int64_t* mask, float* out, int64_t pairs, int T, int D,
                             hipStream_t st);
int launch_entity_token_mean_bf16(const void* feat, const int64_t* mask, float* out, int64_t pairs, int T, int D,
                                  hipStream_t st);
// the same mean of row index[p] of the tables text [E, T, D] / mask [E, T] (fp32): the index is clamped into [0, E - 1] before
// it is used and reported into status (int32[4] or NULL; device_utils.h: report_bad_index) as pair pair_base + p
int launch_entity_token_mean_indexed(const float* text, const int64_t* mask, const int64_t* index, int64_t num_rows, float* out,
                                     int64_t pairs, int T, int D, int32_t* status, int64_t pair_base, hipStream_t st);
// both with a pooling (drin_entity_pooling, checked by the caller): DRIN_POOL_AVG is the two launches above, DRIN_POOL_MAX the
// maximum over the same slice (a NaN inside it wins; an empty slice gives a NaN row)
int check_entity_pooling(const char* who, int pooling);
int launch_entity_token_pool(const float* feat, const int64_t* mask, float* out, int64_t pairs, int T, int D, int pooling,
                             hipStream_t st);
int launch_entity_token_pool_indexed(const float* text, const int64_t* mask, const int64_t* index, int64_t num_rows, float* out,
                                     int64_t pairs, int T, int D, int pooling, int32_t* status, int64_t pair_base, hipStream_t st);
// the other row kernels of GHMFC's table form (ghmfc_table.hip), the same clamp and report:
// out[i, :] = table[index[i], :] for [E, width] fp32 rows
int launch_gather_rows(const float* table, const int64_t* index, int64_t num_rows, float* out, int64_t count, int width,
                       int32_t* status, int64_t pair_base, hipStream_t st);
// out[b * N + n] = cos(x[b, :], rows[index[b * N + n], :]): k_cosine_rows' lane loop on a clamped row.  row_dtype: how `rows` are
// stored - DRIN_FEAT_F32, or DRIN_FEAT_BF16 (widened exactly, lane by lane: the bits of the fp32 rows' launch on the widened table;
// the launch is then timed as k_cosine_gather_bf16)
int launch_cosine_gather(const float* x, const void* rows, int row_dtype, const int64_t* index, int64_t num_rows, float* out, int B, int N,
                         int D, float eps, int32_t* status, int64_t pair_base, hipStream_t st);
// out[i] = (float)rows_bf16[i], n % 4 == 0, both 16-byte aligned: the widen route of an NT product on bf16-stored rows (gemm.h)
int launch_widen_rows(const void* rows_bf16, float* out, int64_t n, hipStream_t st);
// out[b*N + n] = scale * cos(x[b, :], y[(b*N + n) * y_stride : +D])
// (sim1 / sim2 -> out1 / out2: optional [B*N] arrays divided by `div` in the same pass: the CLIP edges of model.py:203)
int launch_cosine_rows(const float* x, const float* y, int64_t y_stride, float* out, int B, int N, int D, float eps,
                       float scale, hipStream_t st, const int64_t* y_index = nullptr, const float* sim1 = nullptr,
                       const float* sim2 = nullptr, float* out1 = nullptr, float* out2 = nullptr, float div = 1.0f);
// the GHMFC row kernels (ghmfc_rows.hip) that the scoring forward composes (ghmfc_forward.hip)
constexpr int kLnMaxWidth = 2048;   // Row<8>
int launch_layernorm_res(const float* x, const float* res, const float* gamma, const float* beta, float* y, int64_t rows, int E,
                         float eps, hipStream_t st, float* mean = nullptr, float* rstd = nullptr);
int launch_seq_max(const float* x, float* out, int B, int S, int E, hipStream_t st, int* idx = nullptr);
int launch_gate_mix(const float* tl, const float* vl, const float* ws, const float* bs, float* out, int B, int D, hipStream_t st);
// model.py:84-92: weighted object-pair similarity
int launch_miei(const float* mobj, const float* mscore, const float* eobj, const float* escore, float* out, int B,
                int N, int Km, int Ke, int R, float cos_eps, float miei_eps, float scale, hipStream_t st,
                const int64_t* e_index = nullptr);
// out[i] = in[i] * mul / div
int launch_scale_div(const float* in, float* out, int64_t n, float mul, float div, hipStream_t st);

// ---- which LayerNorm-backward instantiation a width takes (drin_width_class) ------------------------------------------------------
// k_layernorm_gelu_bwd<V> keeps a row in V float4 register slots per lane: V = ceil(D / 256), 0 when the width is not built.  The one
// place this is decided, like the width bands of the folded path's families (fused.h): the launcher and drin_width_class call it.
constexpr int kLnBwdMaxSlots = 4;
inline int ln_bwd_slots(int D) {
  return (D <= 0 || D % 4 || D > 256 * kLnBwdMaxSlots) ? 0 : (D / 4 + 63) / 64;
}

// ---- GCN elementwise / reduction kernels (gcn_kernels.hip) --------------------------------------
// both aggregations of a scalar-edge layer in one pass (model.py:143-146 + the :128 inputs; the formulas: the kernel's comment);
// e = [4][edge_stride], vm = [2][B][D], ve = [2][B*N][D]
int launch_layer_aggregate(const float* e, int64_t edge_stride, const float* vm, const float* ve, float* agg_m,
                           float* agg_e, int B, int N, int D, bool live_image, hipStream_t st);
// model.py:128: y = gelu(layer_norm(h)) row-wise; optionally keeps mean / rstd for backward
// (act: drin_activation of the vertices, resolved - DRIN_ACT_GELU by default; the name keeps the reference's default)
int launch_layernorm_gelu(const float* h, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                          int64_t rows, int D, float eps, hipStream_t st, int act = DRIN_ACT_GELU);
// two row segments (rows of h, then rows2 of h2) through the same LayerNorm in one launch
int launch_layernorm_gelu2(const float* h, float* y, float* mean, float* rstd, int64_t rows, const float* h2, float* y2,
                           float* mean2, float* rstd2, int64_t rows2, const float* gamma, const float* beta, int D, float eps,
                           hipStream_t st, int act = DRIN_ACT_GELU);
// model.py:148-153 + :133: out[b,n] = sigmoid(mean_d(fu[b,:] fv[b,n,:]) + e[b,n])
// (z_out: optional [4][B*N], the pre-activations - kept for backward when the activation has no derivative-from-output)
int launch_edge_update4(const float* fu, const float* fv, const float* e, float* out, int B, int N, int D,
                        hipStream_t st, int act = DRIN_ACT_SIGMOID, float* z_out = nullptr);

// ---- backward row kernels (backward_kernels.hip) ------------------------------------------------
// d cos(x[b], y[p]) : dx [B, D], dy [B*N, D]; scratch3 holds 3 * B*N floats
int launch_cosine_bwd(const float* x, const float* y, const float* g, float* dx, float* dy, float* scratch3, int B,
                      int N, int D, float eps, hipStream_t st);
// in place: g (dL/dy) -> dL/dh for y = gelu(LN(h)); accumulates dgamma, dbeta and dbias (= column sum of dL/dh);
// partial: ln_bwd_partial_floats(D) floats of scratch for the per-block column sums
int launch_layernorm_gelu_bwd(const float* h, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, float* g, float* dgamma, float* dbeta, float* dbias, float* partial,
                              int64_t rows, int D, hipStream_t st, int act = DRIN_ACT_GELU);
// the same over two row segments that share gamma / beta and the column sums (mention + entity vertices of one layer)
int launch_layernorm_gelu_bwd2(const float* h, const float* mean, const float* rstd, float* g, int64_t rows, const float* h2,
                               const float* mean2, const float* rstd2, float* g2, int64_t rows2, const float* gamma,
                               const float* beta, float* dgamma, float* dbeta, float* dbias, float* partial, int D,
                               hipStream_t st, int act = DRIN_ACT_GELU, SliceSum* defer = nullptr, float* level1_own = nullptr);
// (defer + level1_own [3][kLnBwdLevel1Rows][D] floats, ln_bwd_level1(D, layer) into the partial buffer: the second level of the column-sum reduction joins the caller's slice sum)
// sigmoid backward of the scalar edge update + both entity-side gradients dfv_t, dfv_i in one pass (see the kernel)
// (act | kActFromPre (device_utils.h: 0x100): e_new holds the pre-activation instead of the stored edge; also launch_sigmoid_bwd)
int launch_edge_update_bwd(const float* g, const float* e_new, const float* fu, float* dpre, float* dfv, int B, int N, int D,
                           float scale, hipStream_t st, int act = DRIN_ACT_SIGMOID);
// dpre = g * e' * (1 - e')
int launch_sigmoid_bwd(const float* g, const float* e_new, float* dpre, int64_t n, hipStream_t st, int act = DRIN_ACT_SIGMOID);
// out[b,:] = scale (sum_n w1 v1 + sum_n w2 v2) + u (v2, u optional), two of them over the same rows v1 / v2 in one pass:
// w = [4][B*N]; outA takes planes 0 / 1 and uA, outB planes 2 / 3 and uB
int launch_mention_reduce2(const float* w, const float* v1, const float* v2, const float* uA, const float* uB,
                           float* outA, float* outB, int B, int N, int D, float scale, hipStream_t st);
// two independent launch_mention_reduce2 jobs (a, b) over the same B x N x D geometry in one launch; same bits
int launch_mention_reduce2_pair(const float* wa, const float* va1, const float* va2, const float* uaA, const float* uaB, float* outaA,
                                float* outaB, float scale_a, const float* wb, const float* vb1, const float* vb2, const float* ubA,
                                const float* ubB, float* outbA, float* outbB, float scale_b, int B, int N, int D, hipStream_t st);
// out[p,:] = scale (w1[p] m1[b,:] + w2[p] m2[b,:])       (m2 optional)
int launch_entity_combine(const float* w1, const float* m1, const float* w2, const float* m2, float* out, int B, int N,
                          int D, float scale, hipStream_t st);
// entity side of the aggregation backward + edge gradients (see kernel comment); mask = edge_enabled[4]
int launch_entity_side_bwd(const float* dA_mt, const float* dA_mi, const float* dA_et, const float* dA_ei,
                           const float* mt, const float* mi, const float* et, const float* ei, const float* e,
                           const float* de_extra, float* d_et, float* d_ei, float* de, int B, int N, int D,
                           const float* mask, bool accumulate, hipStream_t st);  // accumulate: d_et, d_ei += ...

// ---- input gradients (input_grad_kernels.hip): backward of the parameter-free input stages -----------------
// out[b, t, :] = g[b, :] / (e - s) on the (clipped) span s <= t < e, 0 elsewhere (ghmfc.py:54-60)
int launch_span_mean_bwd(const float* g, const int64_t* start, const int64_t* end, float* out, int B, int L, int D,
                         hipStream_t st);
// out[g, s, c] = in[g, c] / inner (torch.mean(dim=-2) backward)
int launch_axis_mean_bwd(const float* in, float* out, int64_t groups, int inner, int cols, hipStream_t st);
// token-block gradient of the entity pooling + token-0 read (ghmfc.py:245-249, model.py:73-75); out fp32 or bf16
int launch_token_block_bwd(const float* g_pool, const float* g_cls, const int64_t* mask, void* out, int64_t pairs, int T,
                           int D, bool bf16, hipStream_t st);
// out[r] = sum_c in[r, c]
int launch_row_sum(const float* in, float* out, int64_t rows, int C, hipStream_t st);
// backward of launch_miei w.r.t. its four inputs; scratch: miei_bwd_scratch_floats
size_t miei_bwd_scratch_floats(int64_t pairs, int B, int Km, int Ke);
int launch_miei_bwd(const float* mobj, const float* mscore, const float* eobj, const float* escore, const float* g,
                    float* d_mobj, float* d_mscore, float* d_eobj, float* d_escore, float* scratch, int B, int N, int Km,
                    int Ke, int R, float cos_eps, float miei_eps, hipStream_t st);

// ---- the mention representation head (mention_rows.hip) ----------------------------------------------
// the drin_mention_head of the *_head entry points (api.hip): its checks (NULL: the linear encoder, DRIN_OK), whether it replaces
// the mention-text Linear, and where the two rows' max positions sit in head->max_index (NULL, NULL without a max)
int validate_head(const drin_mention_head* h, const char* who);
bool rows_head(const drin_mention_head* h);
void head_positions(const drin_config* c, const drin_mention_head* h, int32_t** edge, int32_t** vertex);
// edge_row[b] = repr(raw[b]), vertex_row[b] = repr(enc[b]) (enc NULL: the edge row's values); repr: drin_mention_repr.
// raw fp32 or bf16 [B, L, D], enc fp32; start / end read by the span mean only, idx_edge / idx_vertex [B, D] written by the max only
int launch_mention_rows(const void* raw, bool raw_bf16, const float* enc, const int64_t* start, const int64_t* end, int repr,
                        float* edge_row, float* vertex_row, int* idx_edge, int* idx_vertex, int B, int L, int D, hipStream_t st);
// d_raw / d_enc [B, L, D], each WRITTEN whole or NULL: d_raw takes the edge row's term (and the vertex row's without an encoded
// block), d_enc the vertex row's; g_edge / g_vertex [B, D] or NULL (no gradient through that row)
int launch_mention_rows_bwd(const float* g_edge, const float* g_vertex, const int64_t* start, const int64_t* end, const int* idx_edge,
                            const int* idx_vertex, int repr, bool has_encoded, float* d_raw, float* d_enc, int B, int L, int D,
                            hipStream_t st);

// ---- vector-edge ablation (vector_kernels.hip) --------------------------------------------------
int launch_expand_edges(const float* es, float* out, int64_t pairs4, int D, hipStream_t st);
int launch_mention_reduce_vec(const float* w1, const float* v1, const float* w2, const float* v2, const float* u,
                              float* out, int B, int N, int D, float scale, bool mean_style, hipStream_t st);
int launch_entity_aggregate_vec(const float* e1, const float* m1, const float* e2, const float* m2, const float* v,
                                float* out, int B, int N, int D, hipStream_t st);
int launch_edge_pre_vec(const float* fu, const float* fv, const float* e, float* pre, int B, int N, int D,
                        hipStream_t st);
int launch_sigmoid_inplace(float* x, int64_t n, hipStream_t st, int act = DRIN_ACT_SIGMOID, float* z_out = nullptr);
int launch_edge_pre_vec_bwd(const float* dpre, float* dfu, float* dfv, int B, int N, int D, hipStream_t st);
int launch_entity_side_bwd_vec(const float* dA_mt, const float* dA_mi, const float* dA_et, const float* dA_ei,
                               const float* mt, const float* mi, const float* et, const float* ei, const float* e,
                               const float* de_extra, float* d_et, float* d_ei, float* de, int B, int N, int D,
                               const float* mask, hipStream_t st);


// ---- workspace self-checks (drin_host_selftest) ----------------------------------------------------------------------
// The layouts that live beside their kernels state their regions (arena.h: Region) with the floats the kernels index; all must
// start on a 256-byte boundary, be disjoint and end inside the layout's total.  DRIN_E_WORKSPACE with the region named otherwise.
inline int regions_hold(const char* layout, const Region* r, int n, size_t total) {
  const char* bad = first_bad_region(r, n, total);
  if (bad == nullptr) return DRIN_OK;
  set_error("selftest: %s: region %s is misaligned, overlaps another one or ends past the total of %zu floats", layout, bad, total);
  return DRIN_E_WORKSPACE;
}
int fused_layout_selfcheck(const drin_config& c);    // FusedLayout, Prepared (fused_forward.hip)
int cached_layout_selfcheck(const drin_config& c);   // CachedLayout (entity_cache.hip)
int melhi_layout_selfcheck(int B, int N, int D, int R, int L);           // MelhiLayout (melhi_kernels.hip)
int ghmfc_layout_selfcheck(int B, int N, int D, int R, int L, int P, int T);   // GhmfcLayout (ghmfc_forward.hip)
// the same layout as drin_ghmfc_forward_table carves it (rows: scored from per-entity rows, no entity regions), and the chunk
// buffer of drin_ghmfc_entity_rows for E entities
int ghmfc_table_layout_selfcheck(int B, int N, int D, int R, int L, int P, int T, bool rows, int64_t E);
// TopkLayout (topk_layout.h; both are thin calls of its topk_layout_fault): the workspace of drin_table_topk - the single-table
// form - and the rules of its kp, chunk and slice count (row_dtype DRIN_FEAT_BF16 with the product's precision: the planes / widen
// region of section 34 as well)
int table_topk_layout_selfcheck(int B, int64_t E, int D, int k, int64_t chunk_entities, int row_dtype = DRIN_FEAT_F32,
                                int precision = DRIN_PREC_F32);
// ... and of drin_table_topk_sum - the summed form - for S live terms of the given widths
int table_topk_sum_layout_selfcheck(const int* widths, int S, int B, int64_t E, int k, int64_t chunk_entities, const int* dtypes = nullptr,
                                    int precision = DRIN_PREC_F32);

}  // namespace drin
