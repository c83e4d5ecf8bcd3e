// C ABI of libdrin_hip.so (include/drin_hip.h): argument validation, workspace layout and the launch
// sequence of Model.forward (drin/model.py:164-209).  Host code only; kernels live in the sibling files.
#include <dlfcn.h>
#include <stdarg.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <stdio.h>
#include <string.h>

#include "fused.h"
#include "gemm_probe_check.h"
#include "internal.h"
#include "layout.h"
#include "wgrad_probe_check.h"

namespace drin {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
  set_error("%s: %s", what, hipGetErrorString(e));
  return DRIN_E_HIP;
}

// ---- the device of a call (internal.h: DeviceScope) -----------------------------------------------
static thread_local int g_call_device = -1;
static thread_local drin_gemm_route g_gemm_route = {};
drin_gemm_route& gemm_route() { return g_gemm_route; }
static thread_local WgradTrace g_wgrad_trace = {};
WgradTrace& wgrad_trace() { return g_wgrad_trace; }

int call_device() {
  if (g_call_device >= 0) return g_call_device;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  return dev;
}

DeviceScope::DeviceScope(void* stream, const void* device_pointer, const char* entry_point)
    : status(DRIN_OK), prev(-1), dev(-1), outer(g_call_device), switched(false) {
  hipError_t e = hipGetDevice(&prev);
  if (e != hipSuccess) {
    // no usable device on this host: nothing to bind; argument validation still answers, and a launch would report the HIP error
    (void)hipGetLastError();
    prev = -1;
    return;
  }
  dev = prev;
  if (stream != nullptr) {
    hipDevice_t d = 0;
    e = hipStreamGetDevice((hipStream_t)stream, &d);
    if (e != hipSuccess) {
      set_error("%s: hipStreamGetDevice: %s (is `stream` a hipStream_t?)", entry_point, hipGetErrorString(e));
      status = DRIN_E_HIP;
      return;
    }
    dev = (int)d;
  } else if (device_pointer != nullptr) {
    // the NULL stream is "the default stream of the current device": take the device that owns the call's memory instead, so
    // that a NULL-stream call on another device's tensors runs on that device's default stream
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, device_pointer) == hipSuccess && attr.type == hipMemoryTypeDevice)
      dev = attr.device;
    else
      (void)hipGetLastError();   // an unregistered pointer: keep the current device (validation will say what is wrong)
  }
  if (dev != prev) {
    e = hipSetDevice(dev);
    if (e != hipSuccess) {
      set_error("%s: hipSetDevice(%d): %s", entry_point, dev, hipGetErrorString(e));
      status = DRIN_E_HIP;
      return;
    }
    switched = true;
  }
  g_call_device = dev;
}

DeviceScope::~DeviceScope() {
  if (status != DRIN_OK || prev < 0) return;
  g_call_device = outer;
  if (switched) (void)hipSetDevice(prev);
}

// ---- the library's side stream of a device (internal.h: SideLane) --------------------------------
static SideLane g_side_lanes[64];
static std::mutex g_side_lanes_mutex;

int side_lane(SideLane** out) {
  const int dev = call_device();
  if (dev < 0 || dev >= 64) {
    set_error("side stream: device %d outside the 64 the library keeps state for", dev);
    return DRIN_E_UNSUPPORTED;
  }
  SideLane& lane = g_side_lanes[dev];
  if (!lane.ready.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lock(g_side_lanes_mutex);
    if (!lane.ready.load(std::memory_order_relaxed)) {
      hipError_t e = hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&lane.fork, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&lane.join, hipEventDisableTiming);
      if (e != hipSuccess) return hip_fail(e, "side stream of the device");
      lane.ready.store(true, std::memory_order_release);
    }
  }
  *out = &lane;
  return DRIN_OK;
}

// ---- roctx ranges (opt-in: DRIN_ROCTX) ----------------------------------------------------------
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (!getenv("DRIN_ROCTX")) return;
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
static const Roctx& roctx() {
  static const Roctx r;  // thread-safe one-time initialisation
  return r;
}
RoctxRange::RoctxRange(const char* name) : pushed(false) {
  const Roctx& r = roctx();
  if (r.push) {
    r.push(name);
    pushed = true;
  }
}
RoctxRange::~RoctxRange() {
  if (pushed) roctx().pop();
}

// ---- process-wide kernel profile ---------------------------------------------------------------
// One profile at a time per process; launches from ANY thread are attributed while it is open (autograd
// runs drin_backward on its own thread).  Slots are claimed with an atomic counter; begin / end are
// serialised by a mutex and must not race with launches they are meant to bracket.
struct Profile {
  std::atomic<bool> open{false};
  int capacity = 0;
  std::atomic<int> used{0};
  hipEvent_t* start = nullptr;
  hipEvent_t* stop = nullptr;
  int* cls = nullptr;
};
static Profile g_prof;
static std::mutex g_prof_mutex;

KernelTimer::KernelTimer(int kernel_class, hipStream_t st) : slot(-1), stream(st) {
  Profile& p = g_prof;
  if (!p.open.load(std::memory_order_acquire)) return;
  const int s = p.used.fetch_add(1, std::memory_order_relaxed);
  if (s >= p.capacity) return;
  slot = s;
  p.cls[slot] = kernel_class;
  (void)hipEventRecord(p.start[slot], st);
}

KernelTimer::~KernelTimer() {
  if (slot >= 0) (void)hipEventRecord(g_prof.stop[slot], stream);
}

static void profile_free(Profile& p) {
  for (int i = 0; i < p.capacity; ++i) {
    if (p.start) (void)hipEventDestroy(p.start[i]);
    if (p.stop) (void)hipEventDestroy(p.stop[i]);
  }
  delete[] p.start;
  delete[] p.stop;
  delete[] p.cls;
  p.start = p.stop = nullptr;
  p.cls = nullptr;
  p.capacity = 0;
  p.used.store(0);
  p.open.store(false);
}

int vertex_act(const drin_config* c) { return c->vertex_activation == DRIN_ACT_DEFAULT ? DRIN_ACT_GELU : c->vertex_activation; }
int edge_act(const drin_config* c) { return c->edge_activation == DRIN_ACT_DEFAULT ? DRIN_ACT_SIGMOID : c->edge_activation; }

int validate_config(const drin_config* c) {
  if (!c) {
    set_error("config is NULL");
    return DRIN_E_NULL;
  }
  if (c->batch < 0 || c->num_candidates <= 0 || c->embed_dim <= 0 || c->image_dim <= 0 || c->mention_tokens <= 0 ||
      c->image_regions <= 0 || c->mention_objects < 0 || c->entity_objects < 0 || c->entity_tokens < 0 ||
      c->mention_object_inner < 0 || c->entity_image_inner < 0 || c->entity_object_inner < 0) {
    set_error("config: negative or zero dimension");
    return DRIN_E_SHAPE;
  }
  if (c->embed_dim % 4 || c->image_dim % 4) {
    set_error("config: embed_dim=%d and image_dim=%d must be multiples of 4 (16-byte lane accesses)", c->embed_dim,
              c->image_dim);
    return DRIN_E_SHAPE;
  }
  if (c->embed_dim > 1024) {
    set_error("config: embed_dim=%d > 1024 is not built (LayerNorm row kept in registers)", c->embed_dim);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->vector_edges && (c->embed_dim % 8)) {
    set_error("config: vector edges need embed_dim %% 8 == 0 (got %d)", c->embed_dim);
    return DRIN_E_SHAPE;
  }
  if (c->num_layers < 0 || c->num_layers > DRIN_MAX_LAYERS) {
    set_error("config: num_layers=%d outside [0, %d]", c->num_layers, DRIN_MAX_LAYERS);
    return DRIN_E_SHAPE;
  }
  if ((int64_t)c->batch * c->num_candidates > (int64_t)1 << 30) {
    set_error("config: batch * num_candidates too large for one call; split the batch");
    return DRIN_E_SHAPE;
  }
  if (c->feature_dtype != DRIN_FEAT_F32 && c->feature_dtype != DRIN_FEAT_BF16) {
    set_error("config: feature_dtype %d is not DRIN_FEAT_F32 / DRIN_FEAT_BF16", c->feature_dtype);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->vertex_activation < DRIN_ACT_DEFAULT || c->vertex_activation > DRIN_ACT_SILU) {
    set_error("config: vertex_activation %d is not a drin_activation", c->vertex_activation);
    return DRIN_E_UNSUPPORTED;
  }
  // (sigmoid, tanh, relu: the backward takes the derivative from the stored edge; gelu, silu: the forward keeps the
  //  pre-activation for it, Layout::edge_z)
  if (c->edge_activation < DRIN_ACT_DEFAULT || c->edge_activation > DRIN_ACT_SILU) {
    set_error("config: edge_activation %d is not a drin_activation", c->edge_activation);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->cache_format != DRIN_CACHE_F32 && c->cache_format != DRIN_CACHE_MIXED_F16) {
    set_error("config: cache_format %d is not a drin_cache_format", c->cache_format);
    return DRIN_E_UNSUPPORTED;
  }
  if (c->precision != DRIN_PREC_F32 && c->precision != DRIN_PREC_BF16X3 && c->precision != DRIN_PREC_BF16X3_ALL &&
      c->precision != DRIN_PREC_BF16X3_IF16) {
    set_error("config: precision %d is not a drin_precision", c->precision);
    return DRIN_E_UNSUPPORTED;
  }
  return DRIN_OK;
}

static int validate_batch(const drin_config* c, const drin_batch* b) {
  if (!b) {
    set_error("batch is NULL");
    return DRIN_E_NULL;
  }
  if (c->feature_dtype != DRIN_FEAT_F32) {
    set_error("bf16 feature storage is read by drin_forward_prepared only; widen the features to fp32 for this entry point");
    return DRIN_E_UNSUPPORTED;
  }
  if (c->precision == DRIN_PREC_BF16X3_IF16) {
    set_error("DRIN_PREC_BF16X3_IF16 (the entity-image contraction in one fp16 pass) is an inference mode of drin_forward_prepared; use DRIN_PREC_BF16X3 here");
    return DRIN_E_UNSUPPORTED;
  }
  const void* req[] = {b->mention_text,  b->mention_start,        b->mention_end,     b->mention_image,
                       b->mention_object, b->mention_object_score, b->entity_text,     b->entity_image,
                       b->entity_object,  b->entity_object_score,  b->miet_similarity, b->mtei_similarity};
  const char* names[] = {"mention_text",   "mention_start",        "mention_end",     "mention_image",
                         "mention_object", "mention_object_score", "entity_text",     "entity_image",
                         "entity_object",  "entity_object_score",  "miet_similarity", "mtei_similarity"};
  for (int i = 0; i < 12; ++i) {
    if (!req[i]) {
      set_error("batch.%s is NULL", names[i]);
      return DRIN_E_NULL;
    }
  }
  if (c->entity_tokens > 0 && !b->entity_text_mask) {
    set_error("batch.entity_text_mask is NULL but entity_tokens=%d", c->entity_tokens);
    return DRIN_E_NULL;
  }
  if (b->entity_text_cls && c->entity_tokens > 0) {
    set_error("batch.entity_text_cls goes with pooled entity text (entity_tokens = 0), not with a token block");
    return DRIN_E_UNSUPPORTED;
  }
  const void* al[] = {b->mention_text, b->mention_image, b->mention_object, b->entity_text, b->entity_image,
                      b->entity_object, b->entity_text_cls};
  for (const void* p : al)
    if (!aligned16(p)) {
      set_error("batch: feature tensors must be 16-byte aligned");
      return DRIN_E_ALIGN;
    }
  return DRIN_OK;
}

// rows_head: the mention-text Linear is not part of the model (DRIN_MENTION_ROWS): its two tensors are never read, may be NULL
static int validate_params(const drin_config* c, const drin_params* p, bool rows_head = false) {
  if (!p) {
    set_error("params is NULL");
    return DRIN_E_NULL;
  }
  const void* req[] = {p->w_mention_text,  p->b_mention_text,  p->w_entity_text,  p->b_entity_text,
                       p->w_mention_image, p->b_mention_image, p->w_entity_image, p->b_entity_image};
  for (int i = rows_head ? 2 : 0; i < 8; ++i) {   // by position: the first two are the mention-text Linear
    const void* q = req[i];
    if (!q || !aligned16(q)) {
      set_error("params: vertex encoder tensor NULL or not 16-byte aligned");
      return q ? DRIN_E_ALIGN : DRIN_E_NULL;
    }
  }
  for (int l = 0; l < c->num_layers; ++l) {
    const drin_layer_params& L = p->layer[l];
    const void* lr[] = {L.w_h, L.b_h, L.w_u, L.b_u, L.w_v, L.b_v, L.ln_weight, L.ln_bias};
    for (const void* q : lr)
      if (!q || !aligned16(q)) {
        set_error("params: layer %d tensor NULL or not 16-byte aligned", l);
        return q ? DRIN_E_ALIGN : DRIN_E_NULL;
      }
    if (c->vector_edges && (!L.w_m || !L.b_m || !aligned16(L.w_m) || !aligned16(L.b_m))) {
      set_error("params: layer %d w_m / b_m (vector edges, model.py:112) NULL or not 16-byte aligned", l);
      return DRIN_E_NULL;
    }
  }
  return DRIN_OK;
}

// The mention head of the *_head entry points (drin_hip.h: drin_mention_head).  NULL: the linear encoder.
bool rows_head(const drin_mention_head* h) { return h != nullptr && h->encoder == DRIN_MENTION_ROWS; }
int validate_head(const drin_mention_head* h, const char* who) {
  if (!h) return DRIN_OK;
  if (h->struct_size != sizeof(drin_mention_head)) {
    set_error("%s: head.struct_size = %zu, this library's drin_mention_head has %zu bytes", who, h->struct_size, sizeof(drin_mention_head));
    return DRIN_E_SHAPE;
  }
  if ((h->encoder != DRIN_MENTION_LINEAR && h->encoder != DRIN_MENTION_ROWS) ||
      (h->representation != DRIN_REPR_AVG_EXTRACT && h->representation != DRIN_REPR_MAX_POOL)) {
    set_error("%s: head.encoder = %d / head.representation = %d: not a drin_mention_encoder / drin_mention_repr", who, h->encoder,
              h->representation);
    return DRIN_E_SHAPE;
  }
  if (h->encoder == DRIN_MENTION_LINEAR) {
    if (h->representation == DRIN_REPR_MAX_POOL) {
      set_error("%s: {DRIN_MENTION_LINEAR, DRIN_REPR_MAX_POOL} is not built: common/args.py:12-13 forces avg extract for \"linear\" "
                "(the reference's DRIN code would take the text-text edge by max there; DESIGN.md section 22)", who);
      return DRIN_E_UNSUPPORTED;
    }
    if (h->encoded || h->grad_encoded) {
      set_error("%s: head.encoded / head.grad_encoded go with DRIN_MENTION_ROWS only", who);
      return DRIN_E_SHAPE;
    }
    return DRIN_OK;
  }
  if (h->grad_encoded && !h->encoded) {
    set_error("%s: head.grad_encoded without head.encoded (both rows are then functions of mention_text: ask for its gradient)", who);
    return DRIN_E_SHAPE;
  }
  if (h->representation == DRIN_REPR_MAX_POOL && !h->max_index) {
    set_error("%s: head.max_index is NULL (DRIN_REPR_MAX_POOL keeps the positions of the maxima there)", who);
    return DRIN_E_NULL;
  }
  if (!aligned16(h->encoded) || !aligned16(h->max_index) || !aligned16(h->grad_encoded)) {
    set_error("%s: head.encoded / max_index / grad_encoded must be 16-byte aligned", who);
    return DRIN_E_ALIGN;
  }
  return DRIN_OK;
}
// the positions of the edge row's and the vertex row's maxima in head.max_index [2][B, D] (NULL, NULL without a max)
void head_positions(const drin_config* c, const drin_mention_head* h, int32_t** edge, int32_t** vertex) {
  const bool mx = h->representation == DRIN_REPR_MAX_POOL;
  *edge = mx ? h->max_index : nullptr;
  *vertex = mx ? h->max_index + (size_t)c->batch * c->embed_dim : nullptr;
}

// Operand pointers of the static edges without a workspace, hence without pooled copies (inner dims <= 1): the caller's
// tensors and span-mean scratch.
static Pooled unpooled(const drin_config* c, const drin_batch* b, const float* span_mean) {
  Pooled p;
  p.span_mean = span_mean;
  p.mention_object = b->mention_object;
  p.entity_object = b->entity_object;
  p.entity_image = b->entity_image;
  p.entity_text = b->entity_text;
  // the raw CLS / pooler row of a pair: token 0 of its block (model.py:73-75), or the pooled row as delivered
  p.entity_text_raw_stride = c->entity_tokens > 0 ? (int64_t)c->entity_tokens * c->embed_dim : c->embed_dim;
  return p;
}

// Operand pointers of the vertex / edge encoders: pooled copies in the workspace where the reference
// averages an axis, the caller's tensors where it does not.
void resolve_pooled(const drin_config* c, const drin_batch* b, const Layout& L, float* ws, Pooled* out) {
  *out = unpooled(c, b, ws + L.span_mean);
  out->mention_image = ws + L.mimg_pool;
  if (c->mention_object_inner > 1) out->mention_object = ws + L.mobj_pool;
  if (c->entity_object_inner > 1) out->entity_object = ws + L.eobj_pool;
  if (c->entity_image_inner > 1) out->entity_image = ws + L.eimg_pool;
  if (c->entity_tokens > 0) out->entity_text = ws + L.xet_pool;
}

// Resolves the pooled / raw operand pointers of the vertex and edge encoders and runs the pooling: a pass for every operand
// that resolve_pooled pointed into the workspace.
// (head, DRIN_MENTION_ROWS: the span mean's place takes the edge row repr(mention_text) and the layer-0 mention-text vertex
//  takes repr(encoded) - k_mention_rows, one launch - instead of the span mean that the mention-text Linear would read)
int run_pooling(const drin_config* c, const drin_batch* b, const Layout& L, float* ws, Pooled* out, hipStream_t st,
                const drin_mention_head* head) {
  const int B = c->batch, N = c->num_candidates, D = c->embed_dim, R = c->image_dim;
  const int64_t M = (int64_t)B * N;
  resolve_pooled(c, b, L, ws, out);
  auto copy_of = [](const float* resolved, const float* raw) { return resolved != raw ? const_cast<float*>(resolved) : nullptr; };
  if (rows_head(head)) {
    int32_t *ie, *iv;
    head_positions(c, head, &ie, &iv);
    DRIN_TRY(launch_mention_rows(b->mention_text, false, head->encoded, b->mention_start, b->mention_end, head->representation,
                                 ws + L.span_mean, ws + L.vm[0], ie, iv, B, c->mention_tokens, D, st));
  } else {
    DRIN_TRY(launch_span_mean(b->mention_text, b->mention_start, b->mention_end, ws + L.span_mean, B, c->mention_tokens, D, st));
  }
  DRIN_TRY(launch_axis_mean(b->mention_image, ws + L.mimg_pool, B, c->image_regions, R, st));
  if (float* dst = copy_of(out->mention_object, b->mention_object))
    DRIN_TRY(launch_axis_mean(b->mention_object, dst, (int64_t)B * c->mention_objects, c->mention_object_inner, R, st));
  if (float* dst = copy_of(out->entity_object, b->entity_object))
    DRIN_TRY(launch_axis_mean(b->entity_object, dst, M * c->entity_objects, c->entity_object_inner, R, st));
  if (float* dst = copy_of(out->entity_image, b->entity_image))
    DRIN_TRY(launch_axis_mean(b->entity_image, dst, M, c->entity_image_inner, R, st));
  if (float* dst = copy_of(out->entity_text, b->entity_text))
    DRIN_TRY(launch_entity_token_mean(b->entity_text, b->entity_text_mask, dst, M, c->entity_tokens, D, st));
  return DRIN_OK;
}

int run_static_edges(const drin_config* c, const drin_batch* b, const Pooled& P, float* edges, hipStream_t st) {
  const int B = c->batch, N = c->num_candidates;
  const int64_t M = (int64_t)B * N;
  // tt (model.py:71-76), ti = mtei / 100, it = miet / 100 (model.py:203), ii (model.py:78-92)
  // (entity_text_cls: the raw rows of a batch whose token means were pooled ahead of time)
  const float* raw = b->entity_text_cls ? b->entity_text_cls : b->entity_text;
  const int64_t raw_stride = b->entity_text_cls ? (int64_t)c->embed_dim : P.entity_text_raw_stride;
  // (the two CLIP edges are two loads and two divisions per pair: they ride in the cosine launch)
  DRIN_TRY(launch_cosine_rows(P.span_mean, raw, raw_stride, edges + 0 * M, B, N, c->embed_dim, c->cosine_eps, 1.0f, st,
                              b->entity_index, b->mtei_similarity, b->miet_similarity, edges + 1 * M, edges + 2 * M,
                              c->clip_scale));
  DRIN_TRY(launch_miei(P.mention_object, b->mention_object_score, P.entity_object, b->entity_object_score,
                       edges + 3 * M, B, N, c->mention_objects, c->entity_objects, c->image_dim, c->cosine_eps,
                       c->miei_eps, 1.0f, st, b->entity_index));
  return DRIN_OK;
}

static int copy_out(float* dst, const float* src, size_t n, hipStream_t st) {
  if (!dst) return DRIN_OK;
  hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(trace)");
  return DRIN_OK;
}

static int tap(const drin_trace* t, int l, const Layout& L, const float* ws, int B, int64_t M, int D, hipStream_t st,
               size_t edge_width = 1) {
  if (!t) return DRIN_OK;
  DRIN_TRY(copy_out(t->mention_text_vertex[l], ws + L.vm[l], (size_t)B * D, st));
  DRIN_TRY(copy_out(t->mention_image_vertex[l], ws + L.vm[l] + (size_t)B * D, (size_t)B * D, st));
  DRIN_TRY(copy_out(t->entity_text_vertex[l], ws + L.ve[l], (size_t)M * D, st));
  DRIN_TRY(copy_out(t->entity_image_vertex[l], ws + L.ve[l] + (size_t)M * D, (size_t)M * D, st));
  DRIN_TRY(copy_out(t->edges[l], ws + L.edges[l], (size_t)4 * M * edge_width, st));
  return DRIN_OK;
}

// Table form of the layer-by-layer entry points (training over device-resident entity tables): the entity tensors of the
// batch are TABLES of cfg.num_entities rows and pair p reads row entity_index[p] - inside the static-edge kernels and in
// the row addressing of the vertex-encoder GEMMs (forward x W^T, backward dY^T x), never as gathered copies.
static int indexed_supported(const drin_config* c, const char* who) {
  const int64_t M = (int64_t)c->batch * c->num_candidates;
  const int D = c->embed_dim, R = c->image_dim;
  const bool x3 = c->precision == DRIN_PREC_BF16X3 || c->precision == DRIN_PREC_BF16X3_ALL;
  if (c->num_entities <= 0 || c->entity_tokens != 0 || c->entity_image_inner > 1 || c->entity_object_inner > 1 ||
      c->entity_objects != 1 || c->vector_edges || !x3 || M < 1024 || (D % 32) || (R % 32) || D < 128 || R < 128 ||
      R > 2048 || c->batch > kMaxGridY) {
    set_error("%s: entity_index needs pooled entity text tables (entity_tokens = 0, num_entities > 0), one object per entity, "
              "inner dims <= 1, scalar edges, split-bf16 precision, D and R multiples of 32 (>= 128, R <= 2048) and at least "
              "1024 pairs; gather on the caller side otherwise", who);
    return DRIN_E_UNSUPPORTED;
  }
  return DRIN_OK;
}

// ---- input gradients (drin_backward_ex) -----------------------------------------------------------------------------
// Scratch of drin_input_grads (floats, every region on a 256-byte boundary).  Sized from the config alone.
struct InputGradScratch {
  size_t total_floats = 0;
  size_t g_span = 0, g_raw = 0, cls_stage = 0, g_pool = 0, cos3 = 0, g_mimg = 0, g_eimg = 0, g_mobj = 0, g_eobj = 0;
  size_t g_ms = 0, g_es = 0, g_edge = 0, planes_ei = 0, planes_et = 0, miei = 0;
  void build(const drin_config& c) {
    const size_t B = (size_t)c.batch, N = (size_t)c.num_candidates, D = (size_t)c.embed_dim, R = (size_t)c.image_dim;
    const size_t M = B * N, Km = (size_t)c.mention_objects, Ke = (size_t)c.entity_objects;
    const bool x3 = c.precision == DRIN_PREC_BF16X3 || c.precision == DRIN_PREC_BF16X3_ALL;
    Arena A;
    g_span = A.take(B * D);
    g_raw = A.take(M * D);                                     // text-text edge: gradient of the entity rows it reads
    cls_stage = A.take(c.entity_tokens > 0 ? M * D : 0);       // token 0 of every token block, contiguous
    g_pool = A.take(c.entity_tokens > 0 ? M * D : 0);
    cos3 = A.take(3 * M);
    g_mimg = A.take(B * R);
    g_eimg = A.take(c.entity_image_inner > 1 ? M * R : 0);
    g_mobj = A.take(B * Km * R);
    g_eobj = A.take(M * Ke * R);
    g_ms = A.take(B * Km);
    g_es = A.take(M * Ke);
    g_edge = A.take(4 * M);
    planes_ei = A.take(x3 ? D * R : 0);                        // bf16 (hi, lo) planes of W_ei^T [R][D]
    planes_et = A.take(x3 ? D * D : 0);
    miei = A.take(miei_bwd_scratch_floats((int64_t)M, (int)B, (int)Km, (int)Ke));
    total_floats = A.total;
  }
};

static int input_grad_scratch_selfcheck(const drin_config& c) {
  const size_t B = c.batch, M = B * c.num_candidates, D = c.embed_dim, R = c.image_dim, Km = c.mention_objects, Ke = c.entity_objects;
  const size_t x3 = split_bf16(c.precision), tok = c.entity_tokens > 0;
  InputGradScratch S;
  S.build(c);
  const Region sc[] = {
      {"g_span", S.g_span, B * D}, {"g_raw", S.g_raw, M * D}, {"cls_stage", S.cls_stage, tok * M * D}, {"g_pool", S.g_pool, tok * M * D},
      {"cos3", S.cos3, 3 * M}, {"g_mimg", S.g_mimg, B * R}, {"g_eimg", S.g_eimg, c.entity_image_inner > 1 ? M * R : 0},
      {"g_mobj", S.g_mobj, B * Km * R}, {"g_eobj", S.g_eobj, M * Ke * R}, {"g_ms", S.g_ms, B * Km}, {"g_es", S.g_es, M * Ke},
      {"g_edge", S.g_edge, 4 * M}, {"planes_ei", S.planes_ei, x3 * D * R}, {"planes_et", S.planes_et, x3 * D * D},
      {"miei", S.miei, miei_bwd_scratch_floats((int64_t)M, (int)B, (int)Km, (int)Ke)}};
  return regions_hold("InputGradScratch", sc, (int)(sizeof(sc) / sizeof(sc[0])), S.total_floats);
}

static int validate_input_grads(const drin_config* c, const drin_batch* b, const drin_input_grads* g) {
  if (b->entity_index) {
    set_error("drin_backward_ex: input gradients of a table-form batch (entity_index) are not built; gather the rows");
    return DRIN_E_UNSUPPORTED;
  }
  if (g->entity_text_cls && !b->entity_text_cls) {
    set_error("drin_backward_ex: input_grads.entity_text_cls needs batch.entity_text_cls (the pooled-ahead form)");
    return DRIN_E_NULL;
  }
  if (c->mention_objects * c->entity_objects > 64) {
    set_error("drin_backward_ex: more than 64 object pairs (mention_objects x entity_objects) is not built");
    return DRIN_E_UNSUPPORTED;
  }
  const void* outs[] = {g->mention_text, g->mention_image, g->mention_object, g->mention_object_score, g->entity_text,
                        g->entity_text_cls, g->entity_image, g->entity_object, g->entity_object_score, g->miet_similarity,
                        g->mtei_similarity};
  for (const void* o : outs)
    if (!aligned16(o)) {
      set_error("drin_backward_ex: input gradient outputs must be 16-byte aligned");
      return DRIN_E_ALIGN;
    }
  InputGradScratch S;
  S.build(*c);
  if (!g->scratch || !aligned16(g->scratch) || g->scratch_bytes < S.total_floats * sizeof(float)) {
    set_error("drin_backward_ex: input_grads.scratch is NULL, unaligned or smaller than drin_input_grad_scratch_bytes (%zu)",
              S.total_floats * sizeof(float));
    return g->scratch ? DRIN_E_WORKSPACE : DRIN_E_NULL;
  }
  return DRIN_OK;
}

static int zero_out(void* p, size_t floats, hipStream_t st) {
  if (!p) return DRIN_OK;
  hipError_t e = hipMemsetAsync(p, 0, floats * sizeof(float), st);
  return e == hipSuccess ? DRIN_OK : hip_fail(e, "hipMemsetAsync(input gradient)");
}

// ge: the layer-0 edge gradients [4][B N (x D with vector edges)] (w.r.t. the edges before the edge_enabled mask), NULL
// without GCN layers (the score then reads neither the edges nor the image vertices); g_vm0 = [d mt | d mi],
// g_ve0 = [d et | d ei]: the vertex encoders' output gradients.
static int run_input_grads(const drin_config* c, const drin_batch* b, const drin_params* W, const Pooled& P, const float* ge,
                           const float* g_vm0, const float* g_ve0, const drin_input_grads* ig, hipStream_t st,
                           const drin_mention_head* head = nullptr) {
  const int B = c->batch, N = c->num_candidates, D = c->embed_dim, R = c->image_dim, T = c->entity_tokens;
  const int Km = c->mention_objects, Ke = c->entity_objects;
  const size_t M = (size_t)B * N, BD = (size_t)B * D, MD = M * D;
  const int mobj_in = c->mention_object_inner > 1 ? c->mention_object_inner : 1;
  const int eimg_in = c->entity_image_inner > 1 ? c->entity_image_inner : 1;
  const int eobj_in = c->entity_object_inner > 1 ? c->entity_object_inner : 1;
  InputGradScratch S;
  S.build(*c);
  float* sc = (float*)ig->scratch;
  const bool live = ge != nullptr;   // edges and image vertices reach the score
  const float* g_mt = g_vm0;
  const float* g_mi = g_vm0 + BD;
  const float* g_et = g_ve0;
  const float* g_ei = g_ve0 + MD;
  // pair-sized dX = dY W (W [D][n_out]): launch_gemm_nn, against W^T planes written here when it takes split-bf16
  auto pair_dx = [&](const float* g, const float* w, float* planes, float* out, int n_out, bool acc) -> int {
    if (gemm_nn_takes_bf16x3(c->precision, (int64_t)M, n_out, D)) {
      SplitBatch tb;
      DRIN_TRY(tb.add(w, planes, (int64_t)D * n_out));
      DRIN_TRY(launch_transpose_split_batch(tb, D, n_out, st));
    }
    return launch_gemm_nn({{g, D}, {w, n_out}, out, n_out, (int64_t)M, n_out, D, acc}, c->precision, st, {}, {planes});
  };

  // the scalar layer-0 edges: vector edges are the scalar ones broadcast over D (model.py:202) - their row sums
  const float* gs = ge;
  if (live && c->vector_edges) {
    DRIN_TRY(launch_row_sum(ge, sc + S.g_edge, 4 * (int64_t)M, D, st));
    gs = sc + S.g_edge;
  }

  // text-text edge cos(span mean, raw entity rows) (model.py:71-76): d span mean and d raw rows
  const bool has_cls = b->entity_text_cls != nullptr;
  float* d_raw = sc + S.g_raw;
  if (T == 0 && !has_cls && ig->entity_text) d_raw = ig->entity_text;   // the raw rows ARE entity_text
  if (T == 0 && has_cls && ig->entity_text_cls) d_raw = ig->entity_text_cls;
  const bool want_raw = (T > 0 && ig->entity_text) || (T == 0 && !has_cls && ig->entity_text) || (has_cls && ig->entity_text_cls);
  const bool rows = rows_head(head);
  const bool tt = live && (ig->mention_text || want_raw);
  if (tt) {
    const float* y = has_cls ? b->entity_text_cls : b->entity_text;
    if (T > 0) {   // token 0 of each block (model.py:73-75), staged contiguous for the row kernel
      hipError_t e = hipMemcpy2DAsync(sc + S.cls_stage, (size_t)D * sizeof(float), b->entity_text, (size_t)T * D * sizeof(float),
                                      (size_t)D * sizeof(float), M, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return hip_fail(e, "hipMemcpy2DAsync(token 0 rows)");
      y = sc + S.cls_stage;
    }
    DRIN_TRY(launch_cosine_bwd(P.span_mean, y, gs, sc + S.g_span, d_raw, sc + S.cos3, B, N, D, c->cosine_eps, st));
  } else if (has_cls && ig->entity_text_cls) {
    DRIN_TRY(zero_out(ig->entity_text_cls, MD, st));
  }
  // mention text: d span = d mt W_mt (+ the edge term), then the span mean's backward (ghmfc.py:54-60)
  // (a rows head: no Linear - the edge row's gradient goes to the raw block, the vertex row's to the encoded block, or both to
  //  the raw block when there is no encoded one: k_mention_rows_bwd, every element written once)
  if (rows) {
    int32_t *ie, *iv;
    head_positions(c, head, &ie, &iv);
    DRIN_TRY(launch_mention_rows_bwd(tt ? sc + S.g_span : nullptr, g_mt, b->mention_start, b->mention_end, ie, iv, head->representation,
                                     head->encoded != nullptr, ig->mention_text, head->grad_encoded, B, c->mention_tokens, D, st));
  } else if (ig->mention_text) {
    DRIN_TRY(launch_gemm_nn({{g_mt, D}, {W->w_mention_text, D}, sc + S.g_span, D, B, D, D, tt}, DRIN_PREC_F32, st));
    DRIN_TRY(launch_span_mean_bwd(sc + S.g_span, b->mention_start, b->mention_end, ig->mention_text, B, c->mention_tokens, D, st));
  }
  // entity text: d x_et = d et W_et (+ the edge term when the raw rows are entity_text itself); token blocks: the pooling's
  // backward (ghmfc.py:245-249) with token 0 taking the edge term
  if (ig->entity_text) {
    float* dst = T > 0 ? sc + S.g_pool : ig->entity_text;
    DRIN_TRY(pair_dx(g_et, W->w_entity_text, sc + S.planes_et, dst, D, tt && T == 0 && !has_cls));
    if (T > 0)
      DRIN_TRY(launch_token_block_bwd(sc + S.g_pool, tt ? sc + S.g_raw : nullptr, b->entity_text_mask, ig->entity_text,
                                      (int64_t)M, T, D, false, st));
  }
  // images: d x = d v W (model.py:41-45), then the means' backward
  if (ig->mention_image) {
    if (live) {
      DRIN_TRY(launch_gemm_nn({{g_mi, D}, {W->w_mention_image, R}, sc + S.g_mimg, R, B, R, D}, DRIN_PREC_F32, st));
      DRIN_TRY(launch_axis_mean_bwd(sc + S.g_mimg, ig->mention_image, B, c->image_regions, R, st));
    } else {
      DRIN_TRY(zero_out(ig->mention_image, (size_t)B * c->image_regions * R, st));
    }
  }
  if (ig->entity_image) {
    if (live) {
      float* dst = eimg_in > 1 ? sc + S.g_eimg : ig->entity_image;
      DRIN_TRY(pair_dx(g_ei, W->w_entity_image, sc + S.planes_ei, dst, R, false));
      if (eimg_in > 1) DRIN_TRY(launch_axis_mean_bwd(dst, ig->entity_image, (int64_t)M, eimg_in, R, st));
    } else {
      DRIN_TRY(zero_out(ig->entity_image, M * eimg_in * R, st));
    }
  }
  // image-image edge (model.py:78-92)
  if (ig->mention_object || ig->mention_object_score || ig->entity_object || ig->entity_object_score) {
    if (live) {
      float* d_mobj = mobj_in > 1 || !ig->mention_object ? sc + S.g_mobj : ig->mention_object;
      float* d_eobj = eobj_in > 1 || !ig->entity_object ? sc + S.g_eobj : ig->entity_object;
      float* d_ms = ig->mention_object_score ? ig->mention_object_score : sc + S.g_ms;
      float* d_es = ig->entity_object_score ? ig->entity_object_score : sc + S.g_es;
      DRIN_TRY(launch_miei_bwd(P.mention_object, b->mention_object_score, P.entity_object, b->entity_object_score, gs + 3 * M,
                               d_mobj, d_ms, d_eobj, d_es, sc + S.miei, B, N, Km, Ke, R, c->cosine_eps, c->miei_eps, st));
      if (ig->mention_object && mobj_in > 1)
        DRIN_TRY(launch_axis_mean_bwd(d_mobj, ig->mention_object, (int64_t)B * Km, mobj_in, R, st));
      if (ig->entity_object && eobj_in > 1)
        DRIN_TRY(launch_axis_mean_bwd(d_eobj, ig->entity_object, (int64_t)M * Ke, eobj_in, R, st));
    } else {
      DRIN_TRY(zero_out(ig->mention_object, (size_t)B * Km * mobj_in * R, st));
      DRIN_TRY(zero_out(ig->entity_object, M * Ke * eobj_in * R, st));
      DRIN_TRY(zero_out(ig->mention_object_score, (size_t)B * Km, st));
      DRIN_TRY(zero_out(ig->entity_object_score, M * Ke, st));
    }
  }
  // CLIP edges ti = mtei / clip_scale, it = miet / clip_scale (model.py:203)
  if (ig->mtei_similarity) {
    if (live) DRIN_TRY(launch_scale_div(gs + M, ig->mtei_similarity, (int64_t)M, 1.0f, c->clip_scale, st));
    else DRIN_TRY(zero_out(ig->mtei_similarity, M, st));
  }
  if (ig->miet_similarity) {
    if (live) DRIN_TRY(launch_scale_div(gs + 2 * M, ig->miet_similarity, (int64_t)M, 1.0f, c->clip_scale, st));
    else DRIN_TRY(zero_out(ig->miet_similarity, M, st));
  }
  return DRIN_OK;
}

}  // namespace drin

using namespace drin;

extern "C" {

int drin_version(void) { return DRIN_ABI_VERSION; }

const char* drin_last_error(void) { return g_err; }

const char* drin_build_info(void) { return "gfx950 hipcc " __VERSION__ " " __DATE__; }

int drin_default_config(drin_config* cfg) {
  if (!cfg) {
    set_error("config is NULL");
    return DRIN_E_NULL;
  }
  memset(cfg, 0, sizeof(*cfg));
  cfg->batch = 0;
  cfg->num_candidates = 11;
  cfg->embed_dim = 768;
  cfg->image_dim = 2048;
  cfg->mention_tokens = 128;
  cfg->image_regions = 49;
  cfg->mention_objects = 3;
  cfg->entity_objects = 1;
  cfg->entity_tokens = 0;
  cfg->mention_object_inner = 1;
  cfg->entity_image_inner = 0;
  cfg->entity_object_inner = 0;
  cfg->num_layers = 2;
  cfg->dynamic_edges = 1;
  for (int k = 0; k < 4; ++k) cfg->edge_enabled[k] = 1.0f;
  cfg->layer_norm_eps = 1e-5f;
  cfg->cosine_eps = 1e-8f;
  cfg->miei_eps = 1e-9f;
  cfg->clip_scale = 100.0f;
  cfg->precision = DRIN_PREC_F32;
  return DRIN_OK;
}

size_t drin_workspace_bytes(const drin_config* cfg, int for_training) {
  if (validate_config(cfg) != DRIN_OK) return 0;
  Layout L;
  L.build(*cfg, for_training != 0);
  return L.total_floats * sizeof(float);
}

int drin_indexed_supported(const drin_config* cfg) {
  DRIN_TRY(validate_config(cfg));
  return indexed_supported(cfg, "drin_indexed_supported");
}

int drin_edges_fwd(const drin_config* cfg, const drin_batch* batch, float* edges, float* span_mean, void* stream) {
  DRIN_BIND_DEVICE(stream, edges, "drin_edges_fwd");
  DRIN_TRY(validate_config(cfg));
  DRIN_TRY(validate_batch(cfg, batch));
  if (!edges) {
    set_error("edges is NULL");
    return DRIN_E_NULL;
  }
  if (cfg->mention_object_inner > 1 || cfg->entity_object_inner > 1) {
    set_error("drin_edges_fwd: inner object dims > 1 need the pooled path of drin_forward");
    return DRIN_E_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const int B = cfg->batch, D = cfg->embed_dim;
  if (!span_mean) {
    set_error("drin_edges_fwd: span_mean scratch [B, D] is required");
    return DRIN_E_NULL;
  }
  DRIN_TRY(launch_span_mean(batch->mention_text, batch->mention_start, batch->mention_end, span_mean, B,
                            cfg->mention_tokens, D, st));
  return run_static_edges(cfg, batch, unpooled(cfg, batch, span_mean), edges, st);
}

int drin_pool_fwd(const drin_config* cfg, const drin_batch* batch, float* pooled_entity_text,
                  float* pooled_mention_image, float* pooled_entity_image, void* stream) {
  DRIN_BIND_DEVICE(stream, batch ? (const void*)batch->mention_image : nullptr, "drin_pool_fwd");
  DRIN_TRY(validate_config(cfg));
  if (!batch) {
    set_error("batch is NULL");
    return DRIN_E_NULL;
  }
  const bool bf16 = cfg->feature_dtype == DRIN_FEAT_BF16;
  if (bf16 && (pooled_mention_image || pooled_entity_image)) {
    set_error("drin_pool_fwd: with bf16 feature storage only the entity token pooling is built here (the image means of the "
              "fused path are taken inside drin_forward_prepared)");
    return DRIN_E_UNSUPPORTED;
  }
  // only the inputs of the requested outputs are needed (pooling an entity TABLE once passes the text alone)
  if ((pooled_entity_text && (!batch->entity_text || !batch->entity_text_mask)) ||
      (pooled_mention_image && !batch->mention_image) || (pooled_entity_image && !batch->entity_image)) {
    set_error("drin_pool_fwd: a requested output's input tensor is NULL");
    return DRIN_E_NULL;
  }
  if ((pooled_entity_text && !aligned16(batch->entity_text)) || (pooled_mention_image && !aligned16(batch->mention_image)) ||
      (pooled_entity_image && !aligned16(batch->entity_image))) {
    set_error("drin_pool_fwd: feature tensors must be 16-byte aligned");
    return DRIN_E_ALIGN;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t M = (int64_t)cfg->batch * cfg->num_candidates;
  if (pooled_entity_text) {
    if (cfg->entity_tokens <= 0) {
      set_error("drin_pool_fwd: entity text is already pooled when entity_tokens == 0");
      return DRIN_E_SHAPE;
    }
    if (bf16)  // tokens stored as bf16: pooled in place (half the bytes of the HBM-bound pass), fp32 sums
      DRIN_TRY(launch_entity_token_mean_bf16(batch->entity_text, batch->entity_text_mask, pooled_entity_text, M,
                                             cfg->entity_tokens, cfg->embed_dim, st));
    else
      DRIN_TRY(launch_entity_token_mean(batch->entity_text, batch->entity_text_mask, pooled_entity_text, M,
                                        cfg->entity_tokens, cfg->embed_dim, st));
  }
  if (pooled_mention_image)
    DRIN_TRY(launch_axis_mean(batch->mention_image, pooled_mention_image, cfg->batch, cfg->image_regions,
                              cfg->image_dim, st));
  if (pooled_entity_image) {
    const int inner = cfg->entity_image_inner > 0 ? cfg->entity_image_inner : 1;
    DRIN_TRY(launch_axis_mean(batch->entity_image, pooled_entity_image, M, inner, cfg->image_dim, st));
  }
  return DRIN_OK;
}

int drin_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t rows, int32_t n_out, int32_t k,
                    int32_t precision, void* stream) {
  DRIN_BIND_DEVICE(stream, y, "drin_linear_fwd");
  if (!x || !w || !y) {
    set_error("drin_linear_fwd: NULL operand");
    return DRIN_E_NULL;
  }
  if (rows < 0 || n_out <= 0 || k <= 0) {
    set_error("drin_linear_fwd: bad shape rows=%lld n_out=%d k=%d", (long long)rows, n_out, k);
    return DRIN_E_SHAPE;
  }
  return launch_gemm_nt({{x, k}, {w, k}, bias, y, n_out, rows, n_out, k}, precision, (hipStream_t)stream);
}

int drin_linear_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int64_t rows,
                    int32_t n_out, int32_t k, int32_t precision, float* scratch, size_t scratch_floats, void* stream) {
  DRIN_BIND_DEVICE(stream, dy, "drin_linear_bwd");
  if (!dy || (dx && !w) || (dw && !x)) {
    set_error("drin_linear_bwd: NULL operand");
    return DRIN_E_NULL;
  }
  if (rows < 0 || n_out <= 0 || k <= 0) {
    set_error("drin_linear_bwd: bad shape rows=%lld n_out=%d k=%d", (long long)rows, n_out, k);
    return DRIN_E_SHAPE;
  }
  if (rows == 0) return DRIN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    // the scratch holds W^T [k][n_out] for the split-bf16 form; what that leaves of it lets a partly filled last round of
    // tiles split along K
    const size_t used = Arena::rounded((size_t)n_out * k);
    const GemmScratch tail = scratch_at(scratch, used, scratch_floats > used ? scratch_floats - used : 0);
    DRIN_TRY(launch_gemm_nn({{dy, n_out}, {w, k}, dx, k, rows, k, n_out}, precision, st, {}, {nullptr, {scratch, scratch_floats}, tail}));
  }
  // (stream order makes the scratch reusable product after product; every split reduction goes through it and is added in
  //  order - without scratch one workgroup per output tile / per 256 columns walks the whole reduction: no atomics either way)
  if (dw) DRIN_TRY(launch_gemm_tn({{dy, n_out}, {x, k}, dw, k, rows, n_out, k}, precision, st, scratch_at(scratch, 0, scratch_floats)));
  if (db) DRIN_TRY(launch_colsum(dy, db, rows, n_out, st, scratch, scratch ? scratch_floats : 0));
  return DRIN_OK;
}

int drin_gemm_probe(drin_gemm_probe_args* p, void* stream) {
  char msg[256];
  const int bad = gemm_probe_check(p, msg, sizeof msg);   // (host only: before anything asks the runtime about a pointer)
  if (bad != DRIN_OK) {
    set_error("%s", msg);
    if (p != nullptr && p->struct_size == sizeof(drin_gemm_probe_args)) p->route = drin_gemm_route{};
    return bad;
  }
  p->route = drin_gemm_route{};
  DRIN_BIND_DEVICE(stream, p->y, "drin_gemm_probe");
  hipStream_t st = (hipStream_t)stream;
  gemm_route() = drin_gemm_route{};
  RowTiles rt;
  rt.begin = p->row_tile_begin, rt.end = p->row_tile_end, rt.wgs = p->row_tile_wgs;
  float* y = static_cast<float*>(p->y);
  const float* a = static_cast<const float*>(p->a);
  // the NT ops' product; DRIN_PROBE_GEMM_NT reads only b_hi, as the one-pointer "hi then lo" planes of a workspace
  NtProduct nt{{a, p->lda}, {static_cast<const float*>(p->b), p->ldb}, p->bias, y, p->ldy, p->rows, p->n_out, p->k, p->b_hi, p->b_lo};
  nt.accumulate = p->accumulate != 0;
  const GemmScratch scratch{p->scratch, p->scratch_floats};
  int rc = DRIN_E_UNSUPPORTED;
  switch (p->op) {
    case DRIN_PROBE_GEMM_NT: rc = launch_gemm_nt(nt.with_planes(static_cast<const float*>(p->b_hi)), p->precision, st, scratch); break;
    case DRIN_PROBE_GEMM_NT_BF16X3:
      nt.x_index = p->a_index;
      rc = launch_gemm_nt_bf16x3(nt, st, scratch);
      break;
    case DRIN_PROBE_GEMM_NT_BF16X3_P4: rc = launch_gemm_nt_bf16x3_p4(nt, st, scratch, rt); break;
    case DRIN_PROBE_GEMM_X3_PLANES:
      rc = launch_gemm_x3_planes(p->a, p->a_lo, p->lda, p->b_hi, p->b_lo, p->ldb, p->bias, y, p->ldy, p->rows, p->n_out, p->k, st, scratch, rt);
      break;
    case DRIN_PROBE_GEMM_F16_PLANES:
      rc = launch_gemm_f16_planes(p->a, p->lda, p->b_hi, p->ldb, p->row_scale, p->b_scale, y, p->ldy, p->rows, p->n_out, p->k, st, scratch);
      break;
    case DRIN_PROBE_TO_F16_SCALED: rc = launch_to_f16_scaled(a, p->y, p->rows, p->scratch, st); break;
    default: break;
  }
  p->route = gemm_route();
  return rc;
}

// the ops of drin_wgrad_probe, each the module's own launcher on the caller's products
static int wgrad_probe_run(const drin_wgrad_probe_args* p, hipStream_t st) {
  const drin_wgrad_product* q = p->product;
  const int n = p->n_products;
  TnProduct tn[DRIN_WGRAD_PROBE_MAX];
  for (int i = 0; i < n; ++i) tn[i] = {{q[i].dy, q[i].lddy}, {q[i].x, q[i].ldx}, q[i].dw, q[i].lddw, q[i].rows, q[i].n_out, q[i].k, q[i].x_index, q[i].db};
  const GemmScratch scratch{p->scratch, p->scratch_floats};
  switch (p->op) {
    case DRIN_WGRAD_TN_GROUP: {
      TnGroup g;
      for (int i = 0; i < n; ++i) DRIN_TRY(g.add(tn[i]));
      return launch_gemm_tn_group(g, st, scratch);
    }
    case DRIN_WGRAD_TN_F32_GROUP: {
      F32GemmGroup g;
      for (int i = 0; i < n; ++i) DRIN_TRY(g.add_tn(tn[i]));
      return launch_gemm_tn_f32_group(g, st, scratch);
    }
    case DRIN_WGRAD_TN: return launch_gemm_tn(tn[0], p->precision, st, scratch);
    case DRIN_WGRAD_COLSUM_BATCH: {
      ColsumBatch b;
      for (int i = 0; i < n; ++i) DRIN_TRY(b.add(q[i].dy, q[i].db, q[i].rows, q[i].n_out, q[i].lddy));
      return launch_colsum_batch(b, st, p->scratch, p->scratch_floats);
    }
    case DRIN_WGRAD_PASS: {
      // the three parts of the pass, sized by the functions the workspace layouts size them with
      size_t tile = 0, widest = 0, small_floats = 0;
      for (int i = 0; i < n; ++i) {
        const size_t nk = (size_t)q[i].n_out * q[i].k;
        tile = nk > tile ? nk : tile;
        widest = (size_t)q[i].n_out > widest ? (size_t)q[i].n_out : widest;
        small_floats += Arena::rounded((size_t)small_tn_slices(q[i].rows) * nk);
      }
      Arena arena;
      const size_t tn_floats = tn_group_floats(tile, widest), cs_floats = colsum_batch_floats(widest);
      const size_t tn_at = arena.take(tn_floats), cs_at = arena.take(cs_floats), small_at = arena.take(small_floats);
      if (p->scratch == nullptr || arena.total > p->scratch_floats) {
        set_error("drin_wgrad_probe: the pass needs %zu floats of scratch, %zu given", arena.total, p->scratch_floats);
        return DRIN_E_WORKSPACE;
      }
      WeightGradPass pass{p->precision, false, st, {Arena::at(p->scratch, tn_at), tn_floats}, {Arena::at(p->scratch, small_at), small_floats},
                          {Arena::at(p->scratch, cs_at), cs_floats}};
      for (int i = 0; i < n; ++i) {
        DRIN_TRY(pass.add(tn[i]));
        if (i == p->layers_done_after) pass.layers_done();
      }
      if (!p->staged) return pass.finish(nullptr);
      hipEvent_t ev = nullptr;
      if (hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); e != hipSuccess) return hip_fail(e, "hipEventCreate(wgrad probe)");
      const int rc = pass.finish(ev);
      (void)hipEventDestroy(ev);   // (a recorded event is released once it has completed)
      return rc;
    }
    case DRIN_WGRAD_NN: {
      // dX [rows][k] (+)= dY [rows][n_out] W [n_out][k]: launch_gemm_nn's (M, N, K) = (rows, k, n_out)
      WtForms wt;
      if (p->wt_form != DRIN_WGRAD_WT_NONE && p->wt_floats < (size_t)q->n_out * q->k) {
        set_error("drin_wgrad_probe: %zu floats for W^T, %zu needed", p->wt_floats, (size_t)q->n_out * q->k);
        return DRIN_E_WORKSPACE;
      }
      if (p->wt_form == DRIN_WGRAD_WT_F32_SCRATCH) wt.scratch = {p->wt, p->wt_floats};
      if (p->wt_form == DRIN_WGRAD_WT_PLANES) {
        if (q->ldx != q->k) {
          set_error("drin_wgrad_probe: the planes of W^T are written from a contiguous W (ldx == k)");
          return DRIN_E_SHAPE;
        }
        SplitBatch tb;
        DRIN_TRY(tb.add(q->x, p->wt, (int64_t)q->n_out * q->k));
        DRIN_TRY(launch_transpose_split_batch(tb, q->n_out, q->k, st));
        wt.planes = p->wt;
      }
      return launch_gemm_nn({{q->dy, q->lddy}, {q->x, q->ldx}, q->dw, q->lddw, q->rows, q->k, q->n_out, p->accumulate != 0}, p->precision, st, scratch, wt);
    }
    default: return DRIN_E_UNSUPPORTED;
  }
}

int drin_wgrad_probe(drin_wgrad_probe_args* p, void* stream) {
  char msg[256];
  const int bad = wgrad_probe_check(p, msg, sizeof msg);   // (host only: before anything asks the runtime about a pointer)
  if (bad != DRIN_OK) {
    set_error("%s", msg);
    if (p != nullptr && p->struct_size == sizeof(drin_wgrad_probe_args)) p->route = drin_wgrad_route{};
    return bad;
  }
  p->route = drin_wgrad_route{};
  DRIN_BIND_DEVICE(stream, p->product[0].dy, "drin_wgrad_probe");
  gemm_route() = drin_gemm_route{};
  WgradTrace& t = wgrad_trace();
  t.route = drin_wgrad_route{};
  t.product = p->product, t.n = p->n_products;
  const int rc = wgrad_probe_run(p, (hipStream_t)stream);
  t.product = nullptr, t.n = 0;
  p->route = t.route;
  return rc;
}

// The sizes a launcher of the layer-by-layer path refuses, asked of the launchers' own predicates among the argument checks: a
// call of drin_forward* / drin_backward* runs to its end or is refused here, before its first launch - scores, gradients and
// workspace untouched (include/drin_hip.h states the contract).  Past 65 535 mentions the path itself
// runs (sliced launches, the flat pair grid); what does not:
//   - the backward of the vector-edge update (k_edge_pre_vec_bwd_fu: one workgroup per mention, not sliced);
//   - a pair-sized product of more rows than the exact-fp32 kernel's row tiles fit in one grid.  A product takes that kernel
//     under DRIN_PREC_F32 and, under split-bf16, where its reduction length is no multiple of 32 (launch_gemm_nt,
//     launch_gemm_nt_bf16x3, gemm_nn_takes_bf16x3); the products are walked below with their rows (M = batch * num_candidates).
// both_types: both vertex types of a layer are live (two or more layers, or a traced forward of one); the dynamic edge update of
// a layer runs under the same condition.
static int layers_call_fits(const drin_config* c, bool backward, bool both_types, const char* who) {
  const int64_t M = (int64_t)c->batch * c->num_candidates;
  const int D = c->embed_dim, R = c->image_dim;
  const bool edge_updates = c->dynamic_edges && both_types, vec_updates = c->vector_edges && edge_updates;
  if (backward && vec_updates && !edge_pre_vec_bwd_fits(c->batch)) {
    set_error("%s: batch = %d: the backward of the vector-edge update is built for at most %d mentions per call; split the batch", who,
              c->batch, kMaxGridY);
    return DRIN_E_SHAPE;
  }
  const bool x3 = split_bf16(c->precision);
  int64_t rows = 0;   // of the largest product that runs exact fp32
  auto exact_fp32 = [&](int64_t product_rows, int reduction) {
    if ((!x3 || (reduction % 32)) && product_rows > rows) rows = product_rows;
  };
  exact_fp32(M, D), exact_fp32(M, R);                               // the entity vertex encoders (and the input gradients' dX)
  if (c->num_layers >= 1) exact_fp32((both_types ? 2 : 1) * M, D);  // W_h over the live entity vertex types, and its dX
  if (edge_updates) exact_fp32(2 * M, D);                           // W_v over both entity vertex types, and its dX
  if (vec_updates) {
    exact_fp32(4 * M, D);                                           // W_m over the four edge types, and its dX
    if (backward) exact_fp32(2 * M, D / 2);                         // dfv W_v: the half-width update reduces over D / 2
  }
  if (!gemm_f32_rows_fit(rows)) {
    set_error("%s: batch * num_candidates = %lld: the largest exact-fp32 product of the call has %lld rows, one such product takes "
              "%lld; split the batch", who, (long long)M, (long long)rows, (long long)kF32MaxRows);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

int drin_forward(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                 size_t workspace_bytes, float* scores, int keep_for_backward, const drin_trace* trace, void* stream) {
  return drin_forward_staged(cfg, batch, params, workspace, workspace_bytes, scores, keep_for_backward, trace, nullptr, stream);
}

int drin_forward_staged(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                        size_t workspace_bytes, float* scores, int keep_for_backward, const drin_trace* trace,
                        void* params_ready_event, void* stream) {
  return drin_forward_staged_head(cfg, batch, params, workspace, workspace_bytes, scores, keep_for_backward, trace, params_ready_event,
                                  nullptr, stream);
}

int drin_forward_staged_head(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                             size_t workspace_bytes, float* scores, int keep_for_backward, const drin_trace* trace,
                             void* params_ready_event, const drin_mention_head* head, void* stream) {
  const char* const who = head ? "drin_forward_staged_head" : "drin_forward_staged";
  DRIN_BIND_DEVICE(stream, workspace, who);
  RoctxRange range("drin_forward");
  DRIN_TRY(validate_config(cfg));
  DRIN_TRY(validate_head(head, who));
  const bool rows = rows_head(head);
  DRIN_TRY(validate_batch(cfg, batch));
  DRIN_TRY(validate_params(cfg, params, rows));
  const int64_t* eidx = batch->entity_index;
  if (eidx) DRIN_TRY(indexed_supported(cfg, "drin_forward"));
  DRIN_TRY(layers_call_fits(cfg, false, cfg->num_layers >= 2 || (trace != nullptr && cfg->num_layers >= 1), who));
  if (!scores) {
    set_error("scores is NULL");
    return DRIN_E_NULL;
  }
  Layout L;
  L.build(*cfg, keep_for_backward != 0);
  if (!workspace || !aligned16(workspace)) {
    set_error("workspace is NULL or not 16-byte aligned");
    return workspace ? DRIN_E_ALIGN : DRIN_E_NULL;
  }
  if (workspace_bytes < L.total_floats * sizeof(float)) {
    set_error("workspace has %zu bytes, needs %zu", workspace_bytes, L.total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int B = cfg->batch, N = cfg->num_candidates, D = cfg->embed_dim, R = cfg->image_dim;
  const int64_t M = (int64_t)B * N;
  const int nl = cfg->num_layers;
  const int prec = cfg->precision;
  const int act_v = vertex_act(cfg), act_e = edge_act(cfg);
  if (B == 0) return DRIN_OK;
  // dead work of the last layer (its edge update and its image-vertex updates never reach the score,
  // SURVEY.md 3.2) is only computed when a trace asks to see it
  const bool full = trace != nullptr;

  Pooled P;
  DRIN_TRY(run_pooling(cfg, batch, L, ws, &P, st, head));
  const bool vec = cfg->vector_edges != 0;
  const size_t EW = vec ? (size_t)D : 1;   // floats per edge per pair
  const size_t ES = (size_t)M * EW;        // stride between the four edge types
  if (vec) {  // model.py:202: the scalar edges are broadcast over the feature dimension
    DRIN_TRY(run_static_edges(cfg, batch, P, ws + L.edges_scalar, st));
    DRIN_TRY(launch_expand_edges(ws + L.edges_scalar, ws + L.edges[0], 4 * M, D, st));
  } else {
    DRIN_TRY(run_static_edges(cfg, batch, P, ws + L.edges[0], st));
  }

  // Everything above - the pooling passes and the static edges - reads the batch alone; from here on the parameters are
  // read.  drin_forward_staged: they are final once the caller's event has fired (the previous step's gradient all-reduce
  // and optimiser update on another stream, which the parameter-free head above has just run under).
  if (params_ready_event != nullptr) {
    hipError_t we = hipStreamWaitEvent(st, (hipEvent_t)params_ready_event, 0);
    if (we != hipSuccess) return hip_fail(we, "hipStreamWaitEvent(params_ready)");
  }
  // VertexEncoder (model.py:26-46): four Linears
  float* vm0 = ws + L.vm[0];
  float* ve0 = ws + L.ve[0];
  const GemmScratch sk = scratch_at(ws, L.splitk, L.splitk_floats);  // split-K scratch of the mention-sized products
  // tail-split scratch of the pair-sized split-bf16 products (training layouts only: the weight-gradient partial
  // buffer is idle during the forward pass and between the weight-gradient products of the backward pass)
  const GemmScratch tl = scratch_at(ws, L.tn_part, L.tn_part_floats);
  // mention-sized products beyond the exact-fp32 split-K range (2 B > 512 rows) run split-bf16 on small tiles and split K
  // into the same scratch
  const GemmScratch msk = sk.p ? sk : tl;
  // split-bf16 precision: every weight an NT product runs against is split into bf16 (hi, lo) planes ONCE per call (one
  // batched launch) and then streamed by LDS-DMA, instead of being split by every workgroup in every K-block (the register
  // stager of the 64 x 128 tile spent as many VALU cycles on it as the tile has MFMA cycles)
  auto wp = [&](size_t off) -> const float* { return L.weight_planes ? ws + off : nullptr; };
  if (L.weight_planes) {
    SplitBatch sb;
    if (!rows) DRIN_TRY(sb.add(params->w_mention_text, ws + L.wp_enc[0], (int64_t)D * D));
    DRIN_TRY(sb.add(params->w_mention_image, ws + L.wp_enc[1], (int64_t)D * R));
    DRIN_TRY(sb.add(params->w_entity_text, ws + L.wp_enc[2], (int64_t)D * D));
    DRIN_TRY(sb.add(params->w_entity_image, ws + L.wp_enc[3], (int64_t)D * R));
    for (int l = 0; l < nl; ++l) {
      DRIN_TRY(sb.add(params->layer[l].w_h, ws + L.wp_h[l], (int64_t)D * D));
      if (cfg->dynamic_edges && (l < nl - 1 || full)) {
        DRIN_TRY(sb.add(params->layer[l].w_u, ws + L.wp_u[l], (int64_t)D * D));
        DRIN_TRY(sb.add(params->layer[l].w_v, ws + L.wp_v[l], (int64_t)D * D));
      }
    }
    DRIN_TRY(launch_split_planes_batch(sb, st));
  }
  const NtProduct enc_mi = NtProduct{{P.mention_image, R}, {params->w_mention_image, R}, params->b_mention_image, vm0 + (size_t)B * D, D, B, D, R}
                               .with_planes(wp(L.wp_enc[1]));
  if (rows)   // the mention-text vertex is in vm0 already (run_pooling): the mention-image product alone
    DRIN_TRY(launch_gemm_nt(enc_mi, prec, st, msk));
  else
    DRIN_TRY(launch_gemm_nt_pair(NtProduct{{P.span_mean, D}, {params->w_mention_text, D}, params->b_mention_text, vm0, D, B, D, D}.with_planes(wp(L.wp_enc[0])),
                                 enc_mi, prec, st, msk));
  NtProduct enc_et = NtProduct{{P.entity_text, D}, {params->w_entity_text, D}, params->b_entity_text, ve0, D, M, D, D}.with_planes(wp(L.wp_enc[2]));
  NtProduct enc_ei = NtProduct{{P.entity_image, R}, {params->w_entity_image, R}, params->b_entity_image, ve0 + (size_t)M * D, D, M, D, R}
                         .with_planes(wp(L.wp_enc[3]));
  if (eidx) {  // rows of the entity tables, addressed through the candidate index by the GEMM's stager
    enc_et.x_index = enc_ei.x_index = eidx;
    DRIN_TRY(launch_gemm_nt_bf16x3(enc_et, st, tl));
    DRIN_TRY(launch_gemm_nt_bf16x3(enc_ei, st, tl));
  } else {
    DRIN_TRY(launch_gemm_nt(enc_et, prec, st, tl));
    DRIN_TRY(launch_gemm_nt(enc_ei, prec, st, tl));
  }
  DRIN_TRY(tap(trace, 0, L, ws, B, M, D, st, EW));

  bool all_enabled = true;
  for (int k = 0; k < 4; ++k) all_enabled = all_enabled && cfg->edge_enabled[k] == 1.0f;
  // gelu / silu edges (model.py:118 takes any F.* name): their derivative needs the pre-activation, kept when training
  const bool keep_z = L.training && (act_e == DRIN_ACT_GELU || act_e == DRIN_ACT_SILU);

  for (int l = 0; l < nl; ++l) {
    const drin_layer_params& W = params->layer[l];
    const bool last = l == nl - 1;
    const bool live_image = !last || full;                       // mi / ei updates
    const bool live_edges = cfg->dynamic_edges && (!last || full);
    const float* e = ws + L.edges[l];
    if (!all_enabled) {  // edges = [e * m ...] (model.py:122)
      float* me = ws + L.masked[l];
      for (int k = 0; k < 4; ++k) DRIN_TRY(launch_scale_div(e + k * ES, me + k * ES, (int64_t)ES, cfg->edge_enabled[k], 1.0f, st));
      e = me;
    }
    const float *e_tt = e, *e_ti = e + ES, *e_it = e + 2 * ES, *e_ii = e + 3 * ES;
    const float* mt = ws + L.vm[l];
    const float* mi = mt + (size_t)B * D;
    const float* et = ws + L.ve[l];
    const float* ei = et + (size_t)M * D;
    float* agg_m = ws + L.agg_m[l];
    float* agg_e = ws + L.agg_e[l];
    // neighbour aggregation, vertex_graph of model.py:105
    if (vec) {
      const float inv_n = 1.0f / (float)N;
      DRIN_TRY(launch_mention_reduce_vec(e_tt, et, e_ti, ei, mt, agg_m, B, N, D, inv_n, true, st));
      DRIN_TRY(launch_entity_aggregate_vec(e_tt, mt, e_it, mi, et, agg_e, B, N, D, st));
      if (live_image) {
        DRIN_TRY(launch_mention_reduce_vec(e_it, et, e_ii, ei, mi, agg_m + (size_t)B * D, B, N, D, inv_n, true, st));
        DRIN_TRY(launch_entity_aggregate_vec(e_ti, mt, e_ii, mi, ei, agg_e + (size_t)M * D, B, N, D, st));
      }
    } else {
      DRIN_TRY(launch_layer_aggregate(e, (int64_t)ES, mt, et, agg_m, agg_e, B, N, D, live_image, st));
    }
    const int types = live_image ? 2 : 1;
    // shared W_h + LayerNorm + GELU for all vertex types of the layer (model.py:128)
    float* h_m = ws + L.h_m[l];
    float* h_e = ws + L.h_e[l];
    const bool scalar_update = live_edges && !vec;   // then W_u(mt, mi) is due too and shares the launch of W_h(agg_m)
    const NtProduct wh_m = NtProduct{{agg_m, D}, {W.w_h, D}, W.b_h, h_m, D, (int64_t)types * B, D, D}.with_planes(wp(L.wp_h[l]));
    if (scalar_update) {
      DRIN_TRY(launch_gemm_nt_pair(wh_m, NtProduct{{mt, D}, {W.w_u, D}, W.b_u, ws + L.fu[l], D, 2 * (int64_t)B, D, D}.with_planes(wp(L.wp_u[l])),
                                   prec, st, msk));
    } else {
      DRIN_TRY(launch_gemm_nt(wh_m, prec, st, msk));
    }
    DRIN_TRY(launch_gemm_nt(NtProduct{{agg_e, D}, {W.w_h, D}, W.b_h, h_e, D, (int64_t)types * M, D, D}.with_planes(wp(L.wp_h[l])), prec, st, tl));
    float* st_m = L.training ? ws + L.ln_stat_m[l] : nullptr;
    float* st_e = L.training ? ws + L.ln_stat_e[l] : nullptr;
    // one LayerNorm + GELU launch for the mention and the entity vertices (they share it, model.py:128)
    DRIN_TRY(launch_layernorm_gelu2(h_m, ws + L.vm[l + 1], st_m, st_m ? st_m + 2 * (size_t)B : nullptr, (int64_t)types * B, h_e,
                                    ws + L.ve[l + 1], st_e, st_e ? st_e + 2 * (size_t)M : nullptr, (int64_t)types * M,
                                    W.ln_weight, W.ln_bias, D, cfg->layer_norm_eps, st, act_v));
    // dynamic edges, edge_graph of model.py:107: (mt,et) (mt,ei) (mi,et) (mi,ei)
    float* e_next = ws + L.edges[l + 1];
    if (live_edges && vec) {
      // model.py:150-152,133: cat(W_u(u), W_v(v)) + e -> W_m -> sigmoid, W_u / W_v: D -> D/2
      float* fu = ws + L.fu[l];
      float* fv = ws + L.fv[l];
      float* pre = ws + L.pre[l];
      const int H = D / 2;
      DRIN_TRY(launch_gemm_nt({{mt, D}, {W.w_u, D}, W.b_u, fu, H, 2 * (int64_t)B, H, D}, prec, st, msk));
      DRIN_TRY(launch_gemm_nt({{et, D}, {W.w_v, D}, W.b_v, fv, H, 2 * M, H, D}, prec, st));
      DRIN_TRY(launch_edge_pre_vec(fu, fv, e, pre, B, N, D, st));
      DRIN_TRY(launch_gemm_nt({{pre, D}, {W.w_m, D}, W.b_m, e_next, D, 4 * M, D, D}, prec, st));
      DRIN_TRY(launch_sigmoid_inplace(e_next, 4 * M * D, st, act_e, keep_z ? ws + L.edge_z[l] : nullptr));
    } else if (live_edges) {
      float* fu = ws + L.fu[l];
      float* fv = ws + L.fv[l];
      DRIN_TRY(launch_gemm_nt(NtProduct{{et, D}, {W.w_v, D}, W.b_v, fv, D, 2 * M, D, D}.with_planes(wp(L.wp_v[l])), prec, st, tl));   // fu: with W_h above
      DRIN_TRY(launch_edge_update4(fu, fv, e, e_next, B, N, D, st, act_e, keep_z ? ws + L.edge_z[l] : nullptr));
    } else if (!cfg->dynamic_edges) {
      hipError_t err = hipMemcpyAsync(e_next, e, 4 * ES * sizeof(float), hipMemcpyDeviceToDevice, st);
      if (err != hipSuccess) return hip_fail(err, "hipMemcpyAsync(static edges)");
    }
    if (full) DRIN_TRY(tap(trace, l + 1, L, ws, B, M, D, st, EW));
  }
  // score (model.py:207-209)
  return launch_cosine_rows(ws + L.vm[nl], ws + L.ve[nl], D, scores, B, N, D, cfg->cosine_eps, 1.0f, st);
}

int drin_profile_begin(int max_launches) {
  std::lock_guard<std::mutex> lock(g_prof_mutex);
  Profile& p = g_prof;
  if (p.open.load()) profile_free(p);
  if (max_launches <= 0 || max_launches > (1 << 20)) {
    set_error("drin_profile_begin: max_launches=%d outside (0, 2^20]", max_launches);
    return DRIN_E_SHAPE;
  }
  p.start = new hipEvent_t[max_launches];
  p.stop = new hipEvent_t[max_launches];
  p.cls = new int[max_launches];
  for (int i = 0; i < max_launches; ++i) {
    hipError_t e = hipEventCreate(&p.start[i]);
    if (e == hipSuccess) e = hipEventCreate(&p.stop[i]);
    if (e != hipSuccess) {
      p.capacity = i;
      profile_free(p);
      return hip_fail(e, "hipEventCreate");
    }
  }
  p.capacity = max_launches;
  p.used.store(0);
  p.open.store(true, std::memory_order_release);
  return DRIN_OK;
}

int drin_profile_end(double* ms_by_class, int64_t* launches_by_class) {
  std::lock_guard<std::mutex> lock(g_prof_mutex);
  Profile& p = g_prof;
  if (!p.open.load()) {
    set_error("drin_profile_end: no profile open");
    return DRIN_E_SHAPE;
  }
  for (int k = 0; k < DRIN_KC_COUNT; ++k) {
    if (ms_by_class) ms_by_class[k] = 0.0;
    if (launches_by_class) launches_by_class[k] = 0;
  }
  int status = DRIN_OK;
  p.open.store(false);  // launches from other threads stop claiming slots from here on
  const int claimed = p.used.load();
  const int used = claimed < p.capacity ? claimed : p.capacity;
  for (int i = 0; i < used; ++i) {
    hipError_t e = hipEventSynchronize(p.stop[i]);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.start[i], p.stop[i]);
    if (e != hipSuccess) {
      status = hip_fail(e, "hipEventElapsedTime");
      break;
    }
    const int k = p.cls[i];
    if (k >= 0 && k < DRIN_KC_COUNT) {
      if (ms_by_class) ms_by_class[k] += ms;
      if (launches_by_class) launches_by_class[k] += 1;
    }
  }
  if (status == DRIN_OK && claimed >= p.capacity) {
    set_error("drin_profile_end: profile overflowed its %d launch slots", p.capacity);
    status = DRIN_E_SHAPE;
  }
  profile_free(p);
  return status;
}

const char* drin_kernel_class_name(int kernel_class) {
  static const char* names[DRIN_KC_COUNT] = {"gemm", "pool", "edge", "gcn", "stream", "gemm_x3", "gemm_planes", "optim", "lstm", "cell", "attn", "norm"};
  return (kernel_class >= 0 && kernel_class < DRIN_KC_COUNT) ? names[kernel_class] : "?";
}

int drin_backward(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                  size_t workspace_bytes, const float* grad_scores, const drin_param_grads* grads, void* stream) {
  return drin_backward_staged(cfg, batch, params, workspace, workspace_bytes, grad_scores, grads, nullptr, stream);
}

int drin_backward_staged(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                         size_t workspace_bytes, const float* grad_scores, const drin_param_grads* grads,
                         void* layers_ready_event, void* stream) {
  if (!grads) {
    set_error("drin_backward: grad_scores / grads is NULL");
    return DRIN_E_NULL;
  }
  return drin_backward_ex(cfg, batch, params, workspace, workspace_bytes, grad_scores, grads, nullptr, layers_ready_event,
                          stream);
}

size_t drin_input_grad_scratch_bytes(const drin_config* cfg) {
  if (validate_config(cfg) != DRIN_OK) return 0;
  InputGradScratch S;
  S.build(*cfg);
  return S.total_floats * sizeof(float);
}

int drin_pool_bwd(const drin_config* cfg, const int64_t* entity_text_mask, const float* grad_pooled, const float* grad_cls,
                  void* grad_entity_text, void* stream) {
  DRIN_BIND_DEVICE(stream, grad_entity_text, "drin_pool_bwd");
  DRIN_TRY(validate_config(cfg));
  if (!entity_text_mask || !grad_pooled || !grad_entity_text) {
    set_error("drin_pool_bwd: mask, pooled gradient or output is NULL");
    return DRIN_E_NULL;
  }
  if (cfg->entity_tokens <= 0) {
    set_error("drin_pool_bwd: entity_tokens must be > 0 (a token block)");
    return DRIN_E_SHAPE;
  }
  if (!aligned16(grad_pooled) || !aligned16(grad_cls) || !aligned16(grad_entity_text)) {
    set_error("drin_pool_bwd: gradients must be 16-byte aligned");
    return DRIN_E_ALIGN;
  }
  const int64_t M = (int64_t)cfg->batch * cfg->num_candidates;
  return launch_token_block_bwd(grad_pooled, grad_cls, entity_text_mask, grad_entity_text, M, cfg->entity_tokens,
                                cfg->embed_dim, cfg->feature_dtype == DRIN_FEAT_BF16, (hipStream_t)stream);
}

int drin_backward_ex(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                     size_t workspace_bytes, const float* grad_scores, const drin_param_grads* grads_in,
                     const drin_input_grads* input_grads, void* layers_ready_event, void* stream) {
  return drin_backward_head(cfg, batch, params, workspace, workspace_bytes, grad_scores, grads_in, input_grads, layers_ready_event,
                            nullptr, stream);
}

int drin_backward_head(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                       size_t workspace_bytes, const float* grad_scores, const drin_param_grads* grads_in,
                       const drin_input_grads* input_grads, void* layers_ready_event, const drin_mention_head* head, void* stream) {
  const char* const who = head ? "drin_backward_head" : "drin_backward_staged";
  DRIN_BIND_DEVICE(stream, workspace, who);
  RoctxRange range("drin_backward");
  DRIN_TRY(validate_config(cfg));
  DRIN_TRY(validate_head(head, who));
  const bool rows = rows_head(head);
  DRIN_TRY(validate_batch(cfg, batch));
  DRIN_TRY(validate_params(cfg, params, rows));
  if (!grad_scores) {
    set_error("drin_backward: grad_scores / grads is NULL");
    return DRIN_E_NULL;
  }
  // no parameter gradients wanted: every dW / db destination is NULL, so no weight-gradient product is issued
  static const drin_param_grads kNoGrads = {};
  const drin_param_grads* grads = grads_in ? grads_in : &kNoGrads;
  const int64_t* eidx = batch->entity_index;
  if (eidx) DRIN_TRY(indexed_supported(cfg, "drin_backward"));
  DRIN_TRY(layers_call_fits(cfg, true, cfg->num_layers >= 2, who));
  if (input_grads) DRIN_TRY(validate_input_grads(cfg, batch, input_grads));
  Layout L;
  L.build(*cfg, true);
  if (!workspace || !aligned16(workspace)) {
    set_error("workspace is NULL or not 16-byte aligned");
    return workspace ? DRIN_E_ALIGN : DRIN_E_NULL;
  }
  if (workspace_bytes < L.total_floats * sizeof(float)) {
    set_error("workspace has %zu bytes, needs %zu (was drin_forward run with keep_for_backward?)", workspace_bytes,
              L.total_floats * sizeof(float));
    return DRIN_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int B = cfg->batch, N = cfg->num_candidates, D = cfg->embed_dim, R = cfg->image_dim;
  const size_t M = (size_t)B * N, BD = (size_t)B * D, MD = M * D;
  const int nl = cfg->num_layers;
  const int prec = cfg->precision;
  const int act_v = vertex_act(cfg), act_e = edge_act(cfg);
  if (B == 0) return DRIN_OK;
  Pooled P;
  resolve_pooled(cfg, batch, L, ws, &P);

  // the pass's temporaries (layout.h: BackwardScratch), in Layout::bwd_scratch
  BackwardScratch S;
  S.build(*cfg);
  float* const sc = Arena::at(ws, L.bwd_scratch);
  auto g_vm = [&](int l) { return sc + S.g_vm[l]; };
  auto g_ve = [&](int l) { return sc + S.g_ve[l]; };
  float* const g_e[2] = {sc + S.g_e[0], sc + S.g_e[1]};
  float* const dA_m = sc + S.dA_m;
  float* const dA_e = sc + S.dA_e;
  float* const dpre = sc + S.dpre;
  const bool vec = cfg->vector_edges != 0;
  const size_t EW = vec ? (size_t)D : 1, ES = M * EW;  // floats per edge per pair, stride between edge types

  bool all_enabled = true;
  for (int k = 0; k < 4; ++k) all_enabled = all_enabled && cfg->edge_enabled[k] == 1.0f;
  const GemmScratch tn = scratch_at(ws, L.tn_part, L.tn_part_floats);  // partial tiles of the split-bf16 dW products
  // gelu / silu edges: the derivative is taken at the pre-activation the forward kept (Layout::edge_z)
  const bool from_z = act_e == DRIN_ACT_GELU || act_e == DRIN_ACT_SILU;
  const int act_eb = from_z ? (act_e | 0x100) : act_e;   // device_utils.h: kActFromPre
  float* const csp = ws + L.colsum_part;    // partial rows of the bias column sums
  // dX (+)= dY W (launch_gemm_nn).  Scalar edges: W_h^T and W_v^T of every layer in ONE batched transpose up front (slots
  // 2 l and 2 l + 1 of L.wt), split into bf16 (hi, lo) planes in the same pass - the NT kernel streams them by LDS-DMA;
  // anything else (W_u at 512+ mentions; the half-width W_u / W_v and W_m of vector edges) that takes split-bf16 is
  // transposed per product into the last slot, never one of the pre-transposed weights
  const bool pre_t = !cfg->vector_edges && gemm_nn_takes_bf16x3(prec, (int64_t)M, D, D);
  auto wt_slot = [&](int l, int which) { return ws + L.wt + ((size_t)2 * l + which) * D * D; };
  if (pre_t) {
    SplitBatch tb;
    for (int l = 0; l < nl; ++l) {
      DRIN_TRY(tb.add(params->layer[l].w_h, wt_slot(l, 0), (int64_t)D * D));
      if (cfg->dynamic_edges && l < nl - 1) DRIN_TRY(tb.add(params->layer[l].w_v, wt_slot(l, 1), (int64_t)D * D));
    }
    DRIN_TRY(launch_transpose_split_batch(tb, D, D, st));
  }
  const GemmScratch nn_sk = scratch_at(ws, L.splitk, L.splitk_floats);
  // w_t: bf16 (hi, lo) planes of w^T, already in the workspace
  auto wt = [&](const float* w_t = nullptr) { return WtForms{w_t, {wt_slot(nl, 0), (size_t)D * D}, tn}; };
  // dW (+)= dY^T X with its bias gradient: kernel choice, grouped launches and the order of landing are the GEMM module's
  WeightGradPass dw{prec, vec, st, tn, {ws + L.small_part, L.small_part_floats}, {csp, L.colsum_part_floats}};

  // score = cos(mt_L, et_L) (model.py:207-209)
  DRIN_TRY(launch_cosine_bwd(ws + L.vm[nl], ws + L.ve[nl], grad_scores, g_vm(nl), g_ve(nl), sc + S.cos_scratch, B, N, D,
                             cfg->cosine_eps, st));
  bool have_image = false;  // gradients w.r.t. the image vertices of the current level exist
  bool have_edge = false;   // gradients w.r.t. the current level's edges exist

  for (int l = nl - 1; l >= 0; --l) {
    const drin_layer_params& W = params->layer[l];
    const auto& G = grads->layer[l];
    const int types = have_image ? 2 : 1;
    float* gm = g_vm(l + 1);  // dL/d(new mention vertices) -> dL/dH in place
    float* ge = g_ve(l + 1);
    float* gm_next = g_vm(l);
    float* ge_next = g_ve(l);
    float* dfv = sc + S.dfv_of[l];
    float* dfu = sc + S.dfu_of[l];
    const int cur = (nl - 1 - l) & 1, nxt = cur ^ 1;  // the edge gradients keep two generations
    const float* st_m = ws + L.ln_stat_m[l];
    const float* st_e = ws + L.ln_stat_e[l];
    // (a) LayerNorm + GELU backward; column sums give dgamma, dbeta and db_h
    // (mention and entity rows in one launch)
    // (its column sums' second level rides in the slice sum at the end of the pass: per-layer level-1 rows behind the block rows)
    DRIN_TRY(launch_layernorm_gelu_bwd2(ws + L.h_m[l], st_m, st_m + 2 * (size_t)B, gm, (int64_t)types * B, ws + L.h_e[l], st_e,
                                        st_e + 2 * M, ge, (int64_t)types * M, W.ln_weight, W.ln_bias, G.ln_weight, G.ln_bias,
                                        G.b_h, ws + L.ln_part, D, st, act_v, nl <= 2 ? &dw.ln_sums : nullptr,
                                        ws + L.ln_part + ln_bwd_level1((size_t)D, l)));
    // (b) dW_h += dH^T A
    if (G.w_h) {
      DRIN_TRY(dw.add({{gm, D}, {ws + L.agg_m[l], D}, G.w_h, D, (int64_t)types * B, D, D}));
      DRIN_TRY(dw.add({{ge, D}, {ws + L.agg_e[l], D}, G.w_h, D, (int64_t)(types * M), D, D}));
    }
    // (c) dA = dH W_h
    DRIN_TRY(launch_gemm_nn({{gm, D}, {W.w_h, D}, dA_m, D, (int64_t)types * B, D, D}, prec, st, nn_sk, wt()));
    DRIN_TRY(launch_gemm_nn({{ge, D}, {W.w_h, D}, dA_e, D, (int64_t)(types * M), D, D}, prec, st, nn_sk, wt(pre_t ? wt_slot(l, 0) : nullptr)));
    const float* dA_mt = dA_m;
    const float* dA_mi = types == 2 ? dA_m + BD : nullptr;
    const float* dA_et = dA_e;
    const float* dA_ei = types == 2 ? dA_e + MD : nullptr;

    const float* e = all_enabled ? ws + L.edges[l] : ws + L.masked[l];
    const float* mt = ws + L.vm[l];
    const float* mi = mt + BD;
    const float* et = ws + L.ve[l];
    const float* ei = et + MD;
    const bool edge_update = cfg->dynamic_edges && have_edge;  // this layer's edge update is live
    const float* de_extra = nullptr;
    if (edge_update && vec) {
      // (d, vector edges) e' = sigmoid(W_m(cat(W_u(u), W_v(v)) + e) + b_m)  (model.py:150-152,133)
      const int H = D / 2;
      DRIN_TRY(launch_sigmoid_bwd(g_e[cur], from_z ? ws + L.edge_z[l] : ws + L.edges[l + 1], dpre, 4 * (int64_t)ES, st, act_eb));  // dz
      if (G.w_m) DRIN_TRY(launch_gemm_tn({{dpre, D}, {ws + L.pre[l], D}, G.w_m, D, 4 * (int64_t)M, D, D}, prec, st, tn));
      DRIN_TRY(launch_colsum(dpre, G.b_m, 4 * (int64_t)M, D, st, csp, L.colsum_part_floats));
      DRIN_TRY(launch_gemm_nn({{dpre, D}, {W.w_m, D}, g_e[cur], D, 4 * (int64_t)M, D, D}, prec, st, nn_sk, wt()));  // d(cat + e)
      DRIN_TRY(launch_edge_pre_vec_bwd(g_e[cur], dfu, dfv, B, N, D, st));
      if (G.w_v) DRIN_TRY(launch_gemm_tn({{dfv, H}, {et, D}, G.w_v, D, 2 * (int64_t)M, H, D}, prec, st, tn));
      DRIN_TRY(launch_colsum(dfv, G.b_v, 2 * (int64_t)M, H, st, csp, L.colsum_part_floats));
      if (G.w_u) DRIN_TRY(launch_gemm_tn({{dfu, H}, {mt, D}, G.w_u, D, 2 * (int64_t)B, H, D}, prec, st, tn));
      DRIN_TRY(launch_colsum(dfu, G.b_u, 2 * (int64_t)B, H, st, csp, L.colsum_part_floats));
      de_extra = g_e[cur];
    } else if (edge_update) {
      // (d) e'_k = sigmoid(mean_d(fu fv) + e_k)  (model.py:148-153,133)
      const float* fu = ws + L.fu[l];
      const float inv_d = 1.0f / (float)D;
      // dpre = g e' (1 - e');  dfv_t = (dpre_tt fu_t + dpre_it fu_i) / D ; dfv_i = (dpre_ti fu_t + dpre_ii fu_i) / D: one pass
      DRIN_TRY(launch_edge_update_bwd(g_e[cur], from_z ? ws + L.edge_z[l] : ws + L.edges[l + 1], fu, dpre, dfv, B, N, D, inv_d, st, act_eb));
      // dfu_t = sum_n (dpre_tt fv_t + dpre_ti fv_i) / D ; dfu_i = sum_n (dpre_it fv_t + dpre_ii fv_i) / D: with the mention
      // side of the aggregation backward, (f) below, in ONE launch; dW_u, which reads dfu, is collected behind it
      DRIN_TRY(dw.add({{dfv, D}, {et, D}, G.w_v, D, 2 * (int64_t)M, D, D, nullptr, G.b_v}));
      de_extra = dpre;
    } else if (!cfg->dynamic_edges && have_edge) {
      de_extra = g_e[cur];  // static edges pass through (model.py:136)
    }
    if (vec) {
      const int H = D / 2;
      // (e) entity side of the aggregation backward + edge gradients, element-wise with vector edges
      DRIN_TRY(launch_entity_side_bwd_vec(dA_mt, dA_mi, dA_et, dA_ei, mt, mi, et, ei, e, de_extra, ge_next,
                                          ge_next + MD, g_e[nxt], B, N, D, cfg->edge_enabled, st));
      if (edge_update) DRIN_TRY(launch_gemm_nn({{dfv, H}, {W.w_v, D}, ge_next, D, 2 * (int64_t)M, D, H, true}, prec, st, nn_sk, wt()));
      // (f) mention side
      DRIN_TRY(launch_mention_reduce_vec(e, dA_et, e + ES, dA_ei, dA_mt, gm_next, B, N, D, 1.0f, false, st));
      DRIN_TRY(launch_mention_reduce_vec(e + 2 * ES, dA_et, e + 3 * ES, dA_ei, dA_mi, gm_next + BD, B, N, D, 1.0f, false, st));
      if (edge_update) DRIN_TRY(launch_gemm_nn({{dfu, H}, {W.w_u, D}, gm_next, D, 2 * (int64_t)B, D, H, true}, prec, st, nn_sk, wt()));
    } else {
      // (e) entity side of the aggregation backward + edge gradients
      // (the edge update's dfv W_v goes first and the row kernel adds onto it)
      if (edge_update)
        DRIN_TRY(launch_gemm_nn({{dfv, D}, {W.w_v, D}, ge_next, D, 2 * (int64_t)M, D, D}, prec, st, nn_sk, wt(pre_t ? wt_slot(l, 1) : nullptr)));
      DRIN_TRY(launch_entity_side_bwd(dA_mt, dA_mi, dA_et, dA_ei, mt, mi, et, ei, e, de_extra, ge_next, ge_next + MD,
                                      g_e[nxt], B, N, D, cfg->edge_enabled, edge_update, st));
      // (f) mention side
      if (edge_update) {
        const float* fv = ws + L.fv[l];
        DRIN_TRY(launch_mention_reduce2_pair(dpre, fv, fv + MD, nullptr, nullptr, dfu, dfu + BD, 1.0f / (float)D,          // (d): dfu
                                             e, dA_et, dA_ei, dA_mt, dA_mi, gm_next, gm_next + BD, 1.0f, B, N, D, st));   // (f)
        DRIN_TRY(dw.add({{dfu, D}, {mt, D}, G.w_u, D, 2 * (int64_t)B, D, D, nullptr, G.b_u}));
      } else {
        DRIN_TRY(launch_mention_reduce2(e, dA_et, dA_ei, dA_mt, dA_mi, gm_next, gm_next + BD, B, N, D, 1.0f, st));
      }
      if (edge_update) DRIN_TRY(launch_gemm_nn({{dfu, D}, {W.w_u, D}, gm_next, D, 2 * (int64_t)B, D, D, true}, prec, st, nn_sk, wt()));
    }
    have_image = true;
    have_edge = true;
    // dfv / dfu are overwritten by the next layer down: their column sums go now - except layer 0's, which share the
    // launch of the vertex encoders' bias gradients below
    if (l > 0) DRIN_TRY(dw.flush_bias_sums());
  }

  dw.layers_done();   // (drin_backward_staged: what follows belongs to the vertex encoders)
  // VertexEncoder (model.py:26-46): four Linears over the pooled inputs
  const float* g_mt = g_vm(0);
  const float* g_mi = g_vm(0) + BD;
  const float* g_et = g_ve(0);
  const float* g_ei = g_ve(0) + MD;
  if (!rows) DRIN_TRY(dw.add({{g_mt, D}, {P.span_mean, D}, grads->w_mention_text, D, B, D, D, nullptr, grads->b_mention_text}));
  DRIN_TRY(dw.add({{g_et, D}, {P.entity_text, D}, grads->w_entity_text, D, (int64_t)M, D, D, eidx, grads->b_entity_text}));
  if (have_image) {
    DRIN_TRY(dw.add({{g_mi, D}, {P.mention_image, R}, grads->w_mention_image, R, B, D, R, nullptr, grads->b_mention_image}));
    DRIN_TRY(dw.add({{g_ei, D}, {P.entity_image, R}, grads->w_entity_image, R, (int64_t)M, D, R, eidx, grads->b_entity_image}));
  }
  DRIN_TRY(dw.finish(layers_ready_event));   // everything collected lands; staged: the layers' part, the event, the encoders' part
  if (input_grads == nullptr) {
    // parameters alone are training: the intermediate layer's still need the gradient of its output (the vertex row's term)
    if (rows && head->grad_encoded != nullptr) {
      int32_t *ie, *iv;
      head_positions(cfg, head, &ie, &iv);
      DRIN_TRY(launch_mention_rows_bwd(nullptr, g_mt, batch->mention_start, batch->mention_end, ie, iv, head->representation, true, nullptr,
                                       head->grad_encoded, B, cfg->mention_tokens, D, st));
    }
    return DRIN_OK;
  }
  // the batch tensors' gradients (drin_backward_ex): from the vertex encoders' output gradients and the layer-0 edge
  // gradients, which the layer loop left in g_vm(0) / g_ve(0) / g_e[nl & 1] (nothing above writes them after the loop)
  return run_input_grads(cfg, batch, params, P, nl > 0 ? g_e[nl & 1] : nullptr, g_vm(0), g_ve(0), input_grads, st, head);
}

// ---- host-side self-checks (sanitizer build / CI; no launch is made, no GPU needed) -----------------------------------
int drin_host_selftest(void) {
  // (1) the slice scratch of the mention-sized weight-gradient group covers its worst case at every batch size
  for (int precision : {(int)DRIN_PREC_F32, (int)DRIN_PREC_BF16X3})
    for (int nl : {1, 2, 3})
      for (int n : {1, 11, 101})
        for (int dims = 0; dims < 2; ++dims)
          for (int b = 1; b <= 4300; b += (b < 48 ? 1 : 7)) {
            drin_config c;
            drin_default_config(&c);
            c.batch = b, c.num_candidates = n, c.num_layers = nl, c.precision = precision;
            if (dims) c.embed_dim = 64, c.image_dim = 128;
            Layout L;
            L.build(c, true);
            const size_t need = small_group_worst_case_floats(c, L.tn_part_floats);
            if (need > L.small_part_floats) {
              set_error("selftest: B=%d N=%d layers=%d D=%d precision=%d: the mention-sized weight-gradient group may store %zu "
                        "floats of slices, Layout::small_part_floats = %zu", b, n, nl, c.embed_dim, precision, need, L.small_part_floats);
              return DRIN_E_WORKSPACE;
            }
          }
  // (2) a grouped launch refuses an item with an empty reduction instead of deriving a slice length of 0 from it and
  //     dividing by that (the SIGFPE of round 3's staged backward: value-initialised items past a flushed group)
  alignas(16) static float dummy[16];
  {
    F32GemmGroup g;
    g.n = 2;
    g.item[0] = {{dummy, 4}, {dummy, 4}, dummy, 4, 4, 4, 4};
    g.item[1] = TnProduct();   // M = N = K = 0, NULL operands
    const int rc = launch_gemm_tn_f32_group(g, nullptr, {}, nullptr);
    if (rc != DRIN_E_SHAPE) {
      set_error("selftest: launch_gemm_tn_f32_group accepted an item with an empty reduction (status %d)", rc);
      return rc == DRIN_OK ? DRIN_E_SHAPE : rc;
    }
    F32GemmGroup h;
    h.n = 1;
    h.nt[0] = NtProduct();
    const int rn = launch_gemm_nt_f32_group(h, nullptr, {dummy, 16});
    if (rn != DRIN_E_SHAPE) {
      set_error("selftest: launch_gemm_nt_f32_group accepted an empty item (status %d)", rn);
      return rn == DRIN_OK ? DRIN_E_SHAPE : rn;
    }
  }
  // (3) an empty reduction through the single-product entry: nothing to add, nothing launched, nothing divided
  {
    TnProduct empty{{dummy, 4}, {dummy, 4}, dummy, 4, /*rows=*/0, 4, 4};
    const int rc = launch_gemm_tn(empty, DRIN_PREC_F32, nullptr, {dummy, 16});
    if (rc != DRIN_OK) return rc;
    empty.rows = -1;
    if (launch_gemm_tn(empty, DRIN_PREC_F32, nullptr, {dummy, 16}) != DRIN_E_SHAPE) {
      set_error("selftest: launch_gemm_tn accepted a negative reduction length");
      return DRIN_E_SHAPE;
    }
  }
  // (4) the workspaces declared beside their kernels (the layer-by-layer one: tests/host/workspace_main.cpp): every region on a
  //     256-byte boundary, disjoint, inside the total
  for (int precision : {(int)DRIN_PREC_F32, (int)DRIN_PREC_BF16X3, (int)DRIN_PREC_BF16X3_IF16})
    for (int b : {1, 2, 255, 256, 257, 300, 1024, 2049, 4096})
      for (int n : {1, 11, 101})
        for (int dims = 0; dims < 2; ++dims)
          for (int form = 0; form < 2; ++form) {   // gathered rows | tables with token blocks
            drin_config c;
            drin_default_config(&c);
            c.batch = b, c.num_candidates = n, c.precision = precision;
            if (dims) c.embed_dim = 64, c.image_dim = 128;
            if (form) c.num_entities = 500, c.entity_tokens = 8, c.entity_image_inner = 2;
            DRIN_TRY(fused_layout_selfcheck(c));
            if (precision != DRIN_PREC_BF16X3_IF16) {
              DRIN_TRY(cached_layout_selfcheck(c));
              DRIN_TRY(input_grad_scratch_selfcheck(c));
            }
            if (precision == DRIN_PREC_F32) {
              DRIN_TRY(melhi_layout_selfcheck(b, n, c.embed_dim, c.image_dim, form ? 128 : 7));
              DRIN_TRY(ghmfc_layout_selfcheck(b, n, c.embed_dim, c.image_dim, form ? 128 : 7, form ? 49 : 4, form ? 8 : 0));
              for (int rows = 0; rows < 2; ++rows)
                DRIN_TRY(ghmfc_table_layout_selfcheck(b, n, c.embed_dim, c.image_dim, form ? 128 : 7, form ? 49 : 4, form ? 8 : 0, rows != 0,
                                                      form ? 100000 : 9));
            }
          }
  // GHMFC's table form at its tiny test widths, the reference widths and a long candidate list
  for (int rows = 0; rows < 2; ++rows)
    for (int b : {3, 300}) {
      DRIN_TRY(ghmfc_table_layout_selfcheck(b, 4, 16, 32, 12, 3, 6, rows != 0, 9));
      DRIN_TRY(ghmfc_table_layout_selfcheck(b, 4, 16, 32, 12, 3, 0, rows != 0, 9));
      DRIN_TRY(ghmfc_table_layout_selfcheck(b, 101, 768, 2048, 128, 49, 64, rows != 0, 150));
      DRIN_TRY(ghmfc_table_layout_selfcheck(b, 1001, 768, 2048, 128, 49, 64, rows != 0, 1 << 20));
    }
  // the cosine top-k workspace (table_topk.hip): tiny, the reference width, E = 1 M at B = 4096; default and explicit chunks
  for (int k : {1, 100, 256}) {
    DRIN_TRY(table_topk_layout_selfcheck(3, 300, 16, k, 64));
    DRIN_TRY(table_topk_layout_selfcheck(3, 300, 16, k, 0));
    DRIN_TRY(table_topk_layout_selfcheck(64, 65536, 768, k, 0));
    DRIN_TRY(table_topk_layout_selfcheck(4096, 1000000, 768, k, 0));
    DRIN_TRY(table_topk_layout_selfcheck(kMaxGridY, 1000000, 768, k, 512));
  }
  // the summed-cosine workspace (TopkSumLayout): tiny, the text + CLIP widths at E = 1 M and B = 4096, four terms
  {
    const int tiny[] = {16, 8, 8}, edges[] = {768, 512, 512}, four[] = {16, 260, 4, 768};
    for (int64_t chunk : {(int64_t)0, (int64_t)64}) {
      DRIN_TRY(table_topk_sum_layout_selfcheck(tiny, 3, 3, 300, 20, chunk));
      DRIN_TRY(table_topk_sum_layout_selfcheck(tiny, 1, 1, 7, 7, chunk));
    }
    DRIN_TRY(table_topk_sum_layout_selfcheck(edges, 3, 4096, 1000000, 100, 0));
    DRIN_TRY(table_topk_sum_layout_selfcheck(edges, 3, 4096, 1000000, 100, 512));
    for (int k : {1, 100, 256}) DRIN_TRY(table_topk_sum_layout_selfcheck(four, 4, 9, 70000, k, 0));
    DRIN_TRY(table_topk_sum_layout_selfcheck(four, 4, kMaxGridY, 1000000, 256, 0));
    // bf16-stored rows: the planes of the plane route, the widened chunk of the widen route - tiny (width 16:
    // widen in either precision), the reference widths, E = 1 M at B = 4096; one term fp32 among bf16 ones; default and explicit chunks
    const int all_bf16[] = {DRIN_FEAT_BF16, DRIN_FEAT_BF16, DRIN_FEAT_BF16, DRIN_FEAT_BF16}, mixed[] = {DRIN_FEAT_BF16, DRIN_FEAT_F32, DRIN_FEAT_BF16};
    const int tiny8[] = {16, 8, 8}, wide[] = {32, 16, 16};
    for (int prec : {DRIN_PREC_F32, DRIN_PREC_BF16X3}) {
      for (int64_t chunk : {(int64_t)0, (int64_t)64}) {
        for (int k : {1, 100, 256}) DRIN_TRY(table_topk_layout_selfcheck(3, 300, 16, k, chunk, DRIN_FEAT_BF16, prec));
        DRIN_TRY(table_topk_layout_selfcheck(5, 1500, 32, 64, chunk, DRIN_FEAT_BF16, prec));
        DRIN_TRY(table_topk_sum_layout_selfcheck(tiny8, 3, 3, 300, 20, chunk, all_bf16, prec));
        DRIN_TRY(table_topk_sum_layout_selfcheck(wide, 3, 3, 300, 20, chunk, mixed, prec));
      }
      DRIN_TRY(table_topk_layout_selfcheck(64, 65536, 768, 100, 0, DRIN_FEAT_BF16, prec));
      DRIN_TRY(table_topk_layout_selfcheck(4096, 1000000, 768, 100, 0, DRIN_FEAT_BF16, prec));
      DRIN_TRY(table_topk_layout_selfcheck(4096, 1000000, 776, 100, 0, DRIN_FEAT_BF16, prec));
      DRIN_TRY(table_topk_sum_layout_selfcheck(edges, 3, 4096, 1000000, 100, 0, all_bf16, prec));
      DRIN_TRY(table_topk_sum_layout_selfcheck(edges, 3, 4096, 1000000, 100, 512, mixed, prec));
    }
  }
  // (5) for_grid_slices (internal.h), the launch loop of every sliced launcher: contiguous slices of at most kMaxGridY that cover
  //     [0, count) exactly, none for an empty count; a failing slice ends the walk and its status comes back
  for (int64_t count : {(int64_t)0, (int64_t)1, (int64_t)kMaxGridY, (int64_t)kMaxGridY + 1, 2 * (int64_t)kMaxGridY, 2 * (int64_t)kMaxGridY + 1}) {
    int64_t next = 0;
    int calls = 0;
    bool sound = true;
    const int rc = for_grid_slices(count, [&](int64_t first, int n) -> int {
      sound = sound && first == next && n >= 1 && n <= kMaxGridY && first + n <= count;
      next = first + n;
      ++calls;
      return DRIN_OK;
    });
    if (rc != DRIN_OK || !sound || next != count || calls != (int)cdiv(count, kMaxGridY)) {
      set_error("selftest: for_grid_slices(%lld): status %d, %d slices ending at %lld%s", (long long)count, rc, calls, (long long)next,
                sound ? "" : ", one of them out of order, empty or longer than the limit");
      return rc != DRIN_OK ? rc : DRIN_E_SHAPE;
    }
    calls = 0;
    const int stopped = for_grid_slices(count, [&](int64_t, int) -> int { return ++calls == 2 ? (int)DRIN_E_WORKSPACE : (int)DRIN_OK; });
    const int slices = (int)cdiv(count, kMaxGridY);
    if (stopped != (slices >= 2 ? DRIN_E_WORKSPACE : DRIN_OK) || calls != (slices < 2 ? slices : 2)) {
      set_error("selftest: for_grid_slices(%lld): a failing second slice gave status %d after %d calls", (long long)count, stopped, calls);
      return DRIN_E_SHAPE;
    }
  }
  set_error("");
  return DRIN_OK;
}

}  // extern "C"
