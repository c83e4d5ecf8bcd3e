/*
 * drin_hip.h - C ABI of libdrin_hip.so: the MI355X (gfx950) DRIN scoring path.
 *
 * The reference (starreeze/drin, /root/reference) has no FFI: its boundary for this path is the
 * Python nn.Module `drin/model.py:156-209` (`Model()` / `Model.forward(batch)`), called from
 * `train.py:27-33`.  This library sits directly underneath a drop-in replacement of that Module
 * (`drin_amd/model.py`) and is what a maintainer of the reference would bind with ctypes
 * (INTEGRATION.md).  Each entry point names the reference lines it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions across the boundary.
 *   - every function returns DRIN_OK (0) or a negative drin_status; drin_last_error() gives a
 *     thread-local message for the last failure on the calling thread.
 *   - all data pointers are DEVICE pointers unless a parameter says "host".  The caller owns every
 *     buffer, including the workspace (size from drin_workspace_bytes); the library allocates
 *     nothing and keeps no mutable global state (the opt-in profile of drin_profile_begin apart), so calls are
 *     re-entrant.
 *   - every kernel is launched on the caller's `stream` (a hipStream_t passed as void*); the
 *     library never synchronises (drin_index_status apart, which exists to be the caller's synchronisation point).
 *   - THE DEVICE OF A CALL IS THE DEVICE OF ITS STREAM, not the calling thread's current device: every launching entry
 *     point asks the stream (hipStreamGetDevice), makes that device current for the duration of the call - kernel
 *     attributes, launches, memsets and events all land there - and restores the caller's device before it returns.  With
 *     the NULL stream the device is the one that owns the call's workspace / output pointer (hipPointerGetAttributes), and
 *     THAT device's default stream is used.  A single process may therefore drive several GPUs from one thread without
 *     hipSetDevice between calls; pointers of a call must all live on the stream's device.
 *   - tensors are dense row-major fp32 (`float`), index/mask tensors int64 exactly as
 *     `drin/data.py:110-126` collates them.
 */
#ifndef DRIN_HIP_H_
#define DRIN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRIN_ABI_VERSION 12
#define DRIN_API __attribute__((visibility("default")))

typedef enum {
  DRIN_OK = 0,
  DRIN_E_SHAPE = -1,     /* a dimension is out of the supported range / inconsistent            */
  DRIN_E_NULL = -2,      /* a required pointer is NULL                                           */
  DRIN_E_ALIGN = -3,     /* a pointer or leading dimension misses the 16-byte alignment contract */
  DRIN_E_WORKSPACE = -4, /* workspace smaller than drin_workspace_bytes()                        */
  DRIN_E_HIP = -5,       /* a HIP runtime call failed (launch error, bad stream, ...)            */
  DRIN_E_UNSUPPORTED = -6, /* configuration not built (e.g. vector edge features)               */
  DRIN_E_INDEX = -7      /* drin_index_status: a candidate row index was outside [0, num_entities - 1]
                            (the reference's fancy index, drin/data.py:87-93, raises IndexError)  */
} drin_status;

/* Arithmetic of the contractions.  All other arithmetic is fp32.  Every value here is INSIDE the 1e-4 bar of the path on freshly
 * initialised and on trained weights (tests/test_gpu_round4.py, tests/test_gpu_round5.py); the values 2 and 4 (plain one-pass bf16: 5e-4;
 * one bf16 pass for the image contraction: 1.6e-4 on trained weights) were outside it and were removed with ABI 6. */
typedef enum {
  DRIN_PREC_F32 = 0,    /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32): k-ordered fmaf chain        */
  DRIN_PREC_BF16X3 = 1, /* operands split hi+lo bf16, 3 bf16 MFMAs, fp32 accumulate (~fp32): <= 2e-6 on the scores at
                           initialisation, <= 6e-6 on trained weights.  The default.                */
  DRIN_PREC_BF16X3_ALL = 3, /* BF16X3 also for the mention-sized contractions that BF16X3 leaves on
                              the fp32 kernel for latency reasons (used by the parity tests)      */
  DRIN_PREC_BF16X3_IF16 = 5 /* drin_forward_prepared only: precision BY CONTRACTION.  BF16X3 everywhere except the folded
                              entity-image contraction x_i (W_h1 W_ei)^T - 57 % of the path's FLOPs - which runs ONE pass of the
                              FP16 matrix instruction (11-bit operands).  Its result feeds only the layer-1 entity IMAGE vertex,
                              which reaches the score through mean_n(ti' ei') in the layer-2 mention vertex alone
                              (model.py:124-129,143-144; vertex graph :105): the rounding noise is averaged over the N candidates
                              before it meets the score.  fp16's range is made a non-issue by scaling: k_entity_stream writes
                              every image row as fp16(x / 2^ceil(log2 max|x|)) (exact) with the scale beside it, drin_prepare
                              the folded weight as one fp16 plane under one power-of-two scale, and the contraction multiplies
                              both back in its epilogue.  Measured at N = 101: <= 4e-6 on the scores with freshly initialised
                              weights, <= 2e-5 with trained ones (BF16X3 itself: 2e-6 / 6e-6).  Taken only for num_candidates >= 64
                              (at N = 11 the pass costs 8e-6 at initialisation but 1.2e-4 on trained weights), D = 768, R = 2048,
                              per-pair (not table-form) fp32-stored image rows and calls of at least 128 tiles of 256 x 256
                              (~11 000 pairs); every other call - bf16-stored features included: their two-pass contraction reads
                              the rows in place and writing the plane buys nothing - runs BF16X3 bit for bit.  Other entry points return
                              DRIN_E_UNSUPPORTED for it.  */
} drin_precision;

/* Geometry + switches of one forward.  Names follow common/args.py. */
typedef struct {
  int32_t batch;            /* B mentions in this call                                            */
  int32_t num_candidates;   /* N = num_candidates_model (args.py:101), answer slot included       */
  int32_t embed_dim;        /* D = bert_embed_dim = gcn_embed_dim (args.py:25,45)                 */
  int32_t image_dim;        /* R = resnet_embed_dim (args.py:52)                                  */
  int32_t mention_tokens;   /* L = tokens per mention sentence (args.py:72)                       */
  int32_t image_regions;    /* P = resnet_num_region (args.py:53)                                 */
  int32_t mention_objects;  /* Km (args.py:57)                                                    */
  int32_t entity_objects;   /* Ke (args.py:57)                                                    */
  int32_t entity_tokens;    /* T > 0: WikiMEL token-level entity text [B,N,T,D] + mask [B,N,T];
                               0: WikiDiverse pooled entity text [B,N,D] (ghmfc.py:239-249)       */
  int32_t mention_object_inner; /* size of the dim averaged at model.py:78-79 (1 in both datasets)*/
  int32_t entity_image_inner;   /* size of the dim averaged at model.py:43-44 (0 = tensor is 3-D) */
  int32_t entity_object_inner;  /* size of the dim averaged at model.py:82-83 (0 = tensor is 4-D) */
  int32_t num_layers;       /* num_gcn_layers (args.py:26)                                        */
  int32_t dynamic_edges;    /* gcn_edge_type == "dynamic" (args.py:32)                            */
  float edge_enabled[4];    /* gcn_edge_enabled for (tt, ti, it, ii) (args.py:34, model.py:122)   */
  float layer_norm_eps;     /* 1e-5  (nn.LayerNorm default, model.py:119)                         */
  float cosine_eps;         /* 1e-8  (nn.CosineSimilarity default, model.py:57,162)               */
  float miei_eps;           /* 1e-9  (model.py:92)                                                */
  float clip_scale;         /* 100   (model.py:203)                                               */
  int32_t precision;        /* drin_precision                                                     */
  int32_t num_entities;     /* rows of the entity TABLES when drin_batch.entity_index is set, else 0    */
  int32_t vector_edges;     /* gcn_edge_feature == "vector" (args.py:33): edges are [B, N, D], w_m is a Linear,
                               w_u / w_v map D -> D/2 (model.py:112-116,151-152).  Layer-by-layer path only. */
  int32_t feature_dtype;    /* drin_feature_dtype: storage type of the six FEATURE tensors of drin_batch (mention_text,
                               mention_image, mention_object, entity_text, entity_image, entity_object).  With
                               DRIN_FEAT_BF16 those pointers address bf16 arrays of the same shapes - half the bytes
                               of the HBM-bound pass; scores, similarities, masks, weights and ALL arithmetic stay
                               fp32 (a bf16 value is exact in fp32, so the result equals the reference forward on
                               the same features widened to fp32).  drin_forward_prepared only; the other paths
                               return DRIN_E_UNSUPPORTED (widen the features on the caller side). */
  int32_t vertex_activation; /* drin_activation: gcn_vertex_activation (args.py:35; model.py:117,128), default gelu    */
  int32_t edge_activation;   /* drin_activation: gcn_edge_activation   (args.py:36; model.py:118,133), default sigmoid */
  int32_t cache_format;      /* drin_cache_format: row format of the per-entity cache (drin_build_entity_cache /
                                drin_forward_cached only; every other entry point ignores it)                           */
} drin_config;

/* Row format of the per-entity precompute cache.  DRIN_CACHE_F32: every field fp32 ([5 D + R + 4] floats per entity).
 * DRIN_CACHE_MIXED_F16 ("precision by storage"): the fields that carry a vertex or the text-text edge - the two layer-1
 * entity contractions h_t, h_i and the normalised CLS row (model.py:71-76,128,146) - stay fp32; the operands of per-pair
 * SCALARS - W_v1(et0), W_v1(ei0) (the edge update: a mean over D inside a sigmoid, model.py:148-153) and the score-weighted
 * normalised object row (the image-image edge, model.py:84-92, which feeds mi' and ei' alone) - are stored as fp16 with one
 * power-of-two scale per field and row (exact to apply; the row may have any magnitude): [4 D + R / 2 + 4] floats per
 * entity, 16 400 B instead of 23 568 at D = 768, R = 2 048.  Effect on the scores: 2e-7 at N = 101, 6e-7 at N = 11
 * (oracle/precision_emulation.py; measured: tests/test_gpu_round4.py) - below the split-bf16 contractions' own 1.3e-6; with
 * TRAINED weights <= 3e-6 at N = 101 and <= 1.7e-5 at N = 11 against the fp32 rows (profiles/r4_precision_on_trained_weights.txt).
 * The limit of the format: an fp16 field holds its per-pair scalar (an edge logit, the static image-image edge) to ~1e-5, which the
 * mention aggregates mean_n(edge x vertex) (model.py:143-144) average over the N candidates.  A candidate whose image row is 1e6 times
 * the others' DOMINATES that mean, and the aggregate then inherits the error of its ONE edge: measured 1e-5 .. 7e-5 on the scores of
 * such mentions against the fp64 oracle (fp32 rows: 9e-7), reproduced to 1e-5 by the fp64 oracle with the three fields passed through
 * the format's rounding (tests/test_gpu_round5.py).  Inside the 1e-4 bar, outside the 1e-5 guard: tables with rows that far off
 * scale belong in DRIN_CACHE_F32.
 * Needs embed_dim % 8 == 0 and image_dim % 8 == 0. */
typedef enum {
  DRIN_CACHE_F32 = 0,
  DRIN_CACHE_MIXED_F16 = 1
} drin_cache_format;

/* The reference resolves `getattr(torch.nn.functional, name)` (model.py:117-118) - any function name.  Built here: the
 * five below, for the vertices AND for the edges (sigmoid, tanh and relu take their derivative from the stored output; gelu and
 * silu edges keep the pre-activation for the backward pass - Layout::edge_z; goldens tiny_wd_gelu_edge,
 * tiny_wm_silu_edge_vector).  Every entry point takes them: the layer-by-layer forward / backward and the folded
 * inference paths (whose default-activation kernels are separate instantiations, unchanged by the switch). */
typedef enum {
  DRIN_ACT_DEFAULT = 0, /* gelu for vertex_activation, sigmoid for edge_activation (a zero-initialised config is the reference's) */
  DRIN_ACT_GELU = 1,    /* exact-erf gelu (F.gelu default)                                              */
  DRIN_ACT_SIGMOID = 2,
  DRIN_ACT_RELU = 3,
  DRIN_ACT_TANH = 4,
  DRIN_ACT_SILU = 5
} drin_activation;

typedef enum {
  DRIN_FEAT_F32 = 0,
  DRIN_FEAT_BF16 = 1
} drin_feature_dtype;

/* The 14 tensors `Model.forward` unpacks (drin/model.py:165-180), device pointers.
 * mention_text_mask is carried by the reference but never read by the DRIN compute, so it is absent. */
typedef struct {
  const float* mention_text;          /* [B, L, D]                                               */
  const int64_t* mention_start;       /* [B]   already +1 for CLS (data.py:113)                  */
  const int64_t* mention_end;         /* [B]                                                     */
  const float* mention_image;         /* [B, P, R]                                               */
  const float* mention_object;        /* [B, Km, inner, R]                                       */
  const float* mention_object_score;  /* [B, Km]                                                 */
  const float* entity_text;           /* T>0: [B, N, T, D]   T==0: [B, N, D]                     */
  const int64_t* entity_text_mask;    /* T>0: [B, N, T]      T==0: ignored (may be NULL)         */
  const float* entity_image;          /* [B, N, (inner,) R]                                      */
  const float* entity_object;         /* [B, N, Ke, (inner,) R]                                  */
  const float* entity_object_score;   /* [B, N, Ke]                                              */
  const float* miet_similarity;       /* [B, N]  CLIP logits (model.py:178,203)                  */
  const float* mtei_similarity;       /* [B, N]                                                  */
  /* Optional on-device form of the WikiMEL entity-table gather (drin/data.py:87-93).  When non-NULL,
   * entity_text / entity_text_mask / entity_image / entity_object / entity_object_score are TABLES with
   * cfg.num_entities rows ([E, T, D], [E, T], [E, (inner,) R], ...) and candidate (b, n) reads row
   * entity_index[b, n] (clamped to [0, E-1] by drin_forward_prepared) instead of row b*N + n.  Taken by
   * drin_forward_prepared (token-level or pooled tables) and, for training over tables pooled ahead of time
   * (entity_tokens = 0, entity_text_cls set or not, one object per entity, inner dims <= 1, scalar edges, split-bf16
   * precision, >= 1024 pairs), by drin_forward / drin_backward: the static-edge kernels and the vertex-encoder GEMMs
   * (forward x W^T, backward dY^T x) address the table rows through the index - indices must lie in [0, E-1]. */
  const int64_t* entity_index;        /* [B, N] or NULL                                          */
  /* Optional, T == 0 only: the rows the text-text edge compares the mention span with (model.py:73-75: token 0 of
   * the WikiMEL token block) when entity_text carries token means POOLED AHEAD OF TIME - the pooling of
   * ghmfc.py:245-249 has no weights, so a training loop over an entity table can pool every entity once instead of
   * every candidate every step.  NULL: the edge reads entity_text itself (the WikiDiverse layout).
   * drin_forward / drin_backward / drin_edges_fwd; the fused inference entry points return DRIN_E_UNSUPPORTED. */
  const float* entity_text_cls;       /* [B, N, D] or NULL                                       */
  /* Optional, with entity_index: int32[4] in DEVICE memory where the kernels of drin_forward_prepared / drin_forward_cached
   * REPORT an index outside [0, num_entities - 1].  Such an index is always clamped (no out-of-bounds read whatever the
   * caller sends) - but the clamped row is another entity's, where the reference's fancy index (drin/data.py:87-93) raises.
   * The first kernel to meet one sets word 0 to 1 and leaves the pair b * N + n in word 1 and the offending value in words
   * 2 (low half) and 3 (high half); nothing else ever writes the words: STICKY - the caller zeroes them once and reads them
   * wherever it synchronises anyway, or through drin_index_status.  NULL: clamp silently.  (The table form of drin_forward /
   * drin_backward reads rows through the index without clamping: indices must be valid there, see entity_index.) */
  int32_t* index_status;              /* [4] or NULL                                             */
} drin_batch;

/* One GCNLayer's parameters (drin/model.py:109-119); nn.Linear layout weight[out][in]. */
typedef struct {
  const float *w_h, *b_h, *w_u, *b_u, *w_v, *b_v, *ln_weight, *ln_bias;
  const float *w_m, *b_m; /* vector edges only (model.py:112): [D, D], [D]; then w_u / w_v are [D/2, D] */
} drin_layer_params;

#define DRIN_MAX_LAYERS 8

/* The 24 state_dict tensors. */
typedef struct {
  const float *w_mention_text, *b_mention_text;   /* vertex_encoder.mention_text_encoder.final_layer.linear */
  const float *w_entity_text, *b_entity_text;     /* vertex_encoder.entity_text_encoder.final_layer         */
  const float *w_mention_image, *b_mention_image; /* vertex_encoder.mention_image_linear  [D, R]            */
  const float *w_entity_image, *b_entity_image;   /* vertex_encoder.entity_image_linear   [D, R]            */
  drin_layer_params layer[DRIN_MAX_LAYERS];
} drin_params;

/* Gradients w.r.t. the same tensors; every non-NULL pointer is ACCUMULATED into (+=), so the caller
 * zeroes them (torch .grad semantics).  Parameters the output does not depend on (last layer's
 * w_u / w_v, model.py:130-134) are left untouched. */
typedef struct {
  float *w_mention_text, *b_mention_text, *w_entity_text, *b_entity_text;
  float *w_mention_image, *b_mention_image, *w_entity_image, *b_entity_image;
  struct { float *w_h, *b_h, *w_u, *b_u, *w_v, *b_v, *ln_weight, *ln_bias, *w_m, *b_m; } layer[DRIN_MAX_LAYERS];
} drin_param_grads;

/* Gradients w.r.t. the floating-point batch tensors (drin_backward_ex): what autograd gives every float tensor of the
 * reference's 14-item batch, since its Model.forward is plain torch (drin/model.py:164-209).  Each output has the shape of its
 * drin_batch counterpart (inner dims, the [B, N, T, D] token block when entity_tokens > 0, pooled [B, N, D] text plus
 * entity_text_cls in the pooled-ahead form), is fp32, 16-byte aligned and WRITTEN (not accumulated).  A NULL output is not
 * wanted and nothing is computed for it.  `scratch` (device, 16-byte aligned): drin_input_grad_scratch_bytes(cfg) bytes,
 * used only while the call runs. */
typedef struct {
  float *mention_text, *mention_image, *mention_object, *mention_object_score;
  float *entity_text, *entity_text_cls, *entity_image, *entity_object, *entity_object_score;
  float *miet_similarity, *mtei_similarity;
  void* scratch;
  size_t scratch_bytes;
} drin_input_grads;

/* Optional taps of intermediate values for tests/debugging (any pointer may be NULL).
 * Index l = 0 is the VertexEncoder/EdgeEncoder output, l >= 1 the output of GCN layer l. */
typedef struct {
  float* mention_text_vertex[DRIN_MAX_LAYERS + 1];  /* [B, D]    */
  float* mention_image_vertex[DRIN_MAX_LAYERS + 1]; /* [B, D]    */
  float* entity_text_vertex[DRIN_MAX_LAYERS + 1];   /* [B, N, D] */
  float* entity_image_vertex[DRIN_MAX_LAYERS + 1];  /* [B, N, D] */
  float* edges[DRIN_MAX_LAYERS + 1];                /* [4, B, N] ([4, B, N, D] with vector edges) order tt, ti, it, ii */
} drin_trace;

/* ---- housekeeping ------------------------------------------------------------------------- */
DRIN_API int drin_version(void);                 /* DRIN_ABI_VERSION the library was built with           */
DRIN_API const char* drin_last_error(void);      /* thread-local, never NULL                              */
DRIN_API const char* drin_build_info(void);      /* "gfx950 <compiler> <date>"                            */

/* Fills `cfg` with the reference defaults (eps values, scale, all edges enabled, 2 dynamic layers,
 * WikiDiverse geometry).  Replaces the import-time globals of common/args.py. */
DRIN_API int drin_default_config(drin_config* cfg);

/* Host-side self-checks of the library's launch-sequencing code, for the sanitizer build and CI: no kernel is launched,
 * no GPU is needed.  Checks that the workspace layout gives the mention-sized weight-gradient group of drin_backward
 * (train.py:33-34 through model.py:164-209) its worst-case slice scratch at every batch size, and that the grouped GEMM
 * launchers refuse an item with an empty reduction (DRIN_E_SHAPE) instead of dividing by a slice length derived from it.
 * DRIN_OK, or the first failing check's status with its message in drin_last_error().  No reference counterpart. */
DRIN_API int drin_host_selftest(void);

/* Bytes of device workspace drin_forward / drin_backward need for `cfg` (0 on error). */
DRIN_API size_t drin_workspace_bytes(const drin_config* cfg, int for_training);

/* ---- the path ----------------------------------------------------------------------------- */

/* Parameter-free edge builder: EdgeEncoder.forward (drin/model.py:60-94) + edge assembly
 * (model.py:201-204).  Writes edges[4][B][N] in order (tt, ti, it, ii) and, if non-NULL, the
 * span mean of the mention text [B, D] (ghmfc.py:54-60), which the vertex encoder reuses. */
DRIN_API int drin_edges_fwd(const drin_config* cfg, const drin_batch* batch, float* edges, float* span_mean,
                   void* stream);

/* Input pooling of VertexEncoder.forward: entity token mean (ghmfc.py:245-249, only T>0),
 * mention region mean (model.py:41), entity image inner mean (model.py:43-44).  Any output may be
 * NULL to skip it.  pooled_entity_text [B,N,D], pooled_mention_image [B,R], pooled_entity_image [B,N,R].
 * Only the inputs of the requested outputs are read (pooling an entity TABLE once passes the text and its mask alone).
 * With cfg.feature_dtype == DRIN_FEAT_BF16 the entity token pooling reads bf16 tokens in place (fp32 sums of the
 * exactly widened values); the two image means are then not available here (DRIN_E_UNSUPPORTED). */
DRIN_API int drin_pool_fwd(const drin_config* cfg, const drin_batch* batch, float* pooled_entity_text,
                  float* pooled_mention_image, float* pooled_entity_image, void* stream);

/* y[m, n] = sum_k x[m, k] * w[n, k] + bias[n]   (nn.Linear, weight [n_out][k]); bias may be NULL.
 * The building block behind every Linear of the path (ghmfc.py:69,250; model.py:42,45,128,150-153). */
DRIN_API int drin_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t rows,
                    int32_t n_out, int32_t k, int32_t precision, void* stream);

/* Backward of the same Linear (what autograd does for every nn.Linear of the path under train.py:33-34):
 *   dx[m, k]  = sum_n dy[m, n] w[n, k]      (written; dx may be NULL)
 *   dw[n, k] += sum_m dy[m, n] x[m, k]      (accumulated; dw may be NULL)
 *   db[n]    += sum_m dy[m, n]              (accumulated; db may be NULL)
 * `scratch` (`scratch_floats` floats, may be NULL / 0): n_out * k floats hold the transposed weight the split-bf16 dx
 * product runs against (without them dx stays on the exact fp32 kernel); with at least 28 * n_out * k floats the
 * split-bf16 dw product stores its reduction slices there and adds them in order (bit-reproducible) instead of
 * using fp32 atomics, and a partly filled last round of 256 x 256 output tiles of the dx product is split along the
 * reduction over the idle CUs (partial tiles in the scratch behind the transposed weight, added in order).
 * Small problems take the exact fp32 kernels in every precision. */
DRIN_API int drin_linear_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                             int64_t rows, int32_t n_out, int32_t k, int32_t precision, float* scratch,
                             size_t scratch_floats, void* stream);

/* Model.forward (drin/model.py:164-209): scores[B, N] = cos(mt'', et'').
 * `keep_for_backward` != 0 lays the intermediates backward needs out in `workspace`, which must
 * then stay untouched until drin_backward returns.  `trace` may be NULL.
 *
 * Sizes: batch * num_candidates <= 2^30.  A call of the layer-by-layer entry points (drin_forward, drin_forward_staged[_head],
 * drin_backward, drin_backward_staged, drin_backward_ex, drin_backward_head) either returns DRIN_OK with the right values or
 * is refused among its argument checks, BEFORE its first launch: scores, gradients and workspace are then untouched.  More than
 * 65 535 mentions in one call run (the per-mention launches are cut into slices of 65 535 mentions, the one-wave-per-pair
 * kernels take a flat grid) with two exceptions, both DRIN_E_SHAPE ("split the batch"):
 *   - drin_backward* with vector edges whose update is live (dynamic edges, two or more layers) above 65 535 mentions;
 *   - a call one of whose products has more than 65 535 * 128 rows and runs exact fp32: every product under DRIN_PREC_F32, under
 *     split-bf16 those whose reduction length is no multiple of 32.  With M = batch * num_candidates the products have M rows
 *     (the entity encoders, over embed_dim and image_dim), 2 M (the layers' W_h and W_v over both entity vertex types, over
 *     embed_dim; M in a single untraced layer) and, with live vector-edge updates, 4 M (W_m, over embed_dim) and in the backward
 *     2 M over embed_dim / 2. */
DRIN_API int drin_forward(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                 void* workspace, size_t workspace_bytes, float* scores, int keep_for_backward,
                 const drin_trace* trace, void* stream);

/* DRIN_OK when drin_forward / drin_forward_staged / drin_backward* take `cfg` in table form (drin_batch.entity_index over
 * tables of cfg.num_entities rows, entity text pooled ahead of time); DRIN_E_UNSUPPORTED (drin_last_error says what the
 * table form needs): gather the rows on the caller side.  Host-only, like drin_fused_supported; the entry points apply
 * the same predicate. */
DRIN_API int drin_indexed_supported(const drin_config* cfg);

/* drin_forward for a training loop that runs the previous step's gradient all-reduce and optimiser update on ANOTHER
 * stream (the reference runs one device, train.py:117-118, and has no counterpart).  `params_ready_event`: a
 * hipEvent_t recorded on that stream behind the update, or NULL (= drin_forward).  The parameter-free head of the pass - the
 * pooling kernels and the static edges (ghmfc.py:54-60,245-249; model.py:41-45,60-94), which read the batch alone: 0.2 of
 * the 1.35 ms of a WikiMEL step at batch 64 - is enqueued first; `stream` then waits for the event (hipStreamWaitEvent)
 * before the first launch that reads `params`.  Same kernels, same results as drin_forward. */
DRIN_API int drin_forward_staged(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                 void* workspace, size_t workspace_bytes, float* scores, int keep_for_backward,
                 const drin_trace* trace, void* params_ready_event, void* stream);

/* Backward of drin_forward: given grad_scores[B, N], accumulates parameter gradients into `grads`
 * (loss.backward() of train.py:33-34 through model.py:164-209).  drin_backward_ex adds the gradients of the batch
 * tensors. */
DRIN_API int drin_backward(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                  void* workspace, size_t workspace_bytes, const float* grad_scores,
                  const drin_param_grads* grads, void* stream);

/* drin_backward in two stages for a data-parallel caller (the reference runs one device, train.py:117-118,
 * and has no counterpart).  `layers_ready_event`: a hipEvent_t the caller created, or NULL (= drin_backward).  The event
 * is recorded on `stream` once every gradient of the GCN layers (the `layer[l]` tensors of `grads`) is complete; only
 * the four vertex encoders' gradients (w_/b_ mention_text, entity_text, mention_image, entity_image) are written after
 * it.  A caller whose gradient bucket keeps the two groups apart starts the all-reduce of the layers' part behind the
 * event, under the vertex encoders' weight-gradient products.  The two parts deal the chip's workgroups separately, so the
 * pair-sized weight gradients differ from drin_backward's in the last bits (another split of the same sums; no atomics:
 * each entry point reproduces its own bits run after run) and the pass costs two part-filled launches more - measure
 * before preferring it to drin_forward_staged, which hides the collective without touching the backward pass. */
DRIN_API int drin_backward_staged(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                  void* workspace, size_t workspace_bytes, const float* grad_scores,
                  const drin_param_grads* grads, void* layers_ready_event, void* stream);

/* drin_backward_staged with input gradients: the one backward entry point the two above call (input_grads = NULL), with
 * their launches and results.  `grads` may be NULL: no weight-gradient product runs (frozen-model attribution: gradient x
 * input, or training something upstream of the model).  `input_grads` may be NULL (= drin_backward_staged); else the
 * gradients of the batch tensors are written after every parameter gradient, from the vertex-encoder output gradients and
 * the layer-0 edge gradients the pass computes anyway: the Linear dX products (the two pair-sized ones - entity image
 * [B N, D] x [D, R], entity text - in split-bf16 against transposed weight planes when the precision is split-bf16, exact
 * fp32 otherwise), the span / token / axis mean backward, the text-text cosine, the image-image edge (model.py:78-92), the
 * CLIP edges (/ clip_scale, model.py:203) and the edge_enabled mask (model.py:122).  Not with entity_index (gather the
 * rows: DRIN_E_UNSUPPORTED), and at most 64 object pairs (mention_objects x entity_objects). */
DRIN_API int drin_backward_ex(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                              void* workspace, size_t workspace_bytes, const float* grad_scores,
                              const drin_param_grads* grads, const drin_input_grads* input_grads,
                              void* layers_ready_event, void* stream);
/* Bytes of drin_input_grads.scratch for `cfg` (0 on error). */
DRIN_API size_t drin_input_grad_scratch_bytes(const drin_config* cfg);

/* Backward of drin_pool_fwd's entity token mean (ghmfc.py:245-249) plus the token-0 row the text-text edge reads
 * (model.py:73-75): from the pooled gradient grad_pooled [B, N, D], the token-0 gradient grad_cls [B, N, D] (NULL: zero) and
 * entity_text_mask [B, N, T], WRITES the whole token-block gradient [B, N, T, D] (T = cfg.entity_tokens): token 0 gets
 * grad_cls, tokens 1 .. ntok - 2 grad_pooled / (ntok - 2) (ntok = 0: tokens 1 .. T - 2, the slice's -1 stop), every other
 * token 0.  Stored as fp32 or, with cfg.feature_dtype == DRIN_FEAT_BF16, bf16 (embed_dim % 8 == 0). */
DRIN_API int drin_pool_bwd(const drin_config* cfg, const int64_t* entity_text_mask, const float* grad_pooled,
                           const float* grad_cls, void* grad_entity_text, void* stream);

/* ---- which width form a configuration takes (additive under ABI 12) -------------------------------
 * The width-templated row kernels of the folded and cached inference paths, and the LayerNorm backward of training, are built
 * in a few forms per family, chosen from the widths alone: `tiny` (embed_dim and - where the family reads image rows -
 * image_dim up to 256: one 16-byte quad per lane and register slot), `exact` (768 / 2048: every lane of every slot full, the
 * widths compile-time constants) and `guarded` (anything between: the exact form's slots behind column guards, so that part of
 * the lanes, or whole slots, hold nothing).  drin_width_class answers with the form the family's launcher takes for `cfg` - the
 * launchers switch on the same host function - so that a caller, or a test, asks instead of restating the gates.
 * Returns a drin_width_band (>= 0), or a negative drin_status for a NULL / invalid config or an unknown family.
 * DRIN_WIDTH_NOT_BUILT where the family does not run for `cfg`: a geometry drin_fused_supported refuses (every family but the
 * LayerNorm backward), DRIN_WIDTH_FAMILY_CACHE_PACK with cfg.cache_format == DRIN_CACHE_F32 (fp32 rows are not packed), the
 * cache families with DRIN_CACHE_MIXED_F16 at a width that is no multiple of 8.
 * DRIN_WIDTH_FAMILY_LN_BACKWARD returns V = ceil(embed_dim / 256) in 1 .. 4 instead: the register slots of
 * k_layernorm_gelu_bwd<V> (the training path, any validated width). Host-only. */
typedef enum {
  DRIN_WIDTH_NOT_BUILT = 0,
  DRIN_WIDTH_TINY = 1,
  DRIN_WIDTH_GUARDED = 2,
  DRIN_WIDTH_EXACT = 3
} drin_width_band;
typedef enum {
  DRIN_WIDTH_FAMILY_ENTITY_STREAM = 0, /* k_entity_stream (drin_forward_prepared)                                            */
  DRIN_WIDTH_FAMILY_PAIR_ROWS = 1,     /* k_pair_layer1, k_pair_final: embed_dim and cfg.vertex_activation (a non-default one
                                          has no exact form: guarded at 768)                                                 */
  DRIN_WIDTH_FAMILY_CACHE_ROWS = 2,    /* k_entity_cache_rows (drin_build_entity_cache); one guarded kernel serves 768 / 2048
                                          too, where the answer is still `exact`                                              */
  DRIN_WIDTH_FAMILY_CACHE_PACK = 3,    /* k_cache_pack_mixed: embed_dim alone; the same remark                                */
  DRIN_WIDTH_FAMILY_CACHED_PAIRS = 4,  /* k_cached_pairs (drin_forward_cached): cfg.cache_format (mixed rows are tiny up to
                                          image_dim 512) and cfg.vertex_activation                                           */
  DRIN_WIDTH_FAMILY_LN_BACKWARD = 5    /* k_layernorm_gelu_bwd<V>: returns V                                                  */
} drin_width_family;
DRIN_API int drin_width_class(const drin_config* cfg, int family);

/* ---- fused two-layer inference path ------------------------------------------------------------
 * Same result as drin_forward (fp32 re-association only) for the default geometry num_layers == 2,
 * with the weight-only products folded once per weight version (csrc/fused_forward.hip):
 *   drin_prepare           folds the weights into `prepared` (drin_prepared_bytes; caller-owned, reusable
 *                          for every batch until a parameter changes)
 *   drin_forward_prepared  Model.forward (drin/model.py:164-209) without autograd state
 * drin_fused_supported returns DRIN_OK when `cfg` can take this path (else use drin_forward).
 * drin_forward_prepared and drin_forward_cached take at most 65 535 mentions per call and refuse more (DRIN_E_SHAPE) among their
 * argument checks, before the first launch. */
DRIN_API int drin_fused_supported(const drin_config* cfg);
DRIN_API size_t drin_prepared_bytes(const drin_config* cfg);
DRIN_API size_t drin_fused_workspace_bytes(const drin_config* cfg);
DRIN_API int drin_prepare(const drin_config* cfg, const drin_params* params, void* prepared, size_t prepared_bytes,
                          void* stream);
DRIN_API int drin_forward_prepared(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                                   const void* prepared, void* workspace, size_t workspace_bytes, float* scores,
                                   void* stream);
/* How the row-streaming kernels of the two folded paths divide a mention's candidate list for THIS call size: the number of
 * workgroups (candidate chunks) per mention of k_entity_stream / k_pair_layer1 / k_pair_final (cached == 0:
 * drin_forward_prepared - 16 candidates per workgroup, 48 from 1 024 mentions, the whole list up to 128 from 2 048) or of
 * k_cached_pairs (cached != 0: drin_forward_cached - 64 candidates, 128 from 2 048 mentions; 16 off the exact widths).  The
 * per-mention sums are grouped by these chunks, so a mention's scores in calls of different sizes agree to fp32
 * re-association only (<= 5e-6 measured), and are the same bits every run within one call size.  Introspection for
 * tests and benchmarks (which instantiation did this call take?); 0 when cfg is off the folded paths.  No reference
 * counterpart. */
DRIN_API int32_t drin_workgroups_per_mention(const drin_config* cfg, int32_t cached);

/* How drin_forward_prepared evaluates the folded entity-image contraction x_i (W_h1 W_ei)^T - 57 % of the path's FLOPs - for this
 * configuration (`indexed`: drin_batch.entity_index is set): 0 = the exact fp32 kernel (DRIN_PREC_F32), else the number of
 * bf16 / fp16 MFMA passes: 3 (split-bf16), 2 (bf16-stored image rows are exact in their hi plane), 1 (DRIN_PREC_BF16X3_IF16 where its
 * gate holds: see drin_precision).  The library's own gate, for callers that account executed FLOPs (bench.py). */
DRIN_API int32_t drin_image_contraction_passes(const drin_config* cfg, int32_t indexed);

/* How an EAGER drin_forward_prepared call schedules that contraction (`indexed` as above): the number of its 256-row tiles that run
 * as a few persistent workgroups on the library's own side stream, under the entity stream pass, before the caller's stream takes
 * the rest at full grid; 0 = one launch on the caller's stream (always so for indexed rows, DRIN_PREC_F32, the one-pass fp16
 * contraction, small calls, and for a call made under stream capture, whatever this returns).  The scores are the same bits either
 * way.  The library owns one non-blocking side stream per device for this, created by the first call that uses it. */
DRIN_API int32_t drin_image_contraction_side_tiles(const drin_config* cfg, int32_t indexed);

/* The caller-side check of drin_batch.index_status: waits for `stream` (the ONE entry point that synchronises: it exists to be
 * the point where the caller would synchronise anyway), copies the four words to the host and returns DRIN_OK, or
 * DRIN_E_INDEX with the pair and the value in drin_last_error() - what drin/data.py:87-93 reports as an IndexError - after
 * zeroing the words again.  `index_status` is the device pointer given in drin_batch. */
DRIN_API int drin_index_status(int32_t* index_status, void* stream);

/* ---- per-entity precompute cache for table-form inference ---------------------- *
 * With frozen weights, what the first GCN layer takes from an entity (its rows of the entity_* tables,
 * `drin/data.py:87-93`) does not depend on the mention: `W_h1 W_et x_t`, `W_h1 W_ei x_i`, `W_v1(et0)`,
 * `W_v1(ei0)`, the normalised CLS row and the score-weighted normalised object row are computed ONCE per
 * entity and weight version into `cache` ([num_entities][5 D + R + 4] fp32; cfg.cache_format = DRIN_CACHE_MIXED_F16:
 * [num_entities][4 D + R / 2 + 4] floats of fp32 and scaled-fp16 fields, see drin_cache_format).  drin_forward_cached then
 * scores table-form batches (drin_batch.entity_index + the mention-side tensors + the two similarity
 * matrices; the entity_* pointers are not read) with one gathered pass over cache rows and the layer-2
 * contraction - same scores as drin_forward_prepared to fp32 re-association.  `cfg.num_entities` = table
 * rows; `prepared` = the drin_prepare buffer of the same weights.  `tables`: a drin_batch whose entity_*
 * fields point at the tables (other fields unused). */
DRIN_API size_t drin_entity_cache_bytes(const drin_config* cfg);
DRIN_API size_t drin_entity_cache_build_workspace_bytes(const drin_config* cfg);
DRIN_API size_t drin_cached_workspace_bytes(const drin_config* cfg);
DRIN_API int drin_build_entity_cache(const drin_config* cfg, const drin_batch* tables, const drin_params* params,
                                     const void* prepared, void* cache, size_t cache_bytes, void* workspace,
                                     size_t workspace_bytes, void* stream);
DRIN_API int drin_forward_cached(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                                 const void* prepared, const void* cache, void* workspace, size_t workspace_bytes,
                                 float* scores, void* stream);

/* Building blocks of the split-bf16 precision: x = hi + lo with hi, lo bf16 planes (n % 4 == 0), and the
 * contraction y = x w^T (+ bias) on such planes by LDS-DMA + bf16 MFMA (k % 32 == 0).  Plane pointers are
 * device pointers to bf16 arrays with the row strides of the fp32 originals.  x_lo may be NULL when x is
 * exact in bf16 (then two MFMAs per tile pair instead of three); the weight planes are both required. */
DRIN_API int drin_split_planes(const float* x, void* hi, void* lo, int64_t n, void* stream);
DRIN_API int drin_linear_planes_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo,
                                    const float* bias, float* y, int64_t rows, int32_t n_out, int32_t k,
                                    void* stream);

/* ---- test and tuning entry into the GEMM module ------------------------------------------------ *
 * drin_gemm_probe calls ONE of the module's internal NT launchers (y = x w^T (+ bias)) with caller-chosen arguments - leading
 * dimensions, bias or NULL, accumulate, scratch, weight planes, indexed rows, a slice of row tiles - and reports which kernel
 * form the module's own dispatch code chose for them.  It exists so that every form behind a size gate can be compared with a
 * high-precision product on its own (tests/test_gpu_gemm_forms.py) and so that a gate can be tuned from outside; no product
 * code calls it, and nothing but `struct_size` is promised about it: the struct may change with any version of the library
 * (a caller built against another layout gets DRIN_E_SHAPE).  Pointers are device pointers unless said otherwise. */
enum drin_gemm_probe_op {
  DRIN_PROBE_GEMM_NT = 1,        /* launch_gemm_nt: a fp32 [rows][lda], b fp32 [n_out][ldb]; b_hi: NULL or the weight planes
                                    ([n_out][k] bf16 hi followed by [n_out][k] bf16 lo); precision; scratch = the split scratch */
  DRIN_PROBE_GEMM_NT_BF16X3 = 2, /* launch_gemm_nt_bf16x3: a fp32; b fp32 or (b_hi, b_lo) bf16 planes of row stride ldb;
                                    accumulate; a_index; scratch = the tail-split scratch */
  DRIN_PROBE_GEMM_NT_BF16X3_P4 = 3, /* launch_gemm_nt_bf16x3_p4: a fp32, (b_hi, b_lo); accumulate; scratch; row tiles */
  DRIN_PROBE_GEMM_X3_PLANES = 4, /* launch_gemm_x3_planes: (a, a_lo or NULL) and (b_hi, b_lo) bf16 planes; scratch; row tiles */
  DRIN_PROBE_GEMM_F16_PLANES = 5,/* launch_gemm_f16_planes: a, b_hi single fp16 planes; row_scale [rows], b_scale [1]; scratch */
  DRIN_PROBE_TO_F16_SCALED = 6   /* launch_to_f16_scaled: a fp32 [rows] (rows = element count, % 4) -> y fp16 [rows] under one
                                    power-of-two scale, written to scratch[0] (scratch: two floats) */
};
enum drin_gemm_family {            /* drin_gemm_route.family */
  DRIN_GEMM_FAMILY_NONE = 0,       /* nothing was launched */
  DRIN_GEMM_FAMILY_BF16X3 = 1,     /* k_gemm_bf16x3<bm, bn, ., ., w_planes>: fp32 activation split while staged */
  DRIN_GEMM_FAMILY_BF16X3_P4 = 2,  /* k_gemm_bf16x3_p4<persist>: fp32 activation on weight planes, four-phase pipeline */
  DRIN_GEMM_FAMILY_PLANES = 3,     /* k_gemm_x3_planes<a_lo, true>: both operands as planes, two-phase kernel */
  DRIN_GEMM_FAMILY_PLANES_P4 = 4,  /* k_gemm_x3_planes_p4<a_lo, f16, persist> */
  DRIN_GEMM_FAMILY_F32 = 5,        /* k_gemm_f32<bm, bn>: exact fp32 */
  DRIN_GEMM_FAMILY_F32_GEMV = 6    /* k_gemv_rows: exact fp32, a handful of rows */
};
typedef struct drin_gemm_route {   /* filled by the dispatch code next to the launch of the product's GEMM kernel */
  int32_t launches;                /* GEMM kernels launched by the call (tail add and split-K reduction not counted) */
  int32_t family;                  /* drin_gemm_family of the last one */
  int32_t bm, bn;                  /* tile */
  int32_t w_planes, a_lo, f16, persist, indexed, accumulate;   /* 0 / 1 */
  int32_t ksplit;                  /* K-slices per tile of the tail split carried by this launch (1: none) */
  int32_t splits;                  /* split K over grid z into the scratch + ordered reduction (1: none) */
  int64_t tiles;                   /* output tiles of the whole product */
  int64_t whole_tiles;             /* tiles this launch computes whole, i.e. not as K-slices */
  int64_t tile0;                   /* its first tile in the product's tile sequence */
  int64_t work_items;              /* its grid */
} drin_gemm_route;
typedef struct drin_gemm_probe_args {
  size_t struct_size;              /* sizeof(drin_gemm_probe_args) */
  int32_t op;                      /* drin_gemm_probe_op */
  int32_t precision;               /* drin_precision (DRIN_PROBE_GEMM_NT) */
  int32_t accumulate;              /* y += instead of y = */
  int32_t row_tile_wgs;            /* RowTiles: > 0 = that many persistent workgroups walk the slice */
  int64_t row_tile_begin, row_tile_end;   /* RowTiles: 256-row tiles [begin, end) of the product; end < 0: to the last one */
  const void* a;
  const void* a_lo;
  int64_t lda;
  const void* b;
  const void* b_hi;
  const void* b_lo;
  int64_t ldb;
  const float* bias;               /* [n_out] or NULL */
  void* y;
  int64_t ldy;
  int64_t rows;
  int32_t n_out, k;
  float* scratch;                  /* or NULL */
  size_t scratch_floats;
  const int64_t* a_index;          /* [rows] or NULL: row m of the activation is row a_index[m] of the table `a` (not range-checked) */
  const float* row_scale;
  const float* b_scale;
  drin_gemm_route route;           /* out (host memory, like the struct itself) */
} drin_gemm_probe_args;
/* DRIN_E_NULL / DRIN_E_SHAPE / DRIN_E_UNSUPPORTED from the host checks (NULL struct or required operand, struct_size, negative
 * shape, a leading dimension below its row, unknown op), else whatever the launcher returns; `route` is filled either way. */
DRIN_API int drin_gemm_probe(drin_gemm_probe_args* args, void* stream);

/* drin_wgrad_probe: the same standing for the BACKWARD products - dW (+)= dY^T X, db (+)= column sums of dY, dX (+)= dY W.  It calls
 * ONE of the module's internal launchers (or a whole WeightGradPass) on up to DRIN_WGRAD_PROBE_MAX caller-chosen products and reports
 * what the module's dispatch code did with each (tests/test_gpu_wgrad_forms.py).  No product code calls it; nothing but
 * `struct_size` is promised about it. */
enum drin_wgrad_probe_op {
  DRIN_WGRAD_TN_GROUP = 1,     /* TnGroup::add per product (db = its colsum argument), launch_gemm_tn_group */
  DRIN_WGRAD_TN_F32_GROUP = 2, /* F32GemmGroup::add_tn per product, launch_gemm_tn_f32_group */
  DRIN_WGRAD_TN = 3,           /* launch_gemm_tn on product[0]; precision */
  DRIN_WGRAD_COLSUM_BATCH = 4, /* ColsumBatch::add(dy, db, rows, n_out) per product, launch_colsum_batch */
  DRIN_WGRAD_PASS = 5,         /* a WeightGradPass (precision) whose three scratch parts are carved from `scratch` - tn_group_floats of
                                  the largest n_out x k and n_out, colsum_batch_floats of the largest n_out, then small_tn_slices x
                                  n_out x k per product: DRIN_E_WORKSPACE if that does not fit; add per product, layers_done() after
                                  product[layers_done_after], finish(NULL) or, staged, finish(an event made and destroyed here) */
  DRIN_WGRAD_NN = 6            /* launch_gemm_nn on product[0]: dw [rows][k] (+)= dy [rows][n_out] x [n_out][k]; precision, accumulate,
                                  wt_form, wt; scratch = the split-K scratch */
};
enum drin_wgrad_kernel {           /* drin_wgrad_product_route.kernel */
  DRIN_WGRAD_KERNEL_NONE = 0,      /* no GEMM kernel ran for this product */
  DRIN_WGRAD_KERNEL_TN_BF16X3 = 1, /* k_gemm_tn_bf16x3: split-bf16, 256 x 256 tiles */
  DRIN_WGRAD_KERNEL_TN_F32_SMALL = 2, /* exact fp32, 64 x 64 tiles (k_gemm_f32_group<true, true> / k_gemm_f32<64, 64, true, true>) */
  DRIN_WGRAD_KERNEL_TN_F32_LARGE = 3  /* exact fp32, 128 x 128 tiles */
};
enum drin_wgrad_wt_form { DRIN_WGRAD_WT_NONE = 0, DRIN_WGRAD_WT_F32_SCRATCH = 1, DRIN_WGRAD_WT_PLANES = 2 };
#define DRIN_WGRAD_PROBE_MAX 16
#define DRIN_WGRAD_ROUTE_LAUNCHES 8
typedef struct drin_wgrad_product {
  const float* dy;                 /* [rows][lddy], n_out columns used (DRIN_WGRAD_NN: the activation gradient) */
  int64_t lddy;
  const float* x;                  /* [rows][ldx] or the table, k columns used (DRIN_WGRAD_NN: the weight [n_out][ldx]) */
  int64_t ldx;
  const int64_t* x_index;          /* or NULL: reduction row m of x is row x_index[m] of the table (not range-checked) */
  float* dw;                       /* [n_out][lddw] += (DRIN_WGRAD_NN: dX [rows][lddw]); NULL where the op allows it */
  int64_t lddw;
  float* db;                       /* [n_out] += or NULL */
  int64_t rows;
  int32_t n_out, k;
} drin_wgrad_product;
typedef struct drin_wgrad_product_route {   /* filled by the dispatch code next to the launch that carries the product */
  int32_t kernel;                  /* drin_wgrad_kernel */
  int32_t slices;                  /* slices of the reduction over the rows */
  int32_t in_place;                /* 1: added to dw by the GEMM kernel itself; 0: slices stored, added by the slice sum */
  int32_t db_rode;                 /* 1: the column sums of dy were taken by the split-bf16 TN kernel from the rows it stages */
  int32_t db_slices;               /* the column-sum kernel's row slices (0: no column-sum kernel ran for this product) */
  int32_t launch;                  /* which of the call's GEMM launches carried it (0-based) */
  int64_t rows_per_slice;
} drin_wgrad_product_route;
typedef struct drin_wgrad_route {
  int32_t gemm_launches;           /* GEMM kernels launched by the call */
  int32_t colsum_launches;         /* k_colsum_batch launches */
  int32_t sum_launches;            /* slice-sum kernels (k_slice_sum); the split-K reduction of launch_gemm_tn is counted in reduce_launches */
  int32_t reduce_launches;
  int32_t sum_dsts, sum_segs;      /* destinations and segments over all slice-sum launches */
  int32_t nn_family;               /* DRIN_WGRAD_NN: drin_gemm_family, tile, split K, W^T form taken, accumulate */
  int32_t nn_bm, nn_bn, nn_splits, nn_wt_form, nn_accumulate;
  int64_t grid[DRIN_WGRAD_ROUTE_LAUNCHES];   /* workgroups of each GEMM launch, in order (the first DRIN_WGRAD_ROUTE_LAUNCHES) */
  drin_wgrad_product_route product[DRIN_WGRAD_PROBE_MAX];
} drin_wgrad_route;
typedef struct drin_wgrad_probe_args {
  size_t struct_size;              /* sizeof(drin_wgrad_probe_args) */
  int32_t op;                      /* drin_wgrad_probe_op */
  int32_t precision;               /* drin_precision (TN, PASS, NN) */
  int32_t staged;                  /* PASS: finish(event) instead of finish(NULL) */
  int32_t n_products;              /* 1 .. DRIN_WGRAD_PROBE_MAX */
  int32_t layers_done_after;       /* PASS: layers_done() after this product; < 0: never */
  int32_t accumulate;              /* NN */
  int32_t wt_form;                 /* NN: drin_wgrad_wt_form */
  int32_t reserved;
  float* scratch;                  /* or NULL */
  size_t scratch_floats;
  float* wt;                       /* NN with a wt_form: n_out x k floats of caller memory for W^T (fp32, or its bf16 hi / lo planes,
                                      written here by launch_transpose_split_batch before the product) */
  size_t wt_floats;
  drin_wgrad_product product[DRIN_WGRAD_PROBE_MAX];
  drin_wgrad_route route;          /* out (host memory, like the struct itself) */
} drin_wgrad_probe_args;
/* DRIN_E_NULL / DRIN_E_SHAPE / DRIN_E_UNSUPPORTED from the host checks (NULL struct or operand, struct_size, negative shape, a leading
 * dimension below its row, more than DRIN_WGRAD_PROBE_MAX products, unknown op), else what the launcher returns; `route` is filled either way - zeroed by a refused call - except under
 * another `struct_size`, where the struct is of an unknown layout and nothing in it is written. */
DRIN_API int drin_wgrad_probe(drin_wgrad_probe_args* args, void* stream);

/* ---- caller-side loss and metric of one batch --------------------------------- *
 * Replaces, for scores already on the device, `TripletLoss.forward` (common/utils.py:26-43, called at
 * train.py:34) and `TopkAccuracy.update` (utils.py:60-66, train.py:36-37), and the autograd backward of
 * the former:
 *   scores   [batch, num_candidates] fp32 (num_candidates includes the answer slot, dropped like
 *            utils.py:36-37);  answer [batch, num_candidates-1] uint8 one-hot (all-zero row: no gold);
 *   loss     [1] fp32 (written);  d_scores [batch, num_candidates] fp32 = d loss / d scores, or NULL;
 *   correct  [num_topk] int64, ACCUMULATED (+=) like the metric's `correct` state; `topk` is a HOST array
 *            of up to 8 values of k; the caller adds `batch` to its `total`.
 * Ties count as correct (`y_pred >= lower`), NaN scores order as in torch.topk, a NaN loss propagates. */
DRIN_API size_t drin_loss_workspace_bytes(int32_t batch);
DRIN_API int drin_triplet_topk(const float* scores, const uint8_t* answer, int32_t batch, int32_t num_candidates,
                               float margin, const int32_t* topk, int32_t num_topk, float* loss, float* d_scores,
                               int64_t* correct, void* workspace, size_t workspace_bytes, void* stream);

/* ---- caller-side optimiser step of the training configs ------------------------------------------ *
 * `torch.optim.Adam(self.parameters(), lr)` of train.py:55-56 (torch defaults: betas (0.9, 0.999), eps 1e-8, no weight
 * decay, no amsgrad), one step over `n` contiguous fp32 elements in ONE launch - a flat bucket holding every parameter
 * that receives a gradient, its gradient bucket (what drin_backward wrote / RCCL all-reduced) and the two moment buckets.
 * The op sequence and the per-op fp32 rounding are those of torch's default multi-tensor implementation, so a training
 * loop stepped with it tracks the reference's loop bit for bit (csrc/optim_kernels.hip).  Scalars, formed on the HOST in
 * double precision as torch/optim/adam.py forms them for step t (1-based) and rounded to fp32 here:
 *   lerp_weight = 1 - beta1;  one_minus_beta2 = 1 - beta2;  bias_correction2_sqrt = (1 - beta2^t)^0.5;
 *   neg_step_size = -(lr / (1 - beta1^t)).
 * Every `a + s x` of that sequence is one fma, sqrt and the divisions are correctly rounded - what torch's kernels do on
 * this GPU (tools/adam_diag.py). */
DRIN_API int drin_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                            float lerp_weight, float beta2, float one_minus_beta2, float bias_correction2_sqrt, float eps,
                            float neg_step_size, void* stream);

/* ---- the MELHI baseline (reference baselines/melhi.py, WikiDiverse) ------------------------------ *
 * The reference's train.py selects it with model_type "melhi".  Scores [B, N] = cos(mention_final_map([left | right]),
 * entity_final_map([entity_feature | eim])) where left / right are what the reference's lstm_extract_last returns for the
 * two context sequences of each mention.  H = 3 embed_dim. */
typedef struct {
  int32_t batch;           /* B mentions (1 .. 16384)                                                   */
  int32_t num_candidates;  /* N = num_candidates_model                                                  */
  int32_t embed_dim;       /* D = bert_embed_dim (multiple of 4, <= 1024)                               */
  int32_t image_dim;       /* R = resnet_embed_dim (multiple of 4)                                      */
  int32_t mention_tokens;  /* L = max_mention_sentence_len (>= 2)                                       */
  int32_t image_regions;   /* P = resnet_num_region                                                     */
  int32_t precision;       /* DRIN_PREC_BF16X3 or DRIN_PREC_F32 (the contractions; the recurrence is fp32 FMA) */
  float cosine_eps;        /* 1e-8  (nn.CosineSimilarity default)                                        */
  float thres_tmim;        /* 0.3   (args.py thres_tmim: text / mention-image cosine, strict >)          */
  float thres_imie;        /* 0.3   (args.py thres_imie: mention-image / entity-image cosine, strict >)  */
} drin_melhi_config;

/* The WikiDiverse batch of melhi.py (entity_mask is not read).  Device pointers, fp32 unless int64. */
typedef struct {
  const float* mention_feature;  /* [B, L, D]                                                            */
  const int64_t* mention_mask;   /* [B, L]   0 / 1; its row sum ends the right context                  */
  const int64_t* start;          /* [B]      already +1 for CLS                                          */
  const int64_t* end;            /* [B]                                                                  */
  const float* mention_image;    /* [B, P, R]                                                            */
  const float* entity_feature;   /* [B, N, D]                                                            */
  const float* entity_image;     /* [B, N, R]                                                            */
} drin_melhi_batch;

/* The 10 state_dict tensors (nn.Linear layout weight[out][in]). */
typedef struct {
  const float *w_image_map_text, *b_image_map_text;       /* image_map_text                  [D, R], [D]     */
  const float *w_ih, *w_hh, *b_ih, *b_hh;                 /* mention_encoder.mention_lstm    [4H, H] x2, [4H] x2 */
  const float *w_mention_final_map, *b_mention_final_map; /* mention_encoder.mention_final_map [D, 2H], [D]  */
  const float *w_entity_final_map, *b_entity_final_map;   /* entity_final_map                [D, 2D], [D]    */
} drin_melhi_params;

/* Gradients of the same tensors, ACCUMULATED (+=); NULL: not wanted. */
typedef struct {
  float *w_image_map_text, *b_image_map_text;
  float *w_ih, *w_hh, *b_ih, *b_hh;
  float *w_mention_final_map, *b_mention_final_map;
  float *w_entity_final_map, *b_entity_final_map;
} drin_melhi_param_grads;

/* Bytes of workspace for drin_melhi_forward (for_training = 0) or for a forward kept for drin_melhi_backward (1); 0 on error. */
DRIN_API size_t drin_melhi_workspace_bytes(const drin_melhi_config* cfg, int for_training);

/* Model.forward of melhi.py.  `order` and `lengths` are HOST int32 [2, B] (row 0 the left contexts, row 1 the right ones):
 * lengths[s][b] is the length of the sequence the reference packs (the context length, 1 for its all-zero placeholder row:
 * left = min(start, L) - 1 if start > 1, right = sum(mention_mask) - end if that is > end), and order[s] is the permutation
 * torch.sort(torch.as_tensor(lengths[s], dtype=int64), descending=True) returns on the CPU - NOT stable, so the caller
 * computes it with that call and the library never sorts.  Refused on the host (DRIN_E_INDEX): an order that is not a
 * permutation or not sorted by descending length; lengths outside [1, L - 1] (left) / [1, L] (right): DRIN_E_SHAPE.  The
 * gather tables derived from the order are copied into the workspace with hipMemcpyAsync on `stream`.  The workspace
 * (drin_melhi_workspace_bytes) keeps what drin_melhi_backward needs. */
DRIN_API int drin_melhi_forward(const drin_melhi_config* cfg, const drin_melhi_batch* batch, const drin_melhi_params* params,
                                const int32_t* order, const int32_t* lengths, void* workspace, size_t workspace_bytes,
                                float* scores, void* stream);
/* Backward of the drin_melhi_forward that left `workspace` (sized for training), same batch, params, order and lengths:
 * accumulates the parameter gradients for grad_scores [B, N].  No gradients of the batch tensors. */
DRIN_API int drin_melhi_backward(const drin_melhi_config* cfg, const drin_melhi_batch* batch, const drin_melhi_params* params,
                                 const int32_t* order, const int32_t* lengths, void* workspace, size_t workspace_bytes,
                                 const float* grad_scores, const drin_melhi_param_grads* grads, void* stream);

/* ---- the GHMFC baseline (reference baselines/ghmfc.py), eval-mode scoring ------------------------- *
 * The reference's train.py selects it with model_type "ghmfc"; this is its default configuration (args.py: mention_final_layer_name
 * "multimodal", mention_multimodal_attention "bi", multimodal_subspace_activation "gelu", entity_final_layer_name "linear",
 * entity_final_pooling "avg", online_bert False) in eval() mode, where the dropout inside the four attentions is the identity.
 * Scores [B, N] = cos(MultimodalFusion(text, mask, image), Linear(entity)) (ghmfc.py:131-149, :237-251, :287-298; DESIGN.md
 * section 15).  Training is not implemented. */
typedef struct {
  int32_t batch;           /* B mentions (1 .. 2^20); processed in chunks of 256 inside the call           */
  int32_t num_candidates;  /* N = num_candidates_model                                                    */
  int32_t embed_dim;       /* D = bert_embed_dim   (multiple of 4 and of num_heads, <= 2048, D / H <= 256) */
  int32_t image_dim;       /* R = resnet_embed_dim (the same rules)                                        */
  int32_t mention_tokens;  /* L = max_mention_sentence_len (1 .. 512)                                      */
  int32_t image_regions;   /* P = resnet_num_region (1 .. 512)                                             */
  int32_t num_heads;       /* H = transformer_num_heads (8)                                                */
  int32_t entity_tokens;   /* 0: entity_feature is pooled [B, N, D] (WikiDiverse); T > 0: [B, N, T, D] + entity_mask (WikiMEL) */
  int32_t precision;       /* DRIN_PREC_BF16X3 or DRIN_PREC_F32 (the products; attention, LayerNorm, gate are fp32 FMA) */
  float layer_norm_eps;    /* 1e-5  (nn.LayerNorm default)                                                  */
  float cosine_eps;        /* 1e-8  (nn.CosineSimilarity default)                                           */
} drin_ghmfc_config;

/* The tensors of the reference's offline batch that this configuration reads (begin, end, entity_image are not).
 * Device pointers, fp32 unless int64. */
typedef struct {
  const float* mention_feature;  /* [B, L, D]                                                            */
  const int64_t* mention_mask;   /* [B, L]   nonzero = token; zero = padding (dropped as a KEY, kept as a query) */
  const float* mention_image;    /* [B, P, R]                                                            */
  const float* entity_feature;   /* [B, N, D], or [B, N, T, D] when entity_tokens = T > 0                */
  const int64_t* entity_mask;    /* [B, N, T] when entity_tokens > 0 (mean of tokens 1 : sum - 1), else not read */
} drin_ghmfc_batch;

/* One CrossAttention(dim_a, dim_b) (ghmfc.py:93-128), its 22 tensors in state-dict order; E = dim_a, Eb = dim_b. */
typedef struct {
  const float *a2b_wq, *a2b_wk, *a2b_wv;         /* a2b_attention.{q,k,v}_proj_weight   [E, E], [E, Eb], [E, Eb] */
  const float *a2b_in_bias;                      /* a2b_attention.in_proj_bias          [3 E]                    */
  const float *a2b_wo, *a2b_bo;                  /* a2b_attention.out_proj              [E, E], [E]              */
  const float *a2b_ffn_w, *a2b_ffn_b;            /* a2b_ffn                             [E, E], [E]              */
  const float *b2a_in_w, *b2a_in_bias;           /* b2a_attention.in_proj_{weight,bias} [3 E, E], [3 E]          */
  const float *b2a_wo, *b2a_bo;                  /* b2a_attention.out_proj              [E, E], [E]              */
  const float *b2a_ffn_w, *b2a_ffn_b;            /* b2a_ffn                             [E, E], [E]              */
  const float *ln0_w, *ln0_b, *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;   /* layernorms.0 .. 3  [E] each */
} drin_ghmfc_cross_params;

/* The 52 state_dict tensors of ghmfc.py's Model, in state-dict order (nn.Linear layout weight[out][in]). */
typedef struct {
  drin_ghmfc_cross_params t2v;                   /* mention_encoder.intermediate_layer.t2v_attention  (E = D, Eb = R) */
  drin_ghmfc_cross_params v2t;                   /* mention_encoder.intermediate_layer.v2t_attention  (E = R, Eb = D) */
  const float *w_text_linear, *b_text_linear;    /* ....text_linear    [D, D], [D]                                    */
  const float *w_image_linear, *b_image_linear;  /* ....image_linear   [D, R], [D]                                    */
  const float *w_score_linear, *b_score_linear;  /* ....score_linear   [2, 2 D], [2]                                  */
  const float *w_entity, *b_entity;              /* entity_encoder.final_layer [D, D], [D]                            */
} drin_ghmfc_params;

/* Bytes of workspace for drin_ghmfc_forward: one chunk of min(B, 256) mentions; 0 on error (drin_last_error). */
DRIN_API size_t drin_ghmfc_workspace_bytes(const drin_ghmfc_config* cfg);

/* Model.forward of ghmfc.py in eval() mode: scores [B, N]; mention_repr (may be NULL) receives the [B, D] output of
 * mention_encoder.  Writes `scores`, `mention_repr` and the workspace, nothing else.  A mention whose mask is all zero has
 * zero attention weights wherever the text is the key (the out-projection then returns its bias), as torch's kernel: finite. */
DRIN_API int drin_ghmfc_forward(const drin_ghmfc_config* cfg, const drin_ghmfc_batch* batch, const drin_ghmfc_params* params,
                                void* workspace, size_t workspace_bytes, float* scores, float* mention_repr, void* stream);

/* The mention half of drin_ghmfc_forward alone: mention_repr [B, D] with that call's bits (the same launches in the same
 * shapes).  Neither batch->entity_feature / entity_mask nor cfg->num_candidates / entity_tokens is read: what a caller that
 * links mentions against the whole table (drin_table_topk) needs.  The workspace has no entity regions; 0 bytes on error. */
DRIN_API size_t drin_ghmfc_mention_forward_workspace_bytes(const drin_ghmfc_config* cfg);
DRIN_API int drin_ghmfc_mention_forward(const drin_ghmfc_config* cfg, const drin_ghmfc_batch* batch, const drin_ghmfc_params* params,
                                        void* workspace, size_t workspace_bytes, float* mention_repr, void* stream);

/* The table form of drin_ghmfc_forward: the candidates of a mention are rows of a device-resident entity
 * table, as on WikiMEL, where the reference's loader gathers them on the host (baselines/data.py: the qid2idx gather,
 * `entity_feature[rows]`, 19.9 MB per mention at the reference widths).  `size` = sizeof(drin_ghmfc_table). */
typedef struct {
  size_t size;
  const float* text;         /* [num_entities, entity_tokens, D], or pooled [num_entities, D] when entity_tokens = 0; not read with rows */
  const int64_t* mask;       /* [num_entities, entity_tokens] when entity_tokens > 0, else not read                                     */
  int64_t num_entities;      /* E >= 1                                                                                                   */
  int32_t entity_tokens;     /* T of the TABLE (0 .. 512); drin_ghmfc_config.entity_tokens is not read by the table form                 */
  const int64_t* candidates; /* [B, N] rows of the table; outside [0, E - 1]: clamped and reported (drin_gather_rows above)              */
  int32_t* index_status;     /* int32[4] or NULL                                                                                         */
  const float* rows;         /* NULL, or drin_ghmfc_entity_rows' [num_entities, D]: then the entity half is ONE cosine against them     */
} drin_ghmfc_table;

/* Bytes of workspace for drin_ghmfc_forward_table (less with table->rows: no entity regions); 0 on error (drin_last_error). */
DRIN_API size_t drin_ghmfc_table_workspace_bytes(const drin_ghmfc_config* cfg, const drin_ghmfc_table* table);

/* drin_ghmfc_forward with the entity side (ghmfc.py:237-250, :297-298) read through table->candidates; batch->entity_feature
 * and batch->entity_mask are not read.  The mention half is drin_ghmfc_forward's own.  With table->rows == NULL, per chunk of 256
 * mentions: the indexed token mean (the row gather, for a pooled table), the same [chunk N, D] product, the same cosine - the
 * same values in the same shapes, so scores and mention_repr have the BITS of drin_ghmfc_forward on the gathered batch.  With
 * table->rows the scores agree with it to the rounding of one product evaluated per entity instead of per pair. */
DRIN_API int drin_ghmfc_forward_table(const drin_ghmfc_config* cfg, const drin_ghmfc_batch* batch, const drin_ghmfc_params* params,
                                      const drin_ghmfc_table* table, void* workspace, size_t workspace_bytes, float* scores,
                                      float* mention_repr, void* stream);

/* rows[e, :] = final_layer(pool(text[e])) for every entity (ghmfc.py:245-250 once per ENTITY instead of once per pair): text
 * [num_entities, entity_tokens, width] with mask, or pooled [num_entities, width] when entity_tokens = 0 (no workspace then);
 * w_entity [width, width], b_entity [width]; precision: DRIN_PREC_BF16X3 or DRIN_PREC_F32.  Chunks of 65536 entities: token
 * mean into the workspace, then the product.  The rows depend on entity_encoder.final_layer only: rebuild after it changes. */
DRIN_API size_t drin_ghmfc_entity_rows_workspace_bytes(int64_t num_entities, int32_t entity_tokens, int32_t width);
DRIN_API int drin_ghmfc_entity_rows(const float* text, const int64_t* mask, int64_t num_entities, int32_t entity_tokens, int32_t width,
                                    const float* w_entity, const float* b_entity, int32_t precision, float* rows, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* How the WikiMEL entity tokens are pooled (args.py entity_final_pooling, ghmfc.py:210-214,245-249): the mean or the maximum
 * over tokens 1 : ntok - 1, ntok = sum(mask).  "bert default" has no id: the reference's own EntityEncoder constructor raises
 * ValueError on it.  An empty slice (ntok 1 or 2) gives a NaN row under EITHER pooling: the mean is 0 / 0 there as in the
 * reference, while the reference's max raises IndexError ("max(): Expected reduction dim 0 to have non-zero size"), which a
 * kernel cannot do.  A NaN inside the slice wins the max, as torch.max; nothing outside the slice is read. */
typedef enum { DRIN_POOL_AVG = 0, DRIN_POOL_MAX = 1 } drin_entity_pooling;

/* drin_ghmfc_entity_rows with the entity encoder's settings: `pooling` (drin_entity_pooling; not read when entity_tokens = 0,
 * as the reference pools WikiMEL tokens only) and entity_final_layer_name = "none" as w_entity == b_entity == NULL
 * (final_layer = Identity): the pool then writes straight into `rows` (a pooled table is copied), there is no product and the
 * workspace is not read.  Exactly one of the two being NULL is DRIN_E_NULL.  DRIN_POOL_AVG with both weights: the launches and
 * the bits of drin_ghmfc_entity_rows.  drin_ghmfc_entity_rows_workspace_bytes is a sufficient size. */
DRIN_API int drin_ghmfc_entity_rows_ex(const float* text, const int64_t* mask, int64_t num_entities, int32_t entity_tokens, int32_t width,
                                       int32_t pooling, const float* w_entity, const float* b_entity, int32_t precision, float* rows,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* The multi-head softmax-attention core on projected operands (what nn.MultiheadAttention runs between its in- and
 * out-projections, ghmfc.py:120,124): out[b, i, h] = softmax_j(q[b, i, h] . k[b, j, h] / sqrt(head_dim) + mask) v[b, j, h].
 * q [batch * q_len, E], k, v [batch * k_len, E], out [batch * q_len, E] are row-major with row strides ldq, ldk, ldv, ldo
 * (floats, >= E = num_heads * head_dim); head h is columns h * head_dim .. (h + 1) * head_dim - 1, so K | V packed in one
 * [rows, 2 E] buffer are k = buf, v = buf + E, ldk = ldv = 2 E.  key_mask: int64 [batch, k_len], nonzero = keep, or NULL.
 * A query row with no kept key gets zeros.  fp32 FMA, max-subtracted, no atomics: the same bits every run.
 * Any q_len >= 1, k_len in [1, 512], head_dim in [1, 256], batch and num_heads in [1, 65535]. */
DRIN_API int drin_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                            const int64_t* key_mask, float* out, int64_t ldo, int32_t batch, int32_t num_heads, int32_t q_len,
                            int32_t k_len, int32_t head_dim, void* stream);

/* drin_attention for training: the same kernel (out has drin_attention's bits) also writes the row statistic the backward
 * recomputes the probabilities from: lse [batch, num_heads, q_len] = log sum_j exp(score) (natural log) over the kept keys
 * of the scaled scores, -inf for a row with no kept key (its out row is zero).  The forward half of what
 * nn.MultiheadAttention runs between its projections at ghmfc.py:120,124 when train.py:33-34 backpropagates. */
DRIN_API int drin_attention_train_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                      const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch,
                                      int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim, void* stream);

/* Backward of the core (what autograd does for ghmfc.py:120,124 under train.py:33-34).  q, k, v, key_mask: the forward's
 * operands; out, lse: what drin_attention_train_fwd wrote; dout [batch * q_len, E] with row stride lddo: the gradient of out.
 * With p = exp(score - lse), delta[i] = sum_c dout[i, c] out[i, c] and ds = p (dout v^T - delta):
 *   dq = ds k / sqrt(head_dim)      [batch * q_len, E], row stride lddq   (may be NULL: not computed)
 *   dk = ds^T q / sqrt(head_dim)    [batch * k_len, E], row stride lddk
 *   dv = p^T dout                   [batch * k_len, E], row stride lddv   (dk and dv: both given or both NULL)
 * Gradients are WRITTEN, not accumulated, and only into their own E columns of each row (strides >= E; dK | dV packed in one
 * [rows, 2 E] buffer are dk = buf, dv = buf + E, lddk = lddv = 2 E).  A dropped key's dk and dv rows are exactly 0; a query
 * row with no kept key has a dq row of exactly 0 and adds nothing to dk or dv.  delta_scratch: [batch, num_heads, q_len]
 * floats, overwritten.  fp32 FMA, no atomics (a workgroup owns its query rows / its keys): the same bits every run, and the
 * bits of dk and dv do not depend on whether dq is asked for.  Limits as drin_attention. */
DRIN_API int drin_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                const int64_t* key_mask, const float* out, int64_t ldo, const float* lse, const float* dout,
                                int64_t lddo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv,
                                float* delta_scratch, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len,
                                int32_t head_dim, void* stream);

/* ---- attention dropout (what nn.MultiheadAttention(dropout = transformer_dropout) does in train() mode, ghmfc.py:96-110) -- *
 * The library's own mask, NOT torch's random stream: element (b, h, i, j) of the [batch, num_heads, q_len, k_len] attention
 * weights is kept iff the Philox4x32-10 word of (seed, call, flat index) is >= llrint(p * 2^32), and a kept weight is
 * multiplied by 1 / (1 - p): out[i] = sum_j P[i, j] M[i, j] / (1 - p) v[j] with P the undropped softmax.  The function is
 * defined once for host and device in csrc/dropout_mask.h (the contract) and exported to the host as
 * drin_attention_dropout_keep.  p in [0, 1), anything else (a NaN too) is DRIN_E_SHAPE; p = 0 gives
 * drin_attention_train_fwd / drin_attention_bwd's bits.  `seed` keys the generator, `call` numbers the draw: the caller
 * gives every forward its own call number and hands the same (p, seed, call) to its backward. */

/* drin_attention_train_fwd with dropout on the weights; lse is unchanged: the log-sum-exp of the undropped scores. */
DRIN_API int drin_attention_dropout_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                        const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch,
                                        int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim, float p, uint64_t seed,
                                        uint64_t call, void* stream);
/* drin_attention_bwd of that forward.  With Pd = P M / (1 - p): dv = Pd^T dout, dp = (dout v^T) M / (1 - p),
 * ds = P (dp - delta), delta[i] = sum_c dout[i, c] out[i, c] as before (out = Pd v).  A key dropped by key_mask still has
 * dk and dv rows of exactly 0. */
DRIN_API int drin_attention_dropout_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                        const int64_t* key_mask, const float* out, int64_t ldo, const float* lse,
                                        const float* dout, int64_t lddo, float* dq, int64_t lddq, float* dk, int64_t lddk,
                                        float* dv, int64_t lddv, float* delta_scratch, int32_t batch, int32_t num_heads,
                                        int32_t q_len, int32_t k_len, int32_t head_dim, float p, uint64_t seed, uint64_t call,
                                        void* stream);
/* HOST only, no GPU: keep_host[((b * num_heads + h) * q_len + i) * k_len + j] = 1 if the weight is kept, else 0. */
DRIN_API int drin_attention_dropout_keep(uint64_t seed, uint64_t call, int32_t batch, int32_t num_heads, int32_t q_len,
                                         int32_t k_len, float p, uint8_t* keep_host);

/* ---- the same core on the matrix pipes (csrc/attention_mfma.hip) --------------------------------- *
 * An opt-in beside the FMA entry points above, which keep their bits.  Every product (q k^T, p v, dout v^T, p^T dout, ds k,
 * ds^T q) is the library's split-bf16 form: each fp32 operand x is hi = bf16(x), lo = bf16(x - hi), and hi hi + hi lo + lo hi
 * accumulate in fp32 through v_mfma_f32_16x16x32_bf16 - close to fp32, not exact.  Softmax, max, sum, lse, delta and
 * ds = p (dp - delta) stay fp32.  Operands, strides, key_mask, limits and the dropout mask (same (p, seed, call), same kept
 * weights) are those of drin_attention_dropout_fwd / _bwd; p in [0, 1), anything else is DRIN_E_SHAPE; p = 0 means no
 * dropout (seed and call are then not read).  No atomics (a workgroup owns its query rows / its keys): the same bits every
 * run.  All arguments are checked on the host before a launch. */

/* out, and lse [batch, num_heads, q_len] unless lse is NULL (inference; out has the same bits either way): the natural
 * log-sum-exp over the kept keys of the undropped scaled scores, -inf for a row with no kept key (its out row is zero). */
DRIN_API int drin_attention_mfma_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                     const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch,
                                     int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim, float p, uint64_t seed,
                                     uint64_t call, void* stream);
/* Backward of that forward (out, lse: what it wrote).  dq may be NULL (not computed); dk and dv are both given or both NULL.
 * Gradients are WRITTEN, not accumulated, and only into their own E columns of each row (strides >= E; dK | dV packed in one
 * [rows, 2 E] buffer are dk = buf, dv = buf + E, lddk = lddv = 2 E).  A dropped key's dk and dv rows are exactly 0; a query
 * row with no kept key has a dq row of exactly 0 and adds nothing to dk or dv.  delta_scratch: [batch, num_heads, q_len]
 * floats, overwritten.  The bits of dk and dv do not depend on whether dq is asked for. */
DRIN_API int drin_attention_mfma_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                     const int64_t* key_mask, const float* out, int64_t ldo, const float* lse, const float* dout,
                                     int64_t lddo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv,
                                     float* delta_scratch, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len,
                                     int32_t head_dim, float p, uint64_t seed, uint64_t call, void* stream);

/* ---- GHMFC's row operations one by one, forward and backward --------------- *
 * What drin_ghmfc_forward runs between its products, exposed so that a training step can be composed from them, and their
 * backward kernels.  Every pointer is a 16-byte aligned device pointer, rows are contiguous, widths are multiples of 4.
 * All arguments are checked on the host before a launch.  fp32 FMA, no atomics: the same bits every run.  Gradients are
 * WRITTEN, not accumulated.  Profiler class DRIN_KC_NORM (the cosine and the token mean keep their own classes). */

/* y = LayerNorm(x [+ res]) * gamma + beta over rows of `width` (<= 2048) floats; res may be NULL; y may be x or res.
 * y has the bits drin_ghmfc_forward's LayerNorm gives; mean, rstd [rows] are the statistics the backward needs. */
DRIN_API int drin_layernorm_res_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                                          float* mean, float* rstd, int64_t rows, int32_t width, float eps, void* stream);
/* Floats of scratch for drin_layernorm_res_bwd's column sums (0: rows < 1 or a bad width). */
DRIN_API size_t drin_layernorm_res_bwd_scratch_floats(int64_t rows, int32_t width);
/* Backward of it: x, res, gamma, mean, rstd as in the forward, dy [rows, width] the gradient of y.  With xhat recomputed and
 * g = dy gamma: dh = rstd (g - mean_c(g) - xhat mean_c(g xhat)) [rows, width] is the gradient of the pre-norm sum, i.e. of
 * x AND of res (dh may be dy).  dgamma = sum_rows dy xhat, dbeta = sum_rows dy [width]: per-workgroup partial sums in
 * `scratch`, then added in a fixed order.  dgamma and dbeta may be NULL (frozen LayerNorm; with both NULL the reduction is
 * skipped and scratch is not read); dh has the same bits either way. */
DRIN_API int drin_layernorm_res_bwd(const float* x, const float* res, const float* mean, const float* rstd, const float* gamma,
                                    const float* dy, float* dh, float* dgamma, float* dbeta, float* scratch,
                                    size_t scratch_floats, int64_t rows, int32_t width, void* stream);

/* out[b, c] = max_s x[b, s, c] over ALL seq_len positions of x [batch, seq_len, width] (a NaN wins, as torch.max), with
 * drin_ghmfc_forward's bits, and idx[b, c] (int32) = the LOWEST position that attains it; a column that holds a NaN reports
 * its lowest NaN position.  batch <= 65535. */
DRIN_API int drin_seq_max_train_fwd(const float* x, float* out, int32_t* idx, int32_t batch, int32_t seq_len, int32_t width,
                                    void* stream);
/* dx [batch, seq_len, width], every element written: dout[b, c] at (b, idx[b, c], c), exactly 0 elsewhere. */
DRIN_API int drin_seq_max_bwd(const float* dout, const int32_t* idx, float* dx, int32_t batch, int32_t seq_len, int32_t width,
                              void* stream);

/* The gate (ghmfc.py:144-149): t = gelu(tl), v = gelu(vl) [batch, width], z = [t | v] ws^T + bs (ws [2, 2 width], bs [2]),
 * s = softmax(z), out = s0 t + s1 v, with drin_ghmfc_forward's bits. */
DRIN_API int drin_gate_mix_fwd(const float* tl, const float* vl, const float* ws, const float* bs, float* out, int32_t batch,
                               int32_t width, void* stream);
DRIN_API size_t drin_gate_mix_bwd_scratch_floats(int32_t batch, int32_t width);
/* Backward of it (width <= 2048): t, v, z, s are recomputed.  With a = sum_c dout_c (t_c - v_c): dz0 = s0 s1 a = -dz1,
 * dt = s0 dout + dz0 ws[0, :width] + dz1 ws[1, :width], dv likewise with s1 and the right halves, dtl = dt gelu'(tl),
 * dvl = dv gelu'(vl) (exact-erf gelu').  dws [2, 2 width] and dbs [2] are sums over the mentions, reduced in order through
 * `scratch`; each may be NULL. */
DRIN_API int drin_gate_mix_bwd(const float* tl, const float* vl, const float* ws, const float* bs, const float* dout, float* dtl,
                               float* dvl, float* dws, float* dbs, float* scratch, size_t scratch_floats, int32_t batch,
                               int32_t width, void* stream);

/* out[b, n] = cos(x[b, :], y[b, n, :]) with nn.CosineSimilarity's eps clamp; x [batch, width], y [batch, num_candidates, width]
 * (num_candidates <= 65535). */
DRIN_API int drin_cosine_rows_fwd(const float* x, const float* y, float* out, int32_t batch, int32_t num_candidates, int32_t width,
                                  float eps, void* stream);
/* dx [batch, width], dy [batch, num_candidates, width] for dout [batch, num_candidates]; scratch: 3 batch num_candidates
 * floats; width <= 1024. */
DRIN_API int drin_cosine_rows_bwd(const float* x, const float* y, const float* dout, float* dx, float* dy, float* scratch,
                                  size_t scratch_floats, int32_t batch, int32_t num_candidates, int32_t width, float eps,
                                  void* stream);
/* out[p, :] = mean(feat[p, 1 : ntok - 1, :]), ntok = sum(mask[p, :]) (ghmfc.py:245-249); feat [pairs, tokens, width], mask
 * int64 [pairs, tokens].  Fewer than 3 tokens: a NaN row, as the reference's empty mean. */
DRIN_API int drin_entity_token_mean(const float* feat, const int64_t* mask, float* out, int64_t pairs, int32_t tokens,
                                    int32_t width, void* stream);
/* The same slice with a pooling (drin_entity_pooling): DRIN_POOL_AVG is drin_entity_token_mean's launch and bits;
 * DRIN_POOL_MAX: out[p, c] = max over t in [1, ntok - 1) of feat[p, t, c], exact (a NaN inside the slice wins, rows outside
 * it are not read, an empty slice gives a NaN row where the reference raises IndexError).  fp32; tokens 1 .. 512. */
DRIN_API int drin_entity_token_pool(const float* feat, const int64_t* mask, float* out, int64_t pairs, int32_t tokens, int32_t width,
                                    int32_t pooling, void* stream);

/* ---- the row operations of GHMFC's table form -------------------------------------------------- *
 * The entity side read through candidate ROWS of a device-resident table instead of gathered features: what the reference
 * gathers on the host per mention (baselines/data.py: `[self.qid2idx[q] ...]`, `entity_feature[rows]`) and then encodes per
 * pair (baselines/ghmfc.py:237-250, :297-298).  `index` is int64; an index outside [0, num_entities - 1] is clamped BEFORE
 * any address is formed from it (nothing out of range is read) and reported into `index_status`, int32[4] on the device,
 * with the semantics of drin_batch.index_status: the first reporter leaves {1, position in index, value low, value high},
 * sticky until drin_index_status - the caller's check - zeroes it; NULL clamps silently.  width % 4 == 0 is the only width
 * condition; table / text, x, rows and out are 16-byte aligned. */
/* out[i, :] = table[index[i], :]; table [num_entities, width] fp32, out [count, width] (count <= 2^31 - 1). */
DRIN_API int drin_gather_rows(const float* table, const int64_t* index, int64_t num_entities, float* out, int64_t count, int32_t width,
                              int32_t* index_status, void* stream);
/* drin_entity_token_mean of table row index[p]: text [num_entities, tokens, width], mask int64 [num_entities, tokens], out
 * [pairs, width] - the slice rules, the summation order and the bits of drin_entity_token_mean on the gathered block. */
DRIN_API int drin_entity_token_mean_indexed(const float* text, const int64_t* mask, const int64_t* index, int64_t num_entities,
                                            float* out, int64_t pairs, int32_t tokens, int32_t width, int32_t* index_status,
                                            void* stream);
/* drin_entity_token_pool of table row index[p] (clamped before any address is formed and reported, as above): the bits of the
 * plain form on the gathered block; DRIN_POOL_AVG is drin_entity_token_mean_indexed. */
DRIN_API int drin_entity_token_pool_indexed(const float* text, const int64_t* mask, const int64_t* index, int64_t num_entities,
                                            float* out, int64_t pairs, int32_t tokens, int32_t width, int32_t pooling,
                                            int32_t* index_status, void* stream);
/* out[b, n] = cos(x[b, :], rows[index[b, n], :]); x [batch, width], rows [num_entities, width], index [batch, num_candidates]:
 * the bits of drin_cosine_rows_fwd on the gathered rows. */
DRIN_API int drin_cosine_rows_indexed_fwd(const float* x, const float* rows, const int64_t* index, int64_t num_entities, float* out,
                                          int32_t batch, int32_t num_candidates, int32_t width, float eps, int32_t* index_status,
                                          void* stream);

/* ---- linking against bf16-STORED table rows --------------------------------------------------------- *
 * The *_ex twins of the link entry points take how the TABLE rows are stored: row_dtype = DRIN_FEAT_F32 | DRIN_FEAT_BF16 (any
 * other value: DRIN_E_UNSUPPORTED).  THE CONTRACT: a bf16 table links exactly as its exactly-widened fp32 copy would.  The rows
 * are read in place - 8 bytes per lane and column quad, each element widened by a 16-bit shift, the sums in the order of the
 * fp32 kernels - and no widened copy of a table ever exists.  With DRIN_FEAT_F32 a twin runs the old entry point's code and
 * returns its bits.  bf16 rows need width % 8 == 0 (DRIN_E_SHAPE) and 16-byte aligned rows (DRIN_E_ALIGN), refused among the
 * argument checks before any launch.  Mentions (x), inverse norms and every output stay fp32.
 *
 * drin_cosine_rows_indexed_fwd with `rows` stored as row_dtype: bit for bit the old entry point on the widened table.  No
 * product: a row kernel. */
DRIN_API int drin_cosine_rows_indexed_fwd_ex(const float* x, const void* rows, int32_t row_dtype, const int64_t* index,
                                             int64_t num_entities, float* out, int32_t batch, int32_t num_candidates, int32_t width,
                                             float eps, int32_t* index_status, void* stream);

/* ---- cosine top-k against the whole table ------------------------------------------------------ *
 * The k best rows of rows [num_entities, width] for every mention x [batch, width] by cosine, without a [batch, num_entities]
 * score matrix: what a first stage does (baselines/data.py ranks num_candidates_model candidates that one chose).
 *
 * THE ORDERING CONTRACT, followed by every kernel and every entry point below.  For one mention, row a ranks before row b iff
 * score(a) > score(b), or the scores compare equal and a < b.  A NaN score ranks below -inf and all NaNs compare equal;
 * -0.0 == +0.0.  This is a total order: a top-k is ONE defined list, whatever way the columns are cut into slices, chunks or
 * calls.  No floating-point atomics anywhere: two runs give the same bits.
 *
 * The selection keeps, per mention, a running list of kp = DRIN_TOPK_KP(k) >= k entries (key, row) in that order, where
 * key = dot(x, row) * inv_norm[row]: the mention's own norm is one positive factor per mention and changes no ranking.
 * 1 <= k <= 256.  A block of dot products is ENTITY-major, as the product rows_chunk x^T leaves it: the dot product of mention
 * b with column c (table row col_base + c) is block[c * ld + b]; ld % 4 == 0, ld >= batch rounded up to a multiple of 4. */
#define DRIN_TOPK_SLICE 4096 /* columns per workgroup of the partial selection */
#define DRIN_TOPK_KP(k) ((k) <= 64 ? 64 : (k) <= 128 ? 128 : 256)

/* out[e] = 1 / max(sqrt(sum_d rows[e, d]^2), eps) for rows [num_entities, width]; eps > 0. */
DRIN_API int drin_row_inv_norms(const float* rows, int64_t num_entities, int32_t width, float eps, float* out, void* stream);
/* The same for rows stored as row_dtype (the contract of the *_ex twins above: a bf16 table links exactly as its exactly-widened
 * fp32 copy would - bit for bit the old entry point on the widened rows).  No product: a row kernel. */
DRIN_API int drin_row_inv_norms_ex(const void* rows, int32_t row_dtype, int64_t num_entities, int32_t width, float eps, float* out,
                                   void* stream);

/* The selection alone, on caller-supplied dot products: merges the `cols` columns of `block` (table rows col_base ..
 * col_base + cols - 1, keys block[c * ld + b] * col_inv_norms[c]; col_inv_norms NULL = 1) into the running lists state_keys
 * [batch, kp] (float) / state_rows [batch, kp] (int64; -1 = an empty entry, its key is NaN), which `first` != 0 initialises
 * instead of reading.  scratch: at least ceil(cols / DRIN_TOPK_SLICE) * batch * kp * 8 bytes.  With out_keys / out_rows (both or
 * neither) the first k entries of the lists - sorted by the contract - are written to out_keys [batch, k], out_rows int64
 * [batch, k] after the merge; cols = 0 (block and scratch not read, first = 0) only does that.  Keys come back canonical
 * (+0.0 for -0.0, one quiet NaN).  block, state_keys, state_rows and scratch are 16-byte aligned; batch 1 .. 65535.  Columns
 * may arrive in any order and any cut; a row fed twice is listed twice. */
DRIN_API int drin_topk_update(const float* block, int64_t ld, int32_t batch, int64_t cols, int64_t col_base, const float* col_inv_norms,
                              int32_t k, float* state_keys, int64_t* state_rows, void* scratch, size_t scratch_bytes, int32_t first,
                              float* out_keys, int64_t* out_rows, void* stream);

/* Bytes of workspace for drin_table_topk; 0 on error (drin_last_error: a bad shape, or a chunk_entities whose block does not
 * fit).  chunk_entities = 0: the default chunk, a multiple of 256 rows whose block of dot products stays within 256 MiB. */
DRIN_API size_t drin_table_topk_workspace_bytes(int32_t batch, int64_t num_entities, int32_t width, int32_t k, int64_t chunk_entities);

/* out_rows [batch, k] (int64) = the k best rows of the table for each mention, out_scores [batch, k] their cosines, ordered by
 * the contract.  Per chunk of chunk_entities rows: ONE product block[chunk, Bp] = rows_chunk x^T (x padded to Bp = batch rounded
 * up to 4 rows in the workspace; `precision`: DRIN_PREC_BF16X3 or DRIN_PREC_F32, the kernel is the GEMM module's choice by the
 * chunk's row count), then the selection with row_inv_norms (drin_row_inv_norms of rows with cosine_eps).  After the last chunk
 * the kp selected rows are scored again as drin_cosine_rows_indexed_fwd scores them (fp32 FMA) and sorted: out_scores ARE that
 * entry point's bits on out_rows; the product's precision only decides which rows reach the list of kp.  batch 1 .. 65535,
 * width % 4 == 0, 1 <= k <= min(256, num_entities).  Writes out_scores, out_rows and the workspace, nothing else. */
DRIN_API int drin_table_topk(const float* x, const float* rows, const float* row_inv_norms, int64_t num_entities, int32_t batch,
                             int32_t width, int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities, void* workspace,
                             size_t workspace_bytes, float* out_scores, int64_t* out_rows, void* stream);
/* drin_table_topk against rows stored as row_dtype: a bf16 table links exactly as its exactly-widened fp32 copy would.  The
 * product of a chunk of bf16 rows takes one of two routes, chosen by the GEMM module.  PLANE route - DRIN_PREC_BF16X3 and
 * width % 32 == 0: the chunk is, as stored, the hi plane of the plane kernel with no lo plane (two of the three split-bf16 MFMAs),
 * against the hi / lo planes of the padded mentions, split once per call; the table's bytes are read once.  WIDEN route -
 * DRIN_PREC_F32, or a width that misses the plane kernel: the chunk is widened into the workspace and the old product runs on
 * it, so in DRIN_PREC_F32 the block of dot products, and with it the selected list, is what drin_table_topk computes on the widened
 * table.  out_scores are drin_cosine_rows_indexed_fwd_ex's bits on out_rows.  The workspace query takes row_dtype and precision
 * because the route decides the extra region: Bp * width floats of planes, or chunk * width floats of widened rows - and the
 * default chunk (chunk_entities = 0) of the widen route keeps that region within the 256 MiB budget as well.  With DRIN_FEAT_F32
 * both are the old entry points: their bytes, their bits. */
DRIN_API size_t drin_table_topk_workspace_bytes_ex(int32_t batch, int64_t num_entities, int32_t width, int32_t k, int64_t chunk_entities,
                                                   int32_t row_dtype, int32_t precision);
DRIN_API int drin_table_topk_ex(const float* x, const void* rows, int32_t row_dtype, const float* row_inv_norms, int64_t num_entities,
                                int32_t batch, int32_t width, int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities,
                                void* workspace, size_t workspace_bytes, float* out_scores, int64_t* out_rows, void* stream);

/* ---- a SUM of cosines against the tables ------------------------------------------------------------ *
 * score(b, e) = sum_s weight_s * cos(x_s[b, :], rows_s[e, :]) over 1 .. DRIN_TOPK_MAX_TERMS (query, table) pairs that share
 * batch and num_entities but not their width: late-fusion retrieval, and DRIN's own layer-0 evidence for a pair (the text-text
 * edge of model.py:71-76 and the two CLIP edges of model.py:203; the image-image edge of model.py:84-92 is no cosine of one row
 * against one row and enters as a term of the RATIO form below).  THE ORDERING CONTRACT above applies. */
#define DRIN_TOPK_MAX_TERMS 4
typedef struct drin_topk_term { /* one cosine of the sum */
  const float* x;             /* [batch, width] */
  const float* rows;          /* [num_entities, width], contiguous */
  const float* row_inv_norms; /* drin_row_inv_norms(rows, cosine_eps) */
  int32_t width;              /* % 4 == 0 */
  float weight;               /* finite; 0 = the term is dropped before any launch and its pointers may be NULL */
} drin_topk_term;

/* The combine alone, on caller-supplied blocks of dot products (entity-major, as drin_topk_update reads them):
 *   out[c * ld + b] = sum_s blocks[s][c * ld + b] * col_inv_norms[s][c] * (row_scales[s][b] * weights[s])
 * in term order, every multiply and add rounded to fp32 on its own (no contraction).  blocks, col_inv_norms, row_scales: HOST
 * arrays of num_terms device pointers - blocks[s] [cols, ld], col_inv_norms[s] [cols], row_scales[s] [ld] (all ld entries are
 * read) - and weights a HOST array of num_terms finite floats.  out [cols, ld] may be blocks[0].  One launch, a pure stream
 * over num_terms blocks in and one out.  blocks, row_scales and out are 16-byte aligned; ld % 4 == 0, ld >= batch rounded up to
 * a multiple of 4; cols >= 1; batch 1 .. 65535.  `batch` only bounds ld from below: ALL ld columns of every row are combined,
 * the padding columns included (drin_topk_update then reads the first `batch` of them).  Writes out, nothing else.  Profiler
 * class DRIN_KC_EDGE. */
DRIN_API int drin_topk_combine(const float* const* blocks, const float* const* col_inv_norms, const float* const* row_scales,
                               const float* weights, int32_t num_terms, int64_t ld, int32_t batch, int64_t cols, float* out,
                               void* stream);

/* Bytes of workspace for drin_table_topk_sum; 0 on error (drin_last_error).  Reads the widths and the weights of `terms` only;
 * a term of weight 0 takes no room.  chunk_entities = 0: the default chunk, a multiple of 256 rows whose live blocks of dot
 * products TOGETHER stay within 256 MiB. */
DRIN_API size_t drin_table_topk_sum_workspace_bytes(const drin_topk_term* terms, int32_t num_terms, int32_t batch, int64_t num_entities,
                                                    int32_t k, int64_t chunk_entities);

/* out_rows [batch, k] (int64) = the k best rows by the summed score for each mention, out_scores [batch, k] their scores,
 * ordered by the contract.  `terms`: a HOST array of num_terms (1 .. 4) terms, at least one with a weight != 0.  Every x_s is
 * padded to Bp rows in the workspace and gets a per-mention factor weight_s / max(|x_s[b]|, cosine_eps) - unlike
 * drin_table_topk, the mention norms differ per term and do change the ranking.  Per chunk of chunk_entities rows: one product
 * per live term into that term's block[chunk, Bp] (`precision`: DRIN_PREC_BF16X3 or DRIN_PREC_F32, the kernel is the GEMM
 * module's choice), ONE combine of the blocks into the scores (drin_topk_combine's sum), then the selection of
 * drin_topk_update.  After the last chunk the kp selected rows are scored again: c_s = the bits drin_cosine_rows_indexed_fwd
 * gives for (x_s, rows_s, row), then acc = w_0 * c_0; acc = acc + w_s * c_s over the live terms in order, every multiply and
 * add rounded to fp32 on its own - out_scores ARE that chain's bits; the products' precision only decides which rows reach the
 * list of kp.  With ONE term of weight 1 the scores of a row are drin_table_topk's bits, but the selection key carries one more
 * fp32 factor (the mention's), so two keys that differ there may round to a tie here - broken by the lower row - and a key may
 * overflow for a mention whose norm is at cosine_eps: which rows reach the list of kp can differ from drin_table_topk's at
 * that boundary; the two calls agree up to such ties, not by construction.  k, batch and precision as drin_table_topk; every live width % 4 == 0; x, rows and row_inv_norms of a live term
 * 16-byte aligned.  Writes out_scores, out_rows and the workspace, nothing else.  Profiler class DRIN_KC_EDGE. */
DRIN_API int drin_table_topk_sum(const drin_topk_term* terms, int32_t num_terms, int64_t num_entities, int32_t batch, int32_t k,
                                 float cosine_eps, int32_t precision, int64_t chunk_entities, void* workspace, size_t workspace_bytes,
                                 float* out_scores, int64_t* out_rows, void* stream);
/* drin_table_topk_sum with the storage of every term's rows: row_dtypes, a HOST array [num_terms] of DRIN_FEAT_F32 |
 * DRIN_FEAT_BF16 beside the unchanged terms (terms[s].rows then addresses bf16 rows; width % 8 == 0).  Terms may mix; the entry
 * of a dropped term (weight 0) is not read.  A bf16 table links exactly as its exactly-widened fp32 copy would: each live term's
 * product takes the plane or the widen route as drin_table_topk_ex's does (per term: DRIN_PREC_BF16X3 and width % 32 == 0 is the
 * plane route), the re-score is drin_cosine_rows_indexed_fwd_ex's, the chain is unchanged.  The workspace grows by Bp * width
 * floats of planes per plane-route term and by ONE widened chunk as wide as the widest widen-route term.  All DRIN_FEAT_F32: the
 * old entry points' bytes and bits. */
DRIN_API size_t drin_table_topk_sum_workspace_bytes_ex(const drin_topk_term* terms, const int32_t* row_dtypes, int32_t num_terms,
                                                       int32_t batch, int64_t num_entities, int32_t k, int64_t chunk_entities,
                                                       int32_t precision);
DRIN_API int drin_table_topk_sum_ex(const drin_topk_term* terms, const int32_t* row_dtypes, int32_t num_terms, int64_t num_entities,
                                    int32_t batch, int32_t k, float cosine_eps, int32_t precision, int64_t chunk_entities, void* workspace,
                                    size_t workspace_bytes, float* out_scores, int64_t* out_rows, void* stream);

/* ---- the image-image edge as a term: the RATIO form ---------------------------------------------------- *
 * model.py:78-92 scores a pair by  ii(b, e) = sum_{i < Km, j < Ke} cos(mobj[b, i], eobj[e, j]) ms[b, i] es[e, j] / (sum_{i, j}
 * ms[b, i] es[e, j] + 1e-9).  Each norm of the cosine is clamped on its own (cosine_from_sums), so the double sum factors into one
 * row per mention and one row per entity:
 *   q[b] = sum_i ms[b, i] mobj[b, i] / max(|mobj[b, i]|, cosine_eps)   S[b] = sum_i ms[b, i]
 *   u[e] = sum_j es[e, j] eobj[e, j] / max(|eobj[e, j]|, cosine_eps)   T[e] = sum_j es[e, j]
 *   ii(b, e) = (q[b] . u[e]) / (S[b] T[e] + 1e-9)          exactly, in real arithmetic
 * - one more product of the kind drin_table_topk_sum runs per chunk, behind a RATIO where a cosine has a product of inverse
 * norms.
 *
 * drin_object_rows replaces the per-pair double loop of model.py:84-92 on either side: out[r, :] = sum_j score[r, j] obj[r, j, :] /
 * max(|obj[r, j, :]|, eps) and mass[r] = sum_j score[r, j] for obj [n, K, width] and score [n, K], both stored as dtype
 * (DRIN_FEAT_F32 | DRIN_FEAT_BF16, read in place and widened exactly: the bits of the fp32 call on the widened values); out
 * [n, width] and mass [n] are fp32.  Per object row one scale score / max(norm, eps) (one fp32 division), then fp32 FMAs into the
 * accumulator and a plain fp32 sum of the scores, both in ascending j.  One wave per output row; every object row is read once
 * (twice past width 2048).  1 <= K <= 16, width % 4 == 0 (% 8 for bf16), eps > 0, n as drin_row_inv_norms; obj and out 16-byte
 * aligned.  No atomics: the same bits every run.  Profiler class DRIN_KC_POOL. */
DRIN_API int drin_object_rows(const void* obj, const void* score, int32_t dtype, int64_t n, int32_t K, int32_t width, float eps,
                              float* out, float* mass, void* stream);

/* The form of term s of a sum: a HOST array parallel to `terms`, like row_dtypes. */
#define DRIN_TOPK_COSINE 0
#define DRIN_TOPK_RATIO 1
typedef struct drin_topk_form { /* form of term s; a NULL array = all DRIN_TOPK_COSINE */
  int32_t form;
  const float* x_mass;   /* RATIO: [batch]         */
  const float* row_mass; /* RATIO: [num_entities]  */
  float eps;             /* RATIO: added to the product of the masses (drin_config.miei_eps = 1e-9f for DRIN) */
} drin_topk_form;

/* out[b, n] = (x[b, :] . rows[index[b, n], :]) / (x_mass[b] * row_mass[index[b, n]] + eps): the re-score of a RATIO term.  The dot
 * product is drin_cosine_rows_indexed_fwd's (fp32 FMA, its lane order and wave sum); then d = x_mass * row_mass, d = d + eps,
 * out = dot / d, each rounded to fp32 on its own with a correctly rounded divide.  x [batch, width], rows [num_entities, width],
 * x_mass [batch], row_mass [num_entities], out [batch, num_candidates]: all fp32.  An index outside [0, num_entities) is clamped
 * before an address is formed from it and reported into index_status (int32[4] or NULL) as drin_cosine_rows_indexed_fwd does.
 * width % 4 == 0, eps finite; x and rows 16-byte aligned; batch, num_candidates as drin_cosine_rows_indexed_fwd.  Two runs give
 * the same bits.  Profiler class DRIN_KC_EDGE. */
DRIN_API int drin_ratio_rows_indexed_fwd(const float* x, const float* x_mass, const float* rows, const float* row_mass,
                                         const int64_t* index, int64_t num_entities, float* out, int32_t batch, int32_t num_candidates,
                                         int32_t width, float eps, int32_t* index_status, void* stream);

/* drin_topk_combine with the form of every term.  forms NULL, or all DRIN_TOPK_COSINE: drin_topk_combine's launch and bits.  A
 * DRIN_TOPK_RATIO term s contributes, per element, d = row_mass[c] * x_mass[b]; d = d + eps; t = blocks[s][c * ld + b] / d;
 * t = t * weights[s]; acc = acc + t (acc = t for term 0) - every operation rounded to fp32 on its own, no contraction, a correctly
 * rounded divide; the cosine terms keep their sequence.  HERE forms[s].x_mass is [ld] (16-byte aligned, all ld entries are read:
 * pad it with zeros) and forms[s].row_mass is [cols], already at the block's first column; col_inv_norms[s] and row_scales[s] of
 * a RATIO term are not read and may be NULL.  Still one launch; out may be blocks[0]. */
DRIN_API int drin_topk_combine_forms(const float* const* blocks, const float* const* col_inv_norms, const float* const* row_scales,
                                     const float* weights, const drin_topk_form* forms, int32_t num_terms, int64_t ld, int32_t batch,
                                     int64_t cols, float* out, void* stream);

/* drin_table_topk_sum_ex with the form of every term: forms, a HOST array [num_terms] or NULL (all DRIN_TOPK_COSINE); row_dtypes
 * may be NULL here (all DRIN_FEAT_F32).  forms NULL or all DRIN_TOPK_COSINE: drin_table_topk_sum_ex's bytes and bits through the
 * same plan - there is no second body.  A DRIN_TOPK_RATIO term contributes weight * (x[b] . rows[e]) / (x_mass[b] * row_mass[e] +
 * eps): its row_inv_norms is not read and may be NULL, its rows are fp32 (a DRIN_FEAT_BF16 entry for it: DRIN_E_UNSUPPORTED among
 * the argument checks), x_mass and row_mass are 4-byte aligned device arrays and eps is finite.  It occupies an ordinary slot of
 * the workspace - its padded mentions, its block, and the per-mention factor region holding x_mass padded to Bp with zeros - so
 * THE WORKSPACE QUERY RETURNS EXACTLY WHAT drin_table_topk_sum_workspace_bytes_ex RETURNS for the same widths, dtypes, batch,
 * num_entities, k, chunk and precision.  Per chunk its product is the GEMM module's choice like any fp32 term's and the one
 * combine is drin_topk_combine_forms'.  The re-score of a RATIO term is drin_ratio_rows_indexed_fwd's bits: out_scores ARE the
 * chain acc = w_0 c_0; acc = acc + w_s c_s of drin_table_topk_sum over those and drin_cosine_rows_indexed_fwd(_ex)'s bits.  The
 * entry of a dropped term (weight 0) is not read. */
DRIN_API size_t drin_table_topk_sum_forms_workspace_bytes(const drin_topk_term* terms, const int32_t* row_dtypes,
                                                          const drin_topk_form* forms, int32_t num_terms, int32_t batch,
                                                          int64_t num_entities, int32_t k, int64_t chunk_entities, int32_t precision);
DRIN_API int drin_table_topk_sum_forms(const drin_topk_term* terms, const int32_t* row_dtypes, const drin_topk_form* forms,
                                       int32_t num_terms, int64_t num_entities, int32_t batch, int32_t k, float cosine_eps,
                                       int32_t precision, int64_t chunk_entities, void* workspace, size_t workspace_bytes,
                                       float* out_scores, int64_t* out_rows, void* stream);

/* ---- DRIN behind a first stage: CLIP edges for run-time candidates and a rerank ---------------- *
 * The two CLIP edges of drin_batch (miet_similarity, mtei_similarity) for candidates that were chosen at run time, from stored
 * CLIP embeddings: replaces preprocess/clip.py:158-172, which computes CLIPModel's logits_per_image / logits_per_text offline
 * per pair of a fixed candidate list - exp(logit_scale) x the cosine of the projected embeddings, the scale that model.py:203
 * divides by again (drin_config.clip_scale).
 *   miet[b, n] = scale * cos(mention_clip_image[b, :], table_clip_text[index[b, n], :])
 *   mtei[b, n] = scale * cos(mention_clip_text[b, :],  table_clip_image[index[b, n], :])
 * mention rows [batch, width], table rows [num_entities, width], index int64 [batch, num_candidates], outputs [batch,
 * num_candidates]; all fp32.  One launch, one read of index per pair.  Every output is, bit for bit, scale * what
 * drin_cosine_rows_indexed_fwd returns for the same rows (one fp32 multiply); a zero row gives 0.  Either edge may be left
 * out: its three pointers (mention rows, table rows, output) NULL together.  index is clamped and reported into index_status
 * (int32[4] or NULL) as the row operations of section 23 do.  The four row pointers are 16-byte aligned, width % 4 == 0,
 * batch 1 .. 65535, num_candidates 1 .. 65535.  Writes miet, mtei and (on a bad index) index_status, nothing else.
 * Profiler class DRIN_KC_EDGE. */
DRIN_API int drin_cross_modal_edges(const float* mention_clip_image, const float* mention_clip_text, const float* table_clip_text,
                                    const float* table_clip_image, const int64_t* index, int64_t num_entities, int32_t batch,
                                    int32_t num_candidates, int32_t width, float scale, float eps, float* miet, float* mtei,
                                    int32_t* index_status, void* stream);
/* The same with both CLIP tables stored as row_dtype (one dtype for both; the mentions' rows stay fp32): a bf16 table links
 * exactly as its exactly-widened fp32 copy would - bit for bit the old entry point on the widened tables.  No product: a row
 * kernel, four table rows in flight per wave as before. */
DRIN_API int drin_cross_modal_edges_ex(const float* mention_clip_image, const float* mention_clip_text, const void* table_clip_text,
                                       const void* table_clip_image, int32_t row_dtype, const int64_t* index, int64_t num_entities,
                                       int32_t batch, int32_t num_candidates, int32_t width, float scale, float eps, float* miet,
                                       float* mtei, int32_t* index_status, void* stream);

/* Per mention, the first k of n (score, row) pairs - scores [batch, n], rows int64 [batch, n] - under THE ORDERING CONTRACT
 * above, with one rule added because a caller's candidate list may name a row twice: between equal scores on equal rows, the
 * lower slot (column of the input) ranks first.  out_scores [batch, k] come back canonical, as drin_topk_update returns its
 * keys (+0.0 for -0.0, one quiet NaN); out_rows int64 [batch, k]; out_slots int32 [batch, k] - the column of each returned
 * pair in the input - may be NULL.  One workgroup per mention, a bitonic sort in LDS.  1 <= k <= n <= 4096, batch 1 .. 65535;
 * rows of any int64 value.  Writes the three outputs, nothing else. */
DRIN_API int drin_rank_rows(const float* scores, const int64_t* rows, int32_t batch, int32_t n, int32_t k, float* out_scores,
                            int64_t* out_rows, int32_t* out_slots, void* stream);

/* ---- activation, row dropout and the span mean (GHMFC's other mention encoders) ---------------- *
 * What nn.TransformerEncoderLayer runs beside its products, attention and LayerNorms (ghmfc.py:72-90), and Avg.avg
 * (ghmfc.py:54-60) as an entry point of its own.  Checked on the host before a launch like the row operations above. */

/* Activation codes of drin_act_dropout_*: NOT drin_activation (whose 0 means "the reference's default"). */
typedef enum {
  DRIN_ROW_ACT_NONE = 0, /* identity: plain dropout                                   */
  DRIN_ROW_ACT_RELU = 1, /* max(x, 0), relu'(0) = 0; a NaN passes, as torch.relu     */
  DRIN_ROW_ACT_GELU = 2  /* exact-erf gelu, the expressions of the gate              */
} drin_row_activation;

/* y = act(x) m / (1 - p), element-wise over [rows, width] contiguous floats (width % 4 == 0, 16-byte aligned pointers, any
 * rows >= 1).  m is the keep mask of drin_attention_dropout_keep(seed, call, rows, 1, 1, width, p, ...): element
 * (row, col) is element row * width + col of csrc/dropout_mask.h.  A dropped element is exactly 0 (a NaN there too).
 * p = 0: no mask, the plain activation's bits; p outside [0, 1), a NaN too: DRIN_E_SHAPE; an unknown act: DRIN_E_SHAPE.
 * y may be x.  Profiler class DRIN_KC_NORM. */
DRIN_API int drin_act_dropout_fwd(const float* x, float* y, int64_t rows, int32_t width, int32_t act, float p, uint64_t seed,
                                  uint64_t call, void* stream);
/* dx = dy act'(x) m / (1 - p) with act' recomputed from the forward's x and the same (p, seed, call).  With
 * DRIN_ROW_ACT_NONE x is not read and may be NULL: the forward applied to dy, bit for bit.  dx may be dy. */
DRIN_API int drin_act_dropout_bwd(const float* x, const float* dy, float* dx, int64_t rows, int32_t width, int32_t act, float p,
                                  uint64_t seed, uint64_t call, void* stream);

/* out[b, :] = mean(seq[b, start[b] : end[b], :]) with Python's slice clipping (negative positions count from seq_len, the
 * range is cut to [0, seq_len]); seq [batch, seq_len, width], start, end int64 [batch].  An empty range gives a NaN row, as
 * torch.mean of an empty slice.  The bits of drin_edges_fwd's span mean.  Profiler class DRIN_KC_POOL. */
DRIN_API int drin_span_mean_fwd(const float* seq, const int64_t* start, const int64_t* end, float* out, int32_t batch,
                                int32_t seq_len, int32_t width, void* stream);
/* dseq [batch, seq_len, width], every element written: dout[b, :] / (end - start) on the rows of the clipped range, exactly
 * 0 elsewhere; an empty range gives a block of zeros. */
DRIN_API int drin_span_mean_bwd(const float* dout, const int64_t* start, const int64_t* end, float* dseq, int32_t batch,
                                int32_t seq_len, int32_t width, void* stream);

/* ---- DRIN's other mention encoders: the representation head ---------------------------------- *
 * Reference: common/args.py:28-29 (mention_final_layer_name "linear" | "transformer" | "none", mention_final_representation),
 * baselines/ghmfc.py:54-70 (Avg, MaxPool), :152-199 (MentionEncoder(inline_bert=False)), drin/model.py:21,58,71-76.  With
 * "none" / "transformer" the mention-text vertex is repr(intermediate(mention_text)) with no Linear behind it, and the
 * text-text edge takes repr(mention_text) of the RAW block; repr is the mean over the mention span or the max over all L
 * positions (padded ones take part; neither the mask nor the span is read).  The intermediate layer (the transformer stack)
 * is the caller's: its output travels as `encoded`. */
typedef enum {
  DRIN_MENTION_LINEAR = 0, /* mt0 = span mean W_mt^T + b_mt: what the entry points without a head compute   */
  DRIN_MENTION_ROWS = 1    /* mt0 = repr(encoded, or mention_text itself), no Linear                         */
} drin_mention_encoder;
typedef enum {
  DRIN_REPR_AVG_EXTRACT = 0, /* Avg.avg (ghmfc.py:54-60): Python slice clipping, an empty span gives a NaN row */
  DRIN_REPR_MAX_POOL = 1     /* MaxPool (ghmfc.py:63-70): a NaN wins, the lowest position attains a tie        */
} drin_mention_repr;
/* Additive under ABI 12: no existing struct changes; the settings travel here, with the struct's own size. */
typedef struct drin_mention_head {
  size_t struct_size;     /* sizeof(drin_mention_head)                                                                      */
  int32_t encoder;        /* drin_mention_encoder                                                                           */
  int32_t representation; /* drin_mention_repr; DRIN_MENTION_LINEAR takes DRIN_REPR_AVG_EXTRACT only (args.py:12-13)        */
  const float* encoded;   /* [B, L, D] fp32: the intermediate layer's output, or NULL = mention_text itself; ROWS only      */
  int32_t* max_index;     /* [2][B, D] (edge row, vertex row), caller-owned, written by forward, read by backward; MAX_POOL */
  float* grad_encoded;    /* backward: [B, L, D], WRITTEN; NULL = not wanted                                                */
} drin_mention_head;

/* drin_forward_staged with a mention head.  head NULL or {DRIN_MENTION_LINEAR, DRIN_REPR_AVG_EXTRACT, NULL}: exactly
 * drin_forward_staged (the same launches, the same bits).  DRIN_MENTION_ROWS: params->w_mention_text / b_mention_text are not
 * read and may be NULL; the edge row lives where the span mean lives and the vertex row goes straight into the layer-0
 * mention-text vertex, so workspace sizes and layouts are those of drin_workspace_bytes.  Vector edges, static edges,
 * edge_enabled, every activation and num_layers = 0 work under a head: it ends at the span-mean row and the layer-0 vertex.
 * DRIN_E_SHAPE: struct_size, an unknown encoder / representation, `encoded` under LINEAR, grad_encoded without encoded;
 * DRIN_E_UNSUPPORTED: {LINEAR, MAX_POOL} (args.py:12-13 forces avg extract for "linear"); DRIN_E_NULL: max_index under MAX_POOL. */
DRIN_API int drin_forward_staged_head(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                                      size_t workspace_bytes, float* scores, int keep_for_backward, const drin_trace* trace,
                                      void* params_ready_event, const drin_mention_head* head, void* stream);
/* drin_backward_ex with the head of the forward pass (the same encoder, representation, encoded and max_index).  Under
 * DRIN_MENTION_ROWS grads->w_mention_text / b_mention_text are never written.  Works with grads only, input_grads only or
 * both: head->grad_encoded (the gradient of `encoded`, what the caller's intermediate layer backpropagates) is written
 * whenever it is non-NULL.  With input_grads->mention_text wanted too, the text-text edge's term goes to the raw block and
 * the vertex's term to the encoded block; with encoded == NULL both terms land in input_grads->mention_text in one write.
 * num_layers = 0: the score reads the vertex alone and the raw block's edge term is zero. */
DRIN_API int drin_backward_head(const drin_config* cfg, const drin_batch* batch, const drin_params* params, void* workspace,
                                size_t workspace_bytes, const float* grad_scores, const drin_param_grads* grads,
                                const drin_input_grads* input_grads, void* layers_ready_event, const drin_mention_head* head,
                                void* stream);

/* drin_forward_prepared (the folded two-layer inference path) with a mention head; NULL or {LINEAR, AVG_EXTRACT}: its bits.
 * DRIN_MENTION_ROWS: the head runs k_mention_rows and the mention-image product alone; with cfg.feature_dtype = DRIN_FEAT_BF16
 * the raw block is read as bf16 (head->encoded stays fp32).  drin_prepare accepts params->w_mention_text == NULL for such a
 * model (and no other NULL weight: DRIN_E_NULL) and zeroes that plane: a prepared buffer built without the Linear belongs to
 * DRIN_MENTION_ROWS calls - passed with a NULL / LINEAR head it scores with a zero mention-text weight, silently.  drin_forward_cached takes no head (the per-entity cache is not built for these encoders). */
DRIN_API int drin_forward_prepared_head(const drin_config* cfg, const drin_batch* batch, const drin_params* params,
                                        const void* prepared, void* workspace, size_t workspace_bytes, float* scores,
                                        const drin_mention_head* head, void* stream);

/* The head's forward kernel on its own: edge_row [batch, width] = repr(raw), vertex_row [batch, width] = repr(encoded), or the
 * edge row's values when encoded is NULL (the block is read once).  raw [batch, seq_len, width] is fp32 (raw_dtype =
 * DRIN_FEAT_F32) or bf16 (DRIN_FEAT_BF16: widened exactly); encoded is fp32.  DRIN_REPR_AVG_EXTRACT reads start / end (int64
 * [batch], drin_span_mean_fwd's clipping; an empty span gives NaN rows) and ignores max_index; DRIN_REPR_MAX_POOL ignores
 * start / end and writes max_index [2][batch, width] (edge row's positions, then the vertex row's) with
 * drin_seq_max_train_fwd's bits and positions.  16-byte aligned pointers, width % 4 == 0.  Profiler class DRIN_KC_POOL. */
DRIN_API int drin_mention_rows_fwd(const void* raw, int32_t raw_dtype, const float* encoded, const int64_t* start,
                                   const int64_t* end, int32_t representation, float* edge_row, float* vertex_row,
                                   int32_t* max_index, int32_t batch, int32_t seq_len, int32_t width, void* stream);
/* Its backward: grad_raw and grad_encoded [batch, seq_len, width], every element of a non-NULL one written exactly once (no
 * atomics: the same bits every run).  An element receives g / (end - start) inside the clipped span (avg; an empty span
 * passes zeros) or g where its position is max_index's (max), exactly 0 elsewhere.  has_encoded != 0: grad_raw takes
 * g_edge_row's term, grad_encoded g_vertex_row's; has_encoded == 0: grad_raw takes the sum of both terms and grad_encoded
 * must be NULL.  g_edge_row / g_vertex_row [batch, width] may be NULL (that row passes no gradient); either destination may
 * be NULL. */
DRIN_API int drin_mention_rows_bwd(const float* g_edge_row, const float* g_vertex_row, const int64_t* start, const int64_t* end,
                                   const int32_t* max_index, int32_t representation, int32_t has_encoded, float* grad_raw,
                                   float* grad_encoded, int32_t batch, int32_t seq_len, int32_t width, void* stream);

/* ---- gradient x input attribution (attribution_kernels.hip) ------------- */

/* The contraction that stands where drin_pool_bwd expands: of the token block's gradient x input, summed over the width, only the
 * terms the entity pooling passes a gradient to (ghmfc.py:245-249: entity_text_feature[1:ntok-1] with ntok = sum(mask), then the
 * mean over the slice; drin_pool_bwd's share g / cnt):
 *   out[p, t] = <tokens[row, t, :], grad_pooled[p, :]> / cnt   for 1 <= t <= cnt,   cnt = ntok - 2  (ntok == 0: the slice's -1
 *   stop, cnt = T - 2),   exactly 0.0f elsewhere - token 0 too: it feeds only the text-text cosine (model.py:73-75), which is
 *   homogeneous of degree 0 in that row, so its gradient x input is 0.
 * tokens is [pairs, T, width] (row = p) or, with entity_index != NULL, a table [num_entities, T, width] read at row
 * entity_index[p] (int64 [pairs]); mask (int64) has the same leading shape and is read through the same index.  A row outside
 * [0, num_entities) is clamped before anything is read and reported in index_status (int32[4] or NULL: drin_batch.index_status'
 * convention).  token_dtype: DRIN_FEAT_F32 or DRIN_FEAT_BF16 (widened exactly); grad_pooled [pairs, width] and out [pairs, T] are
 * fp32.  Every element of out is WRITTEN; rows outside the kept slice are never loaded; a pair with an empty slice (ntok 1 or 2)
 * gets a row of zeros; a NaN or an infinity in grad_pooled reaches the kept tokens of its own pair only.  No atomics: the same
 * bits every run.  16-byte aligned tokens / grad_pooled / out, width % 4 == 0 (bf16: % 8), T >= 1, pairs >= 0 (any count: the
 * launches are sliced).  Profiler class DRIN_KC_POOL. */
DRIN_API int drin_token_attribution(const void* tokens, int32_t token_dtype, const int64_t* mask, const int64_t* entity_index,
                                    int64_t num_entities, int32_t* index_status, const float* grad_pooled, float* out,
                                    int64_t pairs, int32_t T, int32_t width, void* stream);

/* out[r] = sum_c x[r, c] g[r, c]: what (x * x.grad).sum(-1) gives for every other feature of the batch (mention tokens, image
 * regions, image rows with their inner dims flattened into the row, pooled entity text).  x [rows, width] fp32 or bf16
 * (x_dtype, widened exactly), g [rows, width] and out [rows] fp32.  One wave per row up to width 2048, a workgroup per row above;
 * fixed summation order: the same bits every run.  16-byte aligned x / g, width % 4 == 0 (bf16: % 8), 0 <= rows <= 2^31.
 * Profiler class DRIN_KC_POOL. */
DRIN_API int drin_rows_dot(const void* x, int32_t x_dtype, const float* g, float* out, int64_t rows, int32_t width, void* stream);

/* ---- in-process kernel timing (bench.py's roofline leg) ---------------------------------------- */

/* Kernel classes the launches are attributed to. */
typedef enum {
  DRIN_KC_GEMM = 0,   /* k_gemm_f32: exact fp32 MFMA contractions (all backward products too)     */
  DRIN_KC_POOL = 1,   /* input pooling: span / region / token means                               */
  DRIN_KC_EDGE = 2,   /* static edge builders: cosine rows, miei, scaling                          */
  DRIN_KC_GCN = 3,    /* aggregation, LayerNorm+GELU, edge update, their backward                  */
  DRIN_KC_STREAM = 4, /* k_entity_stream / k_cached_pairs: the single HBM-bound pass over entity bytes  */
  DRIN_KC_GEMM_X3 = 5,     /* k_gemm_bf16x3: split-bf16 contraction, fp32 operands split on the fly */
  DRIN_KC_GEMM_PLANES = 6, /* k_gemm_x3_planes: split-bf16 contraction on pre-split planes (LDS-DMA) */
  DRIN_KC_OPTIM = 7,       /* drin_adam_step                                                        */
  DRIN_KC_LSTM = 8,        /* drin_melhi_*: one step of the long LSTM recurrences (forward or backward) */
  DRIN_KC_CELL = 9,        /* drin_melhi_*: mask, time-0 cells, gathers and their backward           */
  DRIN_KC_ATTN = 10,       /* drin_attention* / drin_ghmfc_forward: the softmax-attention core and its backward */
  DRIN_KC_NORM = 11,       /* drin_ghmfc_forward and the row-op entry points: LayerNorm (+ residual), max over a sequence, the gate, activation + row dropout, their backward */
  DRIN_KC_COUNT = 12
} drin_kernel_class;

/* While a profile is open, every launch the library makes - from any thread, e.g. drin_backward on
 * autograd's thread - is bracketed by hipEvents on its stream.  drin_profile_end synchronises those
 * events, returns per-class GPU milliseconds and launch counts (arrays of DRIN_KC_COUNT) and closes the
 * profile.  One profile per process at a time; this is the library's only process-wide state and it is
 * inert unless a profile is open.  The loss kernels (drin_triplet_topk) count under DRIN_KC_EDGE.  The events belong to the
 * device that is current when drin_profile_begin runs: a profile times the calls whose streams live on THAT device (launches on
 * another device run untimed - their results are unaffected). */
DRIN_API int drin_profile_begin(int max_launches);
DRIN_API int drin_profile_end(double* ms_by_class, int64_t* launches_by_class);
DRIN_API const char* drin_kernel_class_name(int kernel_class);

#ifdef __cplusplus
}
#endif
#endif /* DRIN_HIP_H_ */
