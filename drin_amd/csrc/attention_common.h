// What the two softmax-attention cores share on the host side: the FMA core of attention_fma.hip (DESIGN.md sections 15,
// 16, 18) and the matrix-core one of attention_mfma.hip (section 21).  The domain, the dropout arguments, one attention call
// as a struct, and the launchers of both cores, which take it.  The entry points and their checks: attention_api.hip.
#pragma once
#include "dropout_mask.h"
#include "internal.h"

namespace drin {

constexpr int kAttnMaxDh = 256, kAttnMaxLk = 512;

// DROP instantiations of the attention kernels: the weight of (query i, key j) that goes into p V is multiplied by
// keep / (1 - rate) (dropout_mask.h); the running max, the sum l and lse are those of the undropped scores.
struct DropArgs {
  uint32_t threshold;   // dropout_threshold(rate)
  float scale;          // 1 / (1 - rate)
  uint64_t seed, call;
};

// One call of an attention core.  Rows of head h of mention b, position i start at ptr + (b * L + i) * ld + h * dh.
// The forward writes out and lse (lse may be NULL where the entry point allows it); the backward only reads them.
struct AttnCall {
  const float* q; int64_t ldq;
  const float* k; int64_t ldk;
  const float* v; int64_t ldv;
  const int64_t* mask;            // [B, Lk], 0 drops the key; NULL keeps every key
  float* out; int64_t ldo;
  float* lse;                     // [B, H, Lq]
  int B, H, Lq, Lk, dh;
  // the backward alone: dq may be NULL (skipped); dk and dv are both given or both NULL; delta: [B, H, Lq] floats of scratch
  const float* dout = nullptr; int64_t lddo = 0;
  float* dq = nullptr; int64_t lddq = 0;
  float* dk = nullptr; int64_t lddk = 0;
  float* dv = nullptr; int64_t lddv = 0;
  float* delta = nullptr;
};

inline int check_attention_shape(const char* who, int64_t B, int H, int Lq, int Lk, int dh) {
  if (B < 1 || B > kMaxGridY || H < 1 || H > kMaxGridY || Lq < 1 || Lk < 1 || Lk > kAttnMaxLk || dh < 1 || dh > kAttnMaxDh) {
    set_error("%s: batch and heads in [1, %d], q_len >= 1, k_len in [1, %d], head_dim in [1, %d] (got B=%lld H=%d Lq=%d Lk=%d dh=%d)",
              who, kMaxGridY, kAttnMaxLk, kAttnMaxDh, (long long)B, H, Lq, Lk, dh);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

// rate in [0, 1) -> the kernels' arguments; a rate of 0 is the plain path (use = false): the undropped entry points' bits
inline int dropout_args(const char* who, float p, uint64_t seed, uint64_t call, DropArgs* out, bool* use) {
  if (!(p >= 0.f && p < 1.f)) {
    set_error("%s: dropout rate %g is not in [0, 1)", who, (double)p);
    return DRIN_E_SHAPE;
  }
  *use = p > 0.f;
  *out = DropArgs{dropout_threshold(p), 1.0f / (1.0f - p), seed, call};
  return DRIN_OK;
}

// The launchers check nothing: shape, pointers and strides are the caller's (attention_api.hip: attention_forward /
// attention_backward; ghmfc_forward.hip: validate_ghmfc_config).  drop: NULL is the plain path.
// attention_fma.hip
int launch_attention(const AttnCall& c, const DropArgs* drop, hipStream_t st);
int launch_attention_bwd(const AttnCall& c, const DropArgs* drop, hipStream_t st);
// delta [B, H, Lq] of both backwards, one wave per (mention, head, query row) (k_attention_bwd_delta)
int launch_attention_bwd_delta(const AttnCall& c, hipStream_t st);
// attention_mfma.hip
int launch_attention_mfma(const AttnCall& c, const DropArgs* drop, hipStream_t st);
int launch_attention_mfma_bwd(const AttnCall& c, const DropArgs* drop, hipStream_t st);

}  // namespace drin
