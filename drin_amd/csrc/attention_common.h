// What the two softmax-attention cores share on the host side: the FMA core of ghmfc_kernels.hip (DESIGN.md sections 15,
// 16, 18) and the matrix-core one of attention_mfma.hip (section 21).  The domain, the dropout arguments and the launcher of
// the row statistic delta_i = sum_c dO[i, c] O[i, c], which both backwards read.
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

inline int check_attention_shape(int64_t B, int H, int Lq, int Lk, int dh) {
  if (B < 1 || B > 65535 || H < 1 || H > 65535 || Lq < 1 || Lk < 1 || Lk > kAttnMaxLk || dh < 1 || dh > kAttnMaxDh) {
    set_error("attention: batch and heads in [1, 65535], q_len >= 1, k_len in [1, %d], head_dim in [1, %d] (got B=%lld H=%d Lq=%d Lk=%d dh=%d)",
              kAttnMaxLk, kAttnMaxDh, (long long)B, H, Lq, Lk, dh);
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

// delta [B, H, Lq] of the backward, one wave per (mention, head, query row) (k_attention_bwd_delta, ghmfc_kernels.hip)
int launch_attention_bwd_delta(const float* out, int64_t ldo, const float* dout, int64_t lddo, float* delta, int B, int H, int Lq,
                               int dh, hipStream_t st);

}  // namespace drin
