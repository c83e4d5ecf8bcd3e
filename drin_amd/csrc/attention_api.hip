// The entry points of the two softmax-attention cores (attention_fma.hip, attention_mfma.hip) and their host-side checks,
// each written once: an entry point fills an AttnCall (attention_common.h), names its core and goes through
// attention_forward / attention_backward.  Host code only.
#include "attention_common.h"

namespace drin {
namespace {

enum AttnCore { kFma, kMfma };

// every row stride that the call reads is >= heads * head_dim; the stride of an absent gradient is not looked at
int check_strides(const char* who, const AttnCall& c, bool backward) {
  const int64_t E = (int64_t)c.H * c.dh;
  const struct { const char* name; int64_t ld; bool used; } strides[] = {
      {"ldq", c.ldq, true}, {"ldk", c.ldk, true}, {"ldv", c.ldv, true}, {"ldo", c.ldo, true}, {"lddo", c.lddo, backward},
      {"lddq", c.lddq, c.dq != nullptr}, {"lddk", c.lddk, c.dk != nullptr}, {"lddv", c.lddv, c.dv != nullptr}};
  for (const auto& s : strides)
    if (s.used && s.ld < E) {
      set_error("%s: row stride %s = %lld must be >= heads * head_dim = %lld", who, s.name, (long long)s.ld, (long long)E);
      return DRIN_E_SHAPE;
    }
  return DRIN_OK;
}

// p = 0 is the plain path (the entry points without a rate pass it): the undropped instantiations, seed and call unread
int attention_forward(const char* who, AttnCore core, const AttnCall& c, bool lse_required, float p, uint64_t seed, uint64_t call,
                      void* stream) {
  DropArgs drop;
  bool use;
  DRIN_TRY(dropout_args(who, p, seed, call, &drop, &use));
  DRIN_TRY(check_attention_shape(who, c.B, c.H, c.Lq, c.Lk, c.dh));
  if (!c.q || !c.k || !c.v || !c.out || (lse_required && !c.lse)) {
    set_error("%s: q / k / v / out%s is NULL", who, lse_required ? " / lse" : "");
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_strides(who, c, false));
  DRIN_BIND_DEVICE(stream, c.out, who);
  return (core == kMfma ? launch_attention_mfma : launch_attention)(c, use ? &drop : nullptr, (hipStream_t)stream);
}

int attention_backward(const char* who, AttnCore core, const AttnCall& c, float p, uint64_t seed, uint64_t call, void* stream) {
  DropArgs drop;
  bool use;
  DRIN_TRY(dropout_args(who, p, seed, call, &drop, &use));
  DRIN_TRY(check_attention_shape(who, c.B, c.H, c.Lq, c.Lk, c.dh));
  if (!c.q || !c.k || !c.v || !c.out || !c.lse || !c.dout || !c.delta) {
    set_error("%s: q / k / v / out / lse / dout / delta_scratch is NULL", who);
    return DRIN_E_NULL;
  }
  if ((c.dk == nullptr) != (c.dv == nullptr)) {
    set_error("%s: dk and dv are both given or both NULL (dk %s, dv %s)", who, c.dk ? "given" : "NULL", c.dv ? "given" : "NULL");
    return DRIN_E_NULL;
  }
  DRIN_TRY(check_strides(who, c, true));
  if (!c.dq && !c.dk) return DRIN_OK;
  DRIN_BIND_DEVICE(stream, c.delta, who);
  return (core == kMfma ? launch_attention_mfma_bwd : launch_attention_bwd)(c, use ? &drop : nullptr, (hipStream_t)stream);
}

}  // namespace
}  // namespace drin

using namespace drin;

// the arguments every forward / backward entry point has, in the header's names
#define DRIN_ATTN_FWD_CALL(lse) \
  AttnCall { q, ldq, k, ldk, v, ldv, key_mask, out, ldo, lse, batch, num_heads, q_len, k_len, head_dim }
#define DRIN_ATTN_BWD_CALL                                                                                                   \
  AttnCall {                                                                                                                 \
    q, ldq, k, ldk, v, ldv, key_mask, const_cast<float*>(out), ldo, const_cast<float*>(lse), batch, num_heads, q_len, k_len,  \
        head_dim, dout, lddo, dq, lddq, dk, lddk, dv, lddv, delta_scratch                                                    \
  }

int drin_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const int64_t* key_mask,
                   float* out, int64_t ldo, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim,
                   void* stream) {
  return attention_forward("drin_attention", kFma, DRIN_ATTN_FWD_CALL(nullptr), false, 0.f, 0, 0, stream);
}

int drin_attention_train_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                             const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch, int32_t num_heads,
                             int32_t q_len, int32_t k_len, int32_t head_dim, void* stream) {
  return attention_forward("drin_attention_train_fwd", kFma, DRIN_ATTN_FWD_CALL(lse), true, 0.f, 0, 0, stream);
}

int drin_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const int64_t* key_mask,
                       const float* out, int64_t ldo, const float* lse, const float* dout, int64_t lddo, float* dq, int64_t lddq,
                       float* dk, int64_t lddk, float* dv, int64_t lddv, float* delta_scratch, int32_t batch, int32_t num_heads,
                       int32_t q_len, int32_t k_len, int32_t head_dim, void* stream) {
  return attention_backward("drin_attention_bwd", kFma, DRIN_ATTN_BWD_CALL, 0.f, 0, 0, stream);
}

int drin_attention_dropout_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                               const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch, int32_t num_heads,
                               int32_t q_len, int32_t k_len, int32_t head_dim, float p, uint64_t seed, uint64_t call, void* stream) {
  return attention_forward("drin_attention_dropout_fwd", kFma, DRIN_ATTN_FWD_CALL(lse), true, p, seed, call, stream);
}

int drin_attention_dropout_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                               const int64_t* key_mask, const float* out, int64_t ldo, const float* lse, const float* dout,
                               int64_t lddo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv,
                               float* delta_scratch, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim,
                               float p, uint64_t seed, uint64_t call, void* stream) {
  return attention_backward("drin_attention_dropout_bwd", kFma, DRIN_ATTN_BWD_CALL, p, seed, call, stream);
}

int drin_attention_mfma_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                            const int64_t* key_mask, float* out, int64_t ldo, float* lse, int32_t batch, int32_t num_heads,
                            int32_t q_len, int32_t k_len, int32_t head_dim, float p, uint64_t seed, uint64_t call, void* stream) {
  return attention_forward("drin_attention_mfma_fwd", kMfma, DRIN_ATTN_FWD_CALL(lse), false, p, seed, call, stream);
}

int drin_attention_mfma_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                            const int64_t* key_mask, const float* out, int64_t ldo, const float* lse, const float* dout, int64_t lddo,
                            float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, float* delta_scratch,
                            int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len, int32_t head_dim, float p, uint64_t seed,
                            uint64_t call, void* stream) {
  return attention_backward("drin_attention_mfma_bwd", kMfma, DRIN_ATTN_BWD_CALL, p, seed, call, stream);
}

int drin_attention_dropout_keep(uint64_t seed, uint64_t call, int32_t batch, int32_t num_heads, int32_t q_len, int32_t k_len, float p,
                                uint8_t* keep_host) {
  const char* who = "drin_attention_dropout_keep";
  DropArgs drop;
  bool use;
  DRIN_TRY(dropout_args(who, p, seed, call, &drop, &use));
  if (batch < 1 || num_heads < 1 || q_len < 1 || k_len < 1) {
    set_error("%s: batch, heads, q_len and k_len must be >= 1 (got %d, %d, %d, %d)", who, batch, num_heads, q_len, k_len);
    return DRIN_E_SHAPE;
  }
  if (!keep_host) {
    set_error("%s: keep_host is NULL", who);
    return DRIN_E_NULL;
  }
  const uint64_t n = (uint64_t)batch * num_heads * q_len * k_len;
  for (uint64_t e = 0; e < n; ++e) keep_host[e] = dropout_keep(seed, call, e, drop.threshold) ? 1 : 0;
  return DRIN_OK;
}
