// Host-side argument checks of drin_gemm_probe (include/drin_hip.h): plain C++, no HIP - tests/host/gemm_probe_check_main.cpp
// runs them as a stand-alone program under ASan / UBSan.  Nothing here dereferences an operand: only the struct itself is read.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/drin_hip.h"

namespace drin {

// DRIN_OK, or the status to return with its message in msg
inline int gemm_probe_check(const drin_gemm_probe_args* a, char* msg, size_t msg_len) {
  auto fail = [&](int status, const char* what) {
    snprintf(msg, msg_len, "drin_gemm_probe: %s", what);
    return status;
  };
  if (msg_len > 0) msg[0] = 0;
  if (a == nullptr) return fail(DRIN_E_NULL, "NULL argument struct");
  if (a->struct_size != sizeof(drin_gemm_probe_args)) {
    snprintf(msg, msg_len, "drin_gemm_probe: struct_size %zu, this library's drin_gemm_probe_args has %zu", a->struct_size,
             sizeof(drin_gemm_probe_args));
    return DRIN_E_SHAPE;
  }
  if (a->op < DRIN_PROBE_GEMM_NT || a->op > DRIN_PROBE_TO_F16_SCALED) {
    snprintf(msg, msg_len, "drin_gemm_probe: unknown op %d", a->op);
    return DRIN_E_UNSUPPORTED;
  }
  if (a->scratch == nullptr && a->scratch_floats > 0) return fail(DRIN_E_NULL, "scratch_floats without a scratch (NULL)");
  if (a->op == DRIN_PROBE_TO_F16_SCALED) {
    if (!a->a || !a->y || !a->scratch) return fail(DRIN_E_NULL, "to_f16_scaled needs a, y and the two-float scale buffer (NULL)");
    if (a->rows < 0 || a->scratch_floats < 2) return fail(DRIN_E_SHAPE, "to_f16_scaled: negative count, or a scale buffer below two floats");
    return DRIN_OK;
  }
  bool null_operand = !a->a || !a->y;
  switch (a->op) {
    case DRIN_PROBE_GEMM_NT: null_operand = null_operand || !a->b; break;
    case DRIN_PROBE_GEMM_NT_BF16X3: null_operand = null_operand || (!a->b && !(a->b_hi && a->b_lo)); break;
    case DRIN_PROBE_GEMM_NT_BF16X3_P4:
    case DRIN_PROBE_GEMM_X3_PLANES: null_operand = null_operand || !a->b_hi || !a->b_lo; break;
    default: null_operand = null_operand || !a->b_hi || !a->row_scale || !a->b_scale; break;   // DRIN_PROBE_GEMM_F16_PLANES
  }
  if (null_operand) return fail(DRIN_E_NULL, "a required operand of this op is NULL");
  if (a->rows < 0 || a->n_out <= 0 || a->k <= 0) {
    snprintf(msg, msg_len, "drin_gemm_probe: bad shape rows=%lld n_out=%d k=%d", (long long)a->rows, a->n_out, a->k);
    return DRIN_E_SHAPE;
  }
  if (a->lda < a->k || a->ldb < a->k || a->ldy < a->n_out) {
    snprintf(msg, msg_len, "drin_gemm_probe: leading dimensions lda=%lld ldb=%lld (rows of %d) ldy=%lld (rows of %d)", (long long)a->lda,
             (long long)a->ldb, a->k, (long long)a->ldy, a->n_out);
    return DRIN_E_SHAPE;
  }
  if (a->row_tile_begin < 0 || a->row_tile_wgs < 0) return fail(DRIN_E_SHAPE, "negative row tile or workgroup count");
  const bool sliced = a->row_tile_begin != 0 || a->row_tile_end >= 0 || a->row_tile_wgs != 0;
  if (sliced && a->op != DRIN_PROBE_GEMM_NT_BF16X3_P4 && a->op != DRIN_PROBE_GEMM_X3_PLANES)
    return fail(DRIN_E_UNSUPPORTED, "a slice of row tiles exists on the four-phase launchers only");
  if (a->a_index != nullptr && a->op != DRIN_PROBE_GEMM_NT_BF16X3) return fail(DRIN_E_UNSUPPORTED, "indexed rows: launch_gemm_nt_bf16x3 only");
  return DRIN_OK;
}

}  // namespace drin
