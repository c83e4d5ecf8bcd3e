// Host-side argument checks of drin_wgrad_probe (include/drin_hip.h): plain C++, no HIP - tests/host/wgrad_probe_check_main.cpp
// runs them as a stand-alone program under ASan / UBSan.  Nothing here dereferences an operand: only the struct itself is read.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/drin_hip.h"

namespace drin {

// DRIN_OK, or the status to return with its message in msg
inline int wgrad_probe_check(const drin_wgrad_probe_args* a, char* msg, size_t msg_len) {
  auto fail = [&](int status, const char* what) {
    snprintf(msg, msg_len, "drin_wgrad_probe: %s", what);
    return status;
  };
  if (msg_len > 0) msg[0] = 0;
  if (a == nullptr) return fail(DRIN_E_NULL, "NULL argument struct");
  if (a->struct_size != sizeof(drin_wgrad_probe_args)) {
    snprintf(msg, msg_len, "drin_wgrad_probe: struct_size %zu, this library's drin_wgrad_probe_args has %zu", a->struct_size,
             sizeof(drin_wgrad_probe_args));
    return DRIN_E_SHAPE;
  }
  if (a->op < DRIN_WGRAD_TN_GROUP || a->op > DRIN_WGRAD_NN) {
    snprintf(msg, msg_len, "drin_wgrad_probe: unknown op %d", a->op);
    return DRIN_E_UNSUPPORTED;
  }
  if (a->n_products < 1 || a->n_products > DRIN_WGRAD_PROBE_MAX) {
    snprintf(msg, msg_len, "drin_wgrad_probe: %d products, 1 to %d fit the struct", a->n_products, DRIN_WGRAD_PROBE_MAX);
    return DRIN_E_SHAPE;
  }
  const bool single = a->op == DRIN_WGRAD_TN || a->op == DRIN_WGRAD_NN;
  if (single && a->n_products != 1) return fail(DRIN_E_SHAPE, "this op takes one product");
  if (a->scratch == nullptr && a->scratch_floats > 0) return fail(DRIN_E_NULL, "scratch_floats without a scratch (NULL)");
  if (a->op == DRIN_WGRAD_NN) {
    if (a->wt_form < DRIN_WGRAD_WT_NONE || a->wt_form > DRIN_WGRAD_WT_PLANES) return fail(DRIN_E_UNSUPPORTED, "unknown wt_form");
    if (a->wt_form != DRIN_WGRAD_WT_NONE && a->wt == nullptr) return fail(DRIN_E_NULL, "a wt_form without memory for W^T (NULL)");
  }
  if (a->op == DRIN_WGRAD_PASS && a->layers_done_after >= a->n_products) return fail(DRIN_E_SHAPE, "layers_done_after names no product");
  for (int i = 0; i < a->n_products; ++i) {
    const drin_wgrad_product& p = a->product[i];
    const bool sums_only = a->op == DRIN_WGRAD_COLSUM_BATCH;
    // the pass takes a product without dw (a bias gradient alone) or without db; every other op needs what it writes
    const bool need_dw = !sums_only && a->op != DRIN_WGRAD_PASS, need_db = sums_only;
    if (!p.dy || (!sums_only && !p.x) || (need_dw && !p.dw) || (need_db && !p.db) || (a->op == DRIN_WGRAD_PASS && !p.dw && !p.db)) {
      snprintf(msg, msg_len, "drin_wgrad_probe: product %d: a required operand of this op is NULL", i);
      return DRIN_E_NULL;
    }
    if (p.rows < 0 || p.n_out <= 0 || p.k <= 0) {
      snprintf(msg, msg_len, "drin_wgrad_probe: product %d: bad shape rows=%lld n_out=%d k=%d", i, (long long)p.rows, p.n_out, p.k);
      return DRIN_E_SHAPE;
    }
    // TN: dy [rows][n_out], x [rows][k], dw [n_out][k];  NN: dy [rows][n_out], x = W [n_out][k], dw = dX [rows][k]: the same rows
    if (p.lddy < p.n_out || (!sums_only && p.ldx < p.k) || (p.dw != nullptr && !sums_only && p.lddw < p.k)) {
      snprintf(msg, msg_len, "drin_wgrad_probe: product %d: leading dimensions lddy=%lld (rows of %d) ldx=%lld lddw=%lld (rows of %d)", i,
               (long long)p.lddy, p.n_out, (long long)p.ldx, (long long)p.lddw, p.k);
      return DRIN_E_SHAPE;
    }
    if (p.x_index != nullptr && a->op != DRIN_WGRAD_TN_GROUP && a->op != DRIN_WGRAD_PASS) {
      snprintf(msg, msg_len, "drin_wgrad_probe: product %d: indexed rows exist in the split-bf16 group (TN_GROUP, PASS) only", i);
      return DRIN_E_UNSUPPORTED;
    }
  }
  return DRIN_OK;
}

}  // namespace drin
