// Stand-alone host program: the argument checks of drin_wgrad_probe (drin_amd/csrc/wgrad_probe_check.h) under ASan / UBSan.
// Operand pointers are the never-dereferenced value 16; only the struct itself is read.
#include <stdio.h>
#include <string.h>

#include "wgrad_probe_check.h"

static int g_cases = 0, g_failed = 0;

static void expect(const char* what, const drin_wgrad_probe_args* a, int want, const char* needle) {
  char msg[160];
  const int got = drin::wgrad_probe_check(a, msg, sizeof msg);
  ++g_cases;
  if (got != want || (needle != nullptr && strstr(msg, needle) == nullptr)) {
    ++g_failed;
    printf("FAIL %s: status %d (want %d), message '%s'\n", what, got, want, msg);
  }
}

int main() {
  float* const one = reinterpret_cast<float*>(16);
  static drin_wgrad_probe_args ok, a;   // (static: the struct holds 16 products and their routes)
  memset(&ok, 0, sizeof ok);
  ok.struct_size = sizeof ok;
  ok.op = DRIN_WGRAD_TN_GROUP;
  ok.n_products = 2;
  ok.layers_done_after = -1;
  for (int i = 0; i < 2; ++i) {
    drin_wgrad_product& p = ok.product[i];
    p.dy = p.x = one, p.dw = one;
    p.rows = 1055, p.n_out = 132, p.k = 260, p.lddy = 132, p.ldx = 264, p.lddw = 264;
  }

  expect("NULL struct", nullptr, DRIN_E_NULL, "NULL");
  expect("valid group of two", &ok, DRIN_OK, nullptr);
  a = ok, a.struct_size = sizeof ok - 8;
  expect("short struct", &a, DRIN_E_SHAPE, "struct_size");
  a = ok, a.struct_size = 0;
  expect("zero struct_size", &a, DRIN_E_SHAPE, "struct_size");
  a = ok, a.op = 0;
  expect("op 0", &a, DRIN_E_UNSUPPORTED, "unknown op");
  a = ok, a.op = 7;
  expect("op 7", &a, DRIN_E_UNSUPPORTED, "unknown op 7");
  a = ok, a.op = -2147483647 - 1;
  expect("op INT_MIN", &a, DRIN_E_UNSUPPORTED, "unknown op");
  a = ok, a.n_products = 0;
  expect("no product", &a, DRIN_E_SHAPE, "products");
  a = ok, a.n_products = DRIN_WGRAD_PROBE_MAX + 1;   // would read past the array: refused before any product is looked at
  expect("17 products", &a, DRIN_E_SHAPE, "17 products");
  a = ok, a.n_products = -3;
  expect("negative product count", &a, DRIN_E_SHAPE, "products");
  a = ok, a.n_products = 2147483647;
  expect("INT_MAX products", &a, DRIN_E_SHAPE, "products");
  a = ok;
  for (int i = 2; i < DRIN_WGRAD_PROBE_MAX; ++i) a.product[i] = a.product[0];
  a.n_products = DRIN_WGRAD_PROBE_MAX;
  expect("16 products", &a, DRIN_OK, nullptr);
  a.product[15].k = 0;
  expect("the last of 16 is checked", &a, DRIN_E_SHAPE, "product 15");
  a = ok, a.scratch_floats = 64;
  expect("scratch size without scratch", &a, DRIN_E_NULL, "scratch");
  a = ok, a.product[1].dy = nullptr;
  expect("NULL dy", &a, DRIN_E_NULL, "product 1");
  a = ok, a.product[0].x = nullptr;
  expect("NULL x", &a, DRIN_E_NULL, "product 0");
  a = ok, a.product[1].dw = nullptr;
  expect("group without dw", &a, DRIN_E_NULL, "NULL");
  a = ok, a.product[1].rows = -1;
  expect("negative rows", &a, DRIN_E_SHAPE, "rows=-1");
  a = ok, a.product[0].rows = 0;
  expect("no rows", &a, DRIN_OK, nullptr);
  a = ok, a.product[0].n_out = 0;
  expect("n_out 0", &a, DRIN_E_SHAPE, "bad shape");
  a = ok, a.product[1].k = -4;
  expect("negative k", &a, DRIN_E_SHAPE, "bad shape");
  a = ok, a.product[0].lddy = 131;
  expect("lddy below n_out", &a, DRIN_E_SHAPE, "lddy=131");
  a = ok, a.product[0].ldx = 259;
  expect("ldx below k", &a, DRIN_E_SHAPE, "leading");
  a = ok, a.product[1].lddw = -264;
  expect("negative lddw", &a, DRIN_E_SHAPE, "leading");
  a = ok, a.product[1].x_index = reinterpret_cast<const int64_t*>(one);
  expect("indexed rows in the group", &a, DRIN_OK, nullptr);
  a.op = DRIN_WGRAD_TN_F32_GROUP;
  expect("indexed rows in the fp32 group", &a, DRIN_E_UNSUPPORTED, "indexed");

  a = ok, a.op = DRIN_WGRAD_TN;
  expect("two products for launch_gemm_tn", &a, DRIN_E_SHAPE, "one product");
  a.n_products = 1;
  expect("launch_gemm_tn", &a, DRIN_OK, nullptr);
  a.op = DRIN_WGRAD_NN;
  expect("launch_gemm_nn", &a, DRIN_OK, nullptr);
  a.wt_form = 3;
  expect("unknown wt_form", &a, DRIN_E_UNSUPPORTED, "wt_form");
  a.wt_form = DRIN_WGRAD_WT_PLANES;
  expect("planes without memory", &a, DRIN_E_NULL, "W^T");
  a.wt = one;
  expect("planes", &a, DRIN_OK, nullptr);

  a = ok, a.op = DRIN_WGRAD_COLSUM_BATCH;
  expect("column sums without db", &a, DRIN_E_NULL, "NULL");
  a.product[0].db = a.product[1].db = one;
  a.product[0].x = a.product[0].dw = nullptr, a.product[0].ldx = a.product[0].lddw = 0;
  expect("column sums need dy and db only", &a, DRIN_OK, nullptr);

  a = ok, a.op = DRIN_WGRAD_PASS, a.staged = 1, a.layers_done_after = 0;
  expect("staged pass", &a, DRIN_OK, nullptr);
  a.layers_done_after = 2;
  expect("layers_done_after past the products", &a, DRIN_E_SHAPE, "layers_done_after");
  a.layers_done_after = -1, a.product[1].dw = nullptr;
  expect("pass product with neither dw nor db", &a, DRIN_E_NULL, "NULL");
  a.product[1].db = one;
  expect("pass product with a bias gradient alone", &a, DRIN_OK, nullptr);

  char tiny[8];   // shorter than every message: truncated, not overrun
  if (drin::wgrad_probe_check(nullptr, tiny, sizeof tiny) != DRIN_E_NULL || strcmp(tiny, "drin_wg") != 0) ++g_failed;
  ++g_cases;
  a = ok, a.product[0].lddy = 1;
  if (drin::wgrad_probe_check(&a, tiny, sizeof tiny) != DRIN_E_SHAPE || strlen(tiny) != 7) ++g_failed;
  ++g_cases;
  char none[1];
  if (drin::wgrad_probe_check(nullptr, none, 0) != DRIN_E_NULL) ++g_failed;   // no room for a message at all
  ++g_cases;
  if (g_failed) return 1;
  printf("%d cases hold\n", g_cases);
  return 0;
}
