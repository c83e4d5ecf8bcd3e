// Stand-alone host program: the argument checks of drin_gemm_probe (drin_amd/csrc/gemm_probe_check.h) under ASan / UBSan.
// Operand pointers are the never-dereferenced value 16; only the struct itself is read.
#include <stdio.h>
#include <string.h>

#include "gemm_probe_check.h"

static int g_cases = 0, g_failed = 0;

static void expect(const char* what, const drin_gemm_probe_args* a, int want, const char* needle) {
  char msg[128];
  const int got = drin::gemm_probe_check(a, msg, sizeof msg);
  ++g_cases;
  if (got != want || (needle != nullptr && strstr(msg, needle) == nullptr)) {
    ++g_failed;
    printf("FAIL %s: status %d (want %d), message '%s'\n", what, got, want, msg);
  }
}

int main() {
  void* const one = reinterpret_cast<void*>(16);
  drin_gemm_probe_args ok;
  memset(&ok, 0, sizeof ok);
  ok.struct_size = sizeof ok;
  ok.op = DRIN_PROBE_GEMM_X3_PLANES;
  ok.a = ok.b_hi = ok.b_lo = one;
  ok.y = one;
  ok.rows = 300, ok.n_out = 768, ok.k = 64, ok.lda = ok.ldb = 64, ok.ldy = 772;
  ok.row_tile_end = -1;

  expect("NULL struct", nullptr, DRIN_E_NULL, "NULL");
  expect("valid planes call", &ok, DRIN_OK, nullptr);
  drin_gemm_probe_args a = ok;
  a.struct_size = sizeof ok - 8;
  expect("short struct", &a, DRIN_E_SHAPE, "struct_size");
  a = ok, a.struct_size = 0;
  expect("zero struct_size", &a, DRIN_E_SHAPE, "struct_size");
  a = ok, a.op = 0;
  expect("op 0", &a, DRIN_E_UNSUPPORTED, "unknown op");
  a = ok, a.op = 7;
  expect("op 7", &a, DRIN_E_UNSUPPORTED, "unknown op");
  a = ok, a.op = -2147483647 - 1;
  expect("op INT_MIN", &a, DRIN_E_UNSUPPORTED, "unknown op");
  a = ok, a.a = nullptr;
  expect("NULL a", &a, DRIN_E_NULL, "NULL");
  a = ok, a.y = nullptr;
  expect("NULL y", &a, DRIN_E_NULL, "NULL");
  a = ok, a.b_lo = nullptr;
  expect("planes without b_lo", &a, DRIN_E_NULL, "NULL");
  a = ok, a.a_lo = nullptr;
  expect("planes without a_lo is the contract", &a, DRIN_OK, nullptr);
  a = ok, a.scratch_floats = 64;
  expect("scratch size without scratch", &a, DRIN_E_NULL, "scratch");
  a = ok, a.rows = -1;
  expect("negative rows", &a, DRIN_E_SHAPE, "rows=-1");
  a = ok, a.rows = 0;
  expect("no rows", &a, DRIN_OK, nullptr);
  a = ok, a.n_out = 0;
  expect("n_out 0", &a, DRIN_E_SHAPE, "bad shape");
  a = ok, a.k = -32;
  expect("negative k", &a, DRIN_E_SHAPE, "bad shape");
  a = ok, a.lda = 63;
  expect("lda below k", &a, DRIN_E_SHAPE, "leading");
  a = ok, a.ldb = -64;
  expect("negative ldb", &a, DRIN_E_SHAPE, "leading");
  a = ok, a.ldy = 767;
  expect("ldy below n_out", &a, DRIN_E_SHAPE, "leading");
  a = ok, a.row_tile_begin = -1;
  expect("negative row tile", &a, DRIN_E_SHAPE, "negative");
  a = ok, a.row_tile_wgs = -8;
  expect("negative workgroups", &a, DRIN_E_SHAPE, "negative");
  a = ok, a.a_index = static_cast<const int64_t*>(one);
  expect("indexed rows on planes", &a, DRIN_E_UNSUPPORTED, "indexed");

  a = ok, a.op = DRIN_PROBE_GEMM_NT;
  expect("gemm_nt without b", &a, DRIN_E_NULL, "NULL");
  a.b = one;
  expect("gemm_nt", &a, DRIN_OK, nullptr);
  a.row_tile_wgs = 8;
  expect("gemm_nt sliced", &a, DRIN_E_UNSUPPORTED, "slice");
  a = ok, a.op = DRIN_PROBE_GEMM_NT_BF16X3, a.b_hi = a.b_lo = nullptr;
  expect("bf16x3 without any weight", &a, DRIN_E_NULL, "NULL");
  a.b_hi = one;
  expect("bf16x3 with one plane only", &a, DRIN_E_NULL, "NULL");
  a.b = one, a.a_index = static_cast<const int64_t*>(one);
  expect("bf16x3 fp32 weights, indexed", &a, DRIN_OK, nullptr);
  a = ok, a.op = DRIN_PROBE_GEMM_NT_BF16X3_P4, a.row_tile_begin = 1, a.row_tile_end = 2, a.row_tile_wgs = 3;
  expect("p4 sliced", &a, DRIN_OK, nullptr);
  a = ok, a.op = DRIN_PROBE_GEMM_F16_PLANES;
  expect("f16 without scales", &a, DRIN_E_NULL, "NULL");
  a.row_scale = a.b_scale = static_cast<const float*>(one);
  expect("f16", &a, DRIN_OK, nullptr);

  memset(&a, 0, sizeof a);
  a.struct_size = sizeof a, a.op = DRIN_PROBE_TO_F16_SCALED;
  expect("to_f16 without operands", &a, DRIN_E_NULL, "NULL");
  a.a = a.y = one, a.scratch = static_cast<float*>(one), a.scratch_floats = 1;
  expect("to_f16 scale buffer of one float", &a, DRIN_E_SHAPE, "two floats");
  a.scratch_floats = 2, a.rows = -4;
  expect("to_f16 negative count", &a, DRIN_E_SHAPE, "negative");
  a.rows = 4096;
  expect("to_f16", &a, DRIN_OK, nullptr);

  char tiny[8];   // shorter than every message: truncated, not overrun
  if (drin::gemm_probe_check(nullptr, tiny, sizeof tiny) != DRIN_E_NULL || strcmp(tiny, "drin_ge") != 0) ++g_failed;
  ++g_cases;
  char none[1];
  if (drin::gemm_probe_check(nullptr, none, 0) != DRIN_E_NULL) ++g_failed;   // no room for a message at all
  ++g_cases;
  if (g_failed) return 1;
  printf("%d cases hold\n", g_cases);
  return 0;
}
