// Host-side argument checks of the row-operation entry points (ghmfc_rows.hip, mention_rows.hip): NULL, 16-byte alignment,
// counts and widths, each naming the entry point and the argument in drin_last_error.
#pragma once
#include "internal.h"

namespace drin {

// the row-op entry points: every pointer is read or written 16 bytes per lane
struct NamedPtr {
  const char* name;
  const void* p;
  bool required;
};
inline int check_pointers(const char* who, const NamedPtr* ptrs, int n) {
  for (int i = 0; i < n; ++i) {
    if (ptrs[i].required && !ptrs[i].p) {
      set_error("%s: %s is NULL", who, ptrs[i].name);
      return DRIN_E_NULL;
    }
    if (ptrs[i].p && !aligned16(ptrs[i].p)) {
      set_error("%s: %s is not 16-byte aligned", who, ptrs[i].name);
      return DRIN_E_ALIGN;
    }
  }
  return DRIN_OK;
}
#define DRIN_CHECK_POINTERS(who, ...)                                                     \
  do {                                                                                    \
    const NamedPtr _ptrs[] = {__VA_ARGS__};                                               \
    DRIN_TRY(check_pointers(who, _ptrs, (int)(sizeof(_ptrs) / sizeof(_ptrs[0]))));        \
  } while (0)
inline int check_count(const char* who, const char* name, int64_t v, int64_t lo, int64_t hi) {
  if (v < lo || v > hi) {
    set_error("%s: %s = %lld is not in [%lld, %lld]", who, name, (long long)v, (long long)lo, (long long)hi);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}
inline int check_width4(const char* who, int E) {
  if (E <= 0 || E % 4) {
    set_error("%s: width %d must be a positive multiple of 4 (16-byte lane accesses)", who, E);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}
// how the table rows of a link entry point are stored (the *_ex twins): DRIN_FEAT_F32, or DRIN_FEAT_BF16 - 8-byte lane loads of
// four bf16 and 16-byte aligned rows, so width % 8 == 0.  Anything else: DRIN_E_UNSUPPORTED.
inline int check_row_dtype(const char* who, int row_dtype, int width) {
  if (row_dtype != DRIN_FEAT_F32 && row_dtype != DRIN_FEAT_BF16) {
    set_error("%s: row dtype %d is not DRIN_FEAT_F32 / DRIN_FEAT_BF16", who, row_dtype);
    return DRIN_E_UNSUPPORTED;
  }
  if (row_dtype == DRIN_FEAT_BF16 && (width <= 0 || width % 8)) {
    set_error("%s: width %d of bf16-stored rows must be a positive multiple of 8 (16-byte aligned rows)", who, width);
    return DRIN_E_SHAPE;
  }
  return DRIN_OK;
}

}  // namespace drin
