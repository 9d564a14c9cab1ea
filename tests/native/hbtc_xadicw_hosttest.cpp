// Host build of the item pass's x-adic multiplication on the redundant 13 x 30 form (curve.h
// xadic_mul_sac8_w: the packed co-Z table chain, the column of jacw_dbl + jacw_madd_generic, the
// even-d0 correction and the exit) with HBTC_RR_ASSERT: every FqW carries its per-limb and value
// bounds and every operation asserts them, every packed value is a product result below 1.5p, every
// MAD checks the no-carry-out claim.  Behind a C interface for tests/test_xadicw_host.py (ctypes) and
// the stand-alone sanitizer driver hbtc_xadicw_host_main.cpp.
#define HBTC_RR_ASSERT 1
#include <algorithm>
#include <vector>

#include "hbtc_xadicw_ops.h"

using namespace hbtc;

extern "C" {
// n items of 18 words -> 72 words and a flag word each; the LDS-layout buffer is zeroed per item
int xadicw_mul(uint32_t n, const uint32_t* items, uint32_t* out, uint32_t* flags) {
  std::vector<uint32_t> lds(XW_LDS_WORDS);
  for (uint32_t i = 0; i < n; ++i) {
    std::fill(lds.begin(), lds.end(), 0u);
    xadicw_one(items + XW_ITEM_WORDS * (size_t)i, out + XW_OUT_WORDS * (size_t)i, flags + i, lds.data(), true);
  }
  return 0;
}
// n values of 13 limbs -> 12 packed words and 13 limbs each
int xadicw_pack(uint32_t n, const uint32_t* in, uint32_t* out) {
  for (uint32_t i = 0; i < n; ++i) xadicw_roundtrip(in + 13 * (size_t)i, out + 25 * (size_t)i);
  return 0;
}
}
