// Host build of the 13 x 30 Fq code (field.h FqR over fq_rr.h's plain 64-bit schedule), with
// HBTC_RR_ASSERT: every MAD of a product checks the generator's no-carry-out claim and aborts
// otherwise.  Behind a C interface for tests/test_rr_host.py (ctypes) and the stand-alone
// sanitizer driver hbtc_rr_host_main.cpp.
#define HBTC_RR_ASSERT 1
#include <cstring>

#include "hbtc_rr_ops.h"

using namespace hbtc;

extern "C" {
// n items: op, a and b (13 words per item) -> out (13 words per item), flag
int rr_ops(uint32_t n, const uint32_t* ops, const uint32_t* a, const uint32_t* b, uint32_t* out,
           uint32_t* flag) {
  for (uint32_t i = 0; i < n; ++i) rr_apply(ops[i], a + 13 * (size_t)i, b + 13 * (size_t)i, out + 13 * (size_t)i, flag + i);
  return 0;
}

// n compressed G1 points (48 bytes each) -> x, y (24 words per item), flags; rr: the square root
// on 30-bit limbs (k_rlc_decode's form) or the 12 x 32 chain
int rr_decode_g1(uint32_t n, int rr, const uint8_t* c48, uint32_t* out, uint32_t* flags) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[12];
    memcpy(w, c48 + 48 * (size_t)i, 48);
    if (rr) rr_decode<true>(w, out + 24 * (size_t)i, flags + i);
    else rr_decode<false>(w, out + 24 * (size_t)i, flags + i);
  }
  return 0;
}
}
