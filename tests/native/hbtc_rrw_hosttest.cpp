// Host build of the redundant 13 x 30 form (field.h FqW, curve.h jacw_*) over fq_rr.h's plain 64-bit
// schedule, with HBTC_RR_ASSERT: every value carries its per-limb and value bounds, every operation
// asserts them (no limb wrap, product operands inside the relaxed blocks' bound, subtraction
// constants above their subtrahends, zero tests and comparisons on product results below 2p), and
// every MAD checks the no-carry-out claim.  Behind a C interface for tests/test_rrw_host.py (ctypes)
// and the stand-alone sanitizer driver hbtc_rrw_host_main.cpp.
#define HBTC_RR_ASSERT 1
#include <cstring>

#include "hbtc_rrw_ops.h"

using namespace hbtc;

extern "C" {
// n items: op, six input slots (78 words) -> three output slots (39 words), flag
int rrw_ops(uint32_t n, const uint32_t* ops, const uint32_t* in, uint32_t* out, uint32_t* flag) {
  for (uint32_t i = 0; i < n; ++i) rrw_apply(ops[i], in + 78 * (size_t)i, out + 39 * (size_t)i, flag + i);
  return 0;
}

// n compressed G1 encodings (48 bytes each) through rrw_subgroup_one: 72 words and a flag word each
int rrw_subgroup(uint32_t n, const uint8_t* c48, uint32_t* out, uint32_t* flags) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[12];
    memcpy(w, c48 + 48 * (size_t)i, 48);
    rrw_subgroup_one(w, out + 72 * (size_t)i, flags + i);
  }
  return 0;
}
}
