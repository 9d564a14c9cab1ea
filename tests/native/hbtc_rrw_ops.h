// Test-only: one operation of the redundant 13 x 30 form (field.h FqW, curve.h jacw_*) per item,
// shared by the host harness (hbtc_rrw_hosttest.cpp, HBTC_RR_ASSERT on: both bounds tracked and
// asserted at every operation) and the device harness (hbtc_rrw_devtest.hip).  An item has six
// input slots and three output slots of 13 words (raw limbs; an Fq uses the first 12) and a flag.
#pragma once
#include "curve.h"

namespace hbtc {
enum RrwOp : uint32_t {
  RW_ADD = 0,        // out0 = a + b                          (entry-bound operands)
  RW_SUB = 1,        // out0 = a - b   (RR_SUB_2_14)
  RW_NEG = 2,        // out0 = -a      (a on strict limbs, < 3p)
  RW_DBL = 3,        // out0 = 2a
  RW_NORM = 4,       // out0 = fw_norm(a)                     (limbs up to 2^32 - 1, value <= 12p)
  RW_MUL = 5,        // out0 = a b / R'
  RW_SQR = 6,        // out0 = a a / R'
  RW_ZERO_SQR = 7,   // flag = fw_is_zero(fw_sqr(fw_norm(a))) (limbs up to 2^31, value <= 12p)
  RW_ZERO_ONE = 8,   // flag = fw_is_zero(fw_mul(fw_norm(a), one))
  RW_PT_DBL = 9,     // out = jacw_dbl(in0..2)
  RW_PT_ADD_AFF = 10,  // out = jacw_add_aff(in0..2, (in3, in4))
  RW_PT_ADD = 11,      // out = jacw_add(in0..2, in3..5)
  RW_PT_EQ_AFF = 12    // flag = jacw_eq_aff(in0..2, in3, in4)
};

// load raw limbs under a declared bound: limbs 0..11 <= lmax, value <= v16 p / 2^16
HD void rw_load(FqW& r, const uint32_t* w, uint64_t lmax, uint64_t v16) {
  for (int i = 0; i < 13; ++i) r.v[i] = w[i];
#if HBTC_FW_TRACK
  uint64_t lb[13];
  for (int i = 0; i < 13; ++i) lb[i] = i < 12 ? lmax : 0xffffffffull;
  fw_set_bounds(r, lb, v16);
#else
  (void)lmax;
  (void)v16;
#endif
}
HD void rw_entry(FqW& r, const uint32_t* w) { rw_load(r, w, (uint64_t)rr::RR_MASK + rr::RR_W_SLACK, 12ull << 16); }
HD void rw_store(uint32_t* o, const FqW& a) {
  for (int i = 0; i < 13; ++i) o[i] = a.v[i];
}

HD void rrw_apply(uint32_t op, const uint32_t* in, uint32_t* out, uint32_t* flag) {
  for (int i = 0; i < 39; ++i) out[i] = 0;
  uint32_t f = 0;
  FqW a, b, r;
  JacW p, q, s;
  switch (op) {
    case RW_ADD: rw_entry(a, in); rw_entry(b, in + 13); fw_add(r, a, b); rw_store(out, r); break;
    case RW_SUB: rw_entry(a, in); rw_entry(b, in + 13); fw_sub(r, a, b, rr::RR_SUB_2_14, 14); rw_store(out, r); break;
    case RW_NEG: rw_load(a, in, rr::RR_MASK, 3ull << 16); fw_neg(r, a); rw_store(out, r); break;
    case RW_DBL: rw_entry(a, in); fw_dbl(r, a); rw_store(out, r); break;
    case RW_NORM: rw_load(a, in, 0xffffffffull, 12ull << 16); fw_norm(r, a); rw_store(out, r); break;
    case RW_MUL: rw_entry(a, in); rw_entry(b, in + 13); fw_mul(r, a, b); rw_store(out, r); break;
    case RW_SQR: rw_entry(a, in); fw_sqr(r, a); rw_store(out, r); break;
    case RW_ZERO_SQR:
      rw_load(a, in, 1ull << 31, 12ull << 16);
      fw_norm(a, a);
      fw_sqr(r, a);
      f = fw_is_zero(r) ? 1u : 0u;
      break;
    case RW_ZERO_ONE:
      rw_load(a, in, 1ull << 31, 12ull << 16);
      fw_norm(a, a);
      fw_one(b);
      fw_mul(r, a, b);
      f = fw_is_zero(r) ? 1u : 0u;
      break;
    case RW_PT_DBL:
    case RW_PT_ADD_AFF:
    case RW_PT_ADD:
    case RW_PT_EQ_AFF:
      rw_entry(p.x, in);
      rw_entry(p.y, in + 13);
      rw_entry(p.z, in + 26);
      if (op == RW_PT_DBL) {
        jacw_dbl(s, p);
      } else if (op == RW_PT_ADD) {
        rw_entry(q.x, in + 39);
        rw_entry(q.y, in + 52);
        rw_entry(q.z, in + 65);
        jacw_add(s, p, q);
      } else {
        AffW qa;
        rw_load(qa.x, in + 39, rr::RR_MASK, 3ull << 15);
        if (op == RW_PT_ADD_AFF) {
          rw_load(qa.y, in + 52, rr::RR_MASK, 3ull << 15);
          jacw_add_aff(s, p, qa);
        } else {
          rw_entry(qa.y, in + 52);
          f = jacw_eq_aff(p, qa.x, qa.y) ? 1u : 0u;
          break;
        }
      }
      rw_store(out, s.x);
      rw_store(out + 13, s.y);
      rw_store(out + 26, s.z);
      break;
    default: f = 0xffffffffu; break;
  }
  *flag = f;
}

// One compressed G1 encoding (12 words): decode without the subgroup test, then the test on the
// redundant form and on 12 x 32.  o: t1 = [|x|] P of each, 36 words (x, y, z of an Fq Jacobian point)
// from the redundant form then 36 from 12 x 32.  flags: 1 decoded, 2 infinity, 4 verdict of the
// redundant form, 8 verdict of 12 x 32, 16 the two t1 are the same point (jac_eq).
HD void rrw_subgroup_one(const uint32_t* w, uint32_t* o, uint32_t* flags) {
  G1A p;
  uint32_t f = 0;
  for (int i = 0; i < 72; ++i) o[i] = 0;
  if (g1_decompress<true>(p, w, false)) {
    f |= 1u;
    if (p.inf) {
      f |= 2u;
    } else {
      G1J a, b;
      if (g1_in_subgroup_t1_w(p, a)) f |= 4u;
      if (g1_in_subgroup_t1(p, b)) f |= 8u;
      if (jac_eq(a, b)) f |= 16u;
      for (int i = 0; i < 12; ++i) {
        o[i] = a.x.v[i];
        o[12 + i] = a.y.v[i];
        o[24 + i] = a.z.v[i];
        o[36 + i] = b.x.v[i];
        o[48 + i] = b.y.v[i];
        o[60 + i] = b.z.v[i];
      }
    }
  }
  *flags = f;
}
}  // namespace hbtc
