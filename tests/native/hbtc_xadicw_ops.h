// Test-only: the x-adic multiplication of the item pass on the redundant 13 x 30 form (curve.h
// xadic_mul_sac8_w) beside the 12 x 32 one (xadic_mul_sac8<Fq, true>), one item per call, shared by
// the host harness (hbtc_xadicw_hosttest.cpp, HBTC_RR_ASSERT on: both bounds of every FqW tracked and
// asserted at every operation) and the device harness (hbtc_xadicw_devtest.hip).
//   item (18 words): the base point's compressed encoding (12), d0..d3, nbits (16 or 32), lane (< 64)
//   out (72 words) : S of the redundant form, then S of 12 x 32, each x, y, z of a 12 x 32 Montgomery G1J
//   flags          : 1 decoded and not infinity, 2 the two S are the same point (jac_eq)
// lds is 3 x 24 x 64 words laid out [entry][word][lane], as k_rlc_items has it.
#pragma once
#include "curve.h"

namespace hbtc {
constexpr uint32_t XW_ITEM_WORDS = 18, XW_OUT_WORDS = 72, XW_LDS_WORDS = 3 * 24 * 64;

HD void xadicw_one(const uint32_t* it, uint32_t* o, uint32_t* flags, uint32_t* lds, bool with_ref) {
  for (uint32_t i = 0; i < XW_OUT_WORDS; ++i) o[i] = 0;
  uint32_t f = 0;
  G1A p;
  if (g1_decompress<true>(p, it, false) && !p.inf) {
    f |= 1u;
    G1J t1, a, b;
    g1_in_subgroup_t1_w(p, t1);  // t1 = [|x|] p; [x] p = -t1, as k_rlc_items takes it
    jac_neg(t1, t1);
    const uint32_t lane = it[17] & 63u;
    const int nbits = (int)it[16];
    xadic_mul_sac8_w(a, p, t1, it[12], it[13], it[14], it[15], nbits, lds, lane);
    for (int i = 0; i < 12; ++i) {
      o[i] = a.x.v[i];
      o[12 + i] = a.y.v[i];
      o[24 + i] = a.z.v[i];
    }
    if (with_ref) {
      Fq beta;
      fq_set(beta, G1_BETA);
      xadic_mul_sac8<Fq, true>(b, p, t1, beta, it[12], it[13], it[14], it[15], nbits, lds, lane);
      if (jac_eq(a, b)) f |= 2u;
      for (int i = 0; i < 12; ++i) {
        o[36 + i] = b.x.v[i];
        o[48 + i] = b.y.v[i];
        o[60 + i] = b.z.v[i];
      }
    }
  }
  *flags = f;
}

// pack -> unpack of 13 limbs spelling a product result below 1.5p: 12 packed words, then 13 limbs
HD void xadicw_roundtrip(const uint32_t* in, uint32_t* o) {
  FqW a, b;
  for (int i = 0; i < 13; ++i) a.v[i] = in[i];
#if HBTC_FW_TRACK
  fw_set_strict(a, FW_ONE_P + FW_ONE_P / 2);
#endif
  Fq k;
  fw_pack(k, a);
  fw_unpack(b, k);
  for (int i = 0; i < 12; ++i) o[i] = k.v[i];
  for (int i = 0; i < 13; ++i) o[12 + i] = b.v[i];
}
}  // namespace hbtc
