// Test-only: one operation of the 13 x 30 Fq code (field.h FqR, fq_rr.h) per item, shared by the
// host harness (hbtc_rr_hosttest.cpp) and the device harness (hbtc_rr_devtest.hip).  Operands and
// results are raw limbs: 13 words per slot (an Fq uses the first 12).
#pragma once
#include "curve.h"

namespace hbtc {
enum RrOp : uint32_t {
  RR_MUL = 0,      // out = fqr_mul(a, b)                                   (FqR, FqR -> FqR)
  RR_SQR = 1,      // out = fqr_sqr(a)                                      (FqR -> FqR)
  RR_FROM_FQ = 2,  // out = fqr_from_fq(a)                                  (Fq -> FqR)
  RR_TO_FQ = 3,    // out = fqr_to_fq(a)                                    (FqR -> Fq)
  RR_ROUND = 4,    // out = fqr_to_fq(fqr_from_fq(a))                       (Fq -> Fq)
  RR_CANON = 5,    // out = fqr_canon(a)                                    (FqR < 2p -> FqR)
  RR_EQ = 6,       // flag = fqr_eq(a, b)                                   (FqR < 2p each)
  RR_SQRT = 7,     // out = sqrt, flag = is a square: fq_sqrt_rr(a)         (Fq -> Fq)
  RR_SQRT_REF = 8,  // the same through fq_sqrt (the 12 x 32 chain)
  RR_FQ_MUL = 9,    // out = fq_canon(fq_mul(a, b)): the 12 x 32 product      (Fq, Fq -> Fq)
  RR_FQ_CANON = 10  // out = fq_canon(a)                                     (Fq -> Fq)
};

HD void rr_apply(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flag) {
  FqR ra, rb, ro;
  Fq fa, fo;
  for (int i = 0; i < 13; ++i) {
    ra.v[i] = a[i];
    rb.v[i] = b[i];
    ro.v[i] = 0;
  }
  for (int i = 0; i < 12; ++i) {
    fa.v[i] = a[i];
    fo.v[i] = 0;
  }
  uint32_t f = 0;
  bool fq_out = false;
  switch (op) {
    case RR_MUL: fqr_mul(ro, ra, rb); break;
    case RR_SQR: fqr_sqr(ro, ra); break;
    case RR_FROM_FQ: fqr_from_fq(ro, fa); break;
    case RR_TO_FQ: fqr_to_fq(fo, ra); fq_out = true; break;
    case RR_ROUND: fqr_from_fq(ro, fa); fqr_to_fq(fo, ro); fq_out = true; break;
    case RR_CANON: fqr_canon(ro, ra); break;
    case RR_EQ: f = fqr_eq(ra, rb) ? 1u : 0u; break;
    case RR_SQRT: f = fq_sqrt_rr(fo, fa) ? 1u : 0u; fq_out = true; break;
    case RR_SQRT_REF: f = fq_sqrt(fo, fa) ? 1u : 0u; fq_out = true; break;
    case RR_FQ_MUL: {
      Fq fb;
      for (int i = 0; i < 12; ++i) fb.v[i] = b[i];
      fq_mul(fo, fa, fb);
      fq_canon(fo, fo);
      fq_out = true;
      break;
    }
    case RR_FQ_CANON: fq_canon(fo, fa); fq_out = true; break;
    default: f = 0xffffffffu; break;
  }
  for (int i = 0; i < 13; ++i) out[i] = fq_out ? (i < 12 ? fo.v[i] : 0u) : ro.v[i];
  *flag = f;
}

// k_rlc_decode's decode of one compressed G1 point: g1_decompress<RR>(.., false).  out = x then y
// (12 words each, canonical Montgomery), flags = ok | inf << 1.
template <bool RR>
HD void rr_decode(const uint32_t* w, uint32_t* out, uint32_t* flags) {
  G1A p;
  const bool ok = g1_decompress<RR>(p, w, false);
  for (int i = 0; i < 12; ++i) {
    out[i] = p.x.v[i];
    out[12 + i] = p.y.v[i];
  }
  *flags = (ok ? 1u : 0u) | (p.inf ? 2u : 0u);
}
}  // namespace hbtc
