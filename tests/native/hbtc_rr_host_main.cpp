// Stand-alone driver of the 13 x 30 Fq code's host build (hbtc_rr_hosttest.cpp), meant for a
// sanitizer build (`make sanitize-rr`).  Checks that need no big-integer library, the 12 x 32 code
// (a different algorithm: the CIOS loop of field.h mont_mul) serving as the reference:
//   the conversion round trip; product and squaring through the conversions against fq_mul;
//   fq_sqrt_rr against fq_sqrt (verdict and residue); fqr_canon / fqr_eq on p, 0 and x, x + p;
//   all-limbs-maximal operands through the product and the squaring (the host build aborts on a
//   MAD carry-out); the G1 decode with and without the 30-bit square root on random and edge
//   encodings, byte for byte.
// Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int rr_ops(uint32_t n, const uint32_t* ops, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flag);
int rr_decode_g1(uint32_t n, int rr, const uint8_t* c48, uint32_t* out, uint32_t* flags);
}

namespace {
enum { MUL, SQR, FROM_FQ, TO_FQ, ROUND, CANON, EQ, SQRT, SQRT_REF, FQ_MUL, FQ_CANON };
const uint32_t P32[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                          0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};

struct V {
  uint32_t w[13];
};
uint64_t rng_state = 0x243f6a8885a308d3ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 32);
}
V zero() {
  V v;
  memset(v.w, 0, sizeof(v.w));
  return v;
}
V rand_fq(bool plus_p) {  // a value below 2^380 < p, optionally plus p: anywhere in [0, 2p)
  V v = zero();
  for (int i = 0; i < 12; ++i) v.w[i] = rnd();
  v.w[11] &= 0x0fffffffu;
  if (plus_p) {
    uint64_t c = 0;
    for (int i = 0; i < 12; ++i) {
      c += (uint64_t)v.w[i] + P32[i];
      v.w[i] = (uint32_t)c;
      c >>= 32;
    }
  }
  return v;
}
V op(uint32_t o, const V& a, const V& b, uint32_t* flag = nullptr) {
  V r = zero();
  uint32_t f = 0;
  rr_ops(1, &o, a.w, b.w, r.w, &f);
  if (flag) *flag = f;
  return r;
}
bool same(const V& a, const V& b, int n) { return memcmp(a.w, b.w, 4 * (size_t)n) == 0; }
}  // namespace

int main() {
  int bad = 0;
  const V z = zero();
  V p = zero();
  memcpy(p.w, P32, 48);
  for (int rep = 0; rep < 400; ++rep) {
    const V a = rand_fq(rep & 1), b = rand_fq(rep & 2);
    const V ca = op(FQ_CANON, a, z);
    if (!same(op(FQ_CANON, op(ROUND, a, z), z), ca, 12)) { ++bad; printf("round trip %d\n", rep); }
    const V ra = op(FROM_FQ, a, z), rb = op(FROM_FQ, b, z);
    for (int i = 0; i < 13; ++i)
      if (ra.w[i] >> 30) { ++bad; printf("from_fq limb %d\n", rep); }
    const V want = op(FQ_MUL, a, b);
    if (!same(op(FQ_CANON, op(TO_FQ, op(MUL, ra, rb), z), z), want, 12)) { ++bad; printf("mul %d\n", rep); }
    const V wsq = op(FQ_MUL, a, a);
    if (!same(op(FQ_CANON, op(TO_FQ, op(SQR, ra, z), z), z), wsq, 12)) { ++bad; printf("sqr %d\n", rep); }
    // a chain of squarings and products without leaving the form
    V x = ra, y = a;
    for (int k = 0; k < 5; ++k) {
      x = op(MUL, op(SQR, x, z), rb);
      y = op(FQ_MUL, op(FQ_MUL, y, y), b);
    }
    if (!same(op(FQ_CANON, op(TO_FQ, x, z), z), y, 12)) { ++bad; printf("chain %d\n", rep); }
    // equality of representatives: from_fq(a) against from_fq(a + p or a - p)
    uint32_t f = 0;
    V a2 = ca;
    if (!(rep & 1)) {
      uint64_t c = 0;
      for (int i = 0; i < 12; ++i) {
        c += (uint64_t)a2.w[i] + P32[i];
        a2.w[i] = (uint32_t)c;
        c >>= 32;
      }
    }
    op(EQ, ra, op(FROM_FQ, a2, z), &f);
    if (f != 1) { ++bad; printf("eq %d\n", rep); }
    op(EQ, ra, rb, &f);
    if (f != 0) { ++bad; printf("neq %d\n", rep); }
  }
  {  // canon: p -> 0, 0 -> 0 (the limbs of p on 30 bits through the limb change of from_fq are not
     // reachable from outside; use the product: from_fq(p) is congruent to 0)
    uint32_t f = 0;
    const V rp = op(FROM_FQ, p, z), r0 = op(FROM_FQ, z, z);
    op(EQ, rp, r0, &f);
    if (f != 1) { ++bad; printf("p == 0\n"); }
    const V c = op(CANON, rp, z);
    for (int i = 0; i < 13; ++i)
      if (c.w[i]) { ++bad; printf("canon(p R') limb %d\n", i); break; }
  }
  {  // all limbs 2^30 - 1: beyond the value bound, inside the column bound (no abort), and the
     // result still congruent: (m m / R') R' == m m, checked through one more product by R'^2 / R..
     // without big integers only the no-carry-out claim and the limb sizes are checked here
    V m = zero();
    for (int i = 0; i < 13; ++i) m.w[i] = 0x3fffffffu;
    const V r1 = op(MUL, m, m), r2 = op(SQR, m, z);
    if (!same(r1, r2, 13)) { ++bad; printf("max: product != squaring\n"); }
    for (int i = 0; i < 12; ++i)
      if (r1.w[i] >> 30) { ++bad; printf("max limb %d\n", i); }
  }
  for (int rep = 0; rep < 60; ++rep) {  // square roots: squares (a^2) and arbitrary values
    const V a = rand_fq(rep & 1);
    const V s = (rep % 3) ? op(FQ_MUL, a, a) : a;
    uint32_t f1 = 0, f2 = 0;
    const V y1 = op(SQRT, s, z, &f1), y2 = op(SQRT_REF, s, z, &f2);
    if (f1 != f2 || ((rep % 3) && f1 != 1)) { ++bad; printf("sqrt verdict %d\n", rep); }
    if (!same(op(FQ_CANON, y1, z), op(FQ_CANON, y2, z), 12)) { ++bad; printf("sqrt value %d\n", rep); }
  }
  {  // the decode both ways: random x (about half are on the curve), both sign flags, x >= p, a
     // cleared compression flag, valid and invalid infinity encodings
    const int n = 48;
    std::vector<uint8_t> c(48 * n);
    for (int i = 0; i < n; ++i) {
      uint8_t* e = &c[48 * (size_t)i];
      for (int k = 0; k < 48; ++k) e[k] = (uint8_t)(rnd() >> 24);
      e[0] = (uint8_t)(0x80 | ((i & 1) ? 0x20 : 0) | (e[0] & 0x0f));  // compressed, x < 2^380
      if (i == 40) memset(e, 0xff, 48);                                // x >= p with every flag
      if (i == 41) e[0] = (uint8_t)(0x80 | 0x1f);                      // x >= p
      if (i == 42) e[0] &= 0x7f;                                       // not compressed
      if (i == 43) { memset(e, 0, 48); e[0] = 0xc0; }                  // infinity
      if (i == 44) { memset(e, 0, 48); e[0] = 0xc0; e[47] = 1; }       // infinity with a set bit
      if (i == 45) { memset(e, 0, 48); e[0] = 0x80; }                  // x = 0: (0, 2)
      if (i == 46) { memset(e, 0, 48); e[0] = 0xa0; }                  // x = 0: (0, -2)
    }
    std::vector<uint32_t> o1(24 * n), o2(24 * n), f1(n), f2(n);
    rr_decode_g1(n, 1, c.data(), o1.data(), f1.data());
    rr_decode_g1(n, 0, c.data(), o2.data(), f2.data());
    int ok = 0;
    for (int i = 0; i < n; ++i) {
      ok += f1[i] & 1;
      if (f1[i] != f2[i] || memcmp(&o1[24 * (size_t)i], &o2[24 * (size_t)i], 96) != 0) { ++bad; printf("decode %d\n", i); }
    }
    if ((f1[43] & 3) != 3 || (f1[44] & 1) || (f1[42] & 1) || (f1[40] & 1) || (f1[41] & 1) || !(f1[45] & 1) ||
        !(f1[46] & 1) || ok < 10) { ++bad; printf("decode verdicts (%d accepted)\n", ok); }
  }
  printf("13 x 30 Fq host check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
