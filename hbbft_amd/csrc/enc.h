// PublicKey::encrypt_with_rng and Fr polynomial evaluation, the host/device pieces (kernels:
// hbtc_enc.hip; the same functions run on the CPU in tests/native/hbtc_enc_hosttest.cpp).
//
//   u = r G1                      fixed-base comb over a window table of the generator
//   g = r pk                      GLV: r = k0 + k1 x^2, [r] pk = [k0] pk + [k1] (beta x, -y)
//   v = msg XOR hash_bytes(g)     counter-mode ChaCha blocks of 16 pad bytes (hash_hd.h)
//   out = sum_k c_k x^k           Horner over Montgomery Fr
#pragma once
#include "curve.h"
#include "hash_hd.h"

namespace hbtc {

// Window table of the generator: tab[w * 256 + v] = v 2^(8w) G1 (affine, v >= 1; entry 0 of a
// window is unused) for the 32 byte windows of a 256-bit scalar: 8192 entries of 96 B = 768 KB.
constexpr int ENC_WINDOWS = 32;
constexpr int ENC_TAB_ENTRIES = ENC_WINDOWS * 256;
struct EncPt {
  Fq x, y;
};

// k mod r for any 256-bit k (2^256 < 3r: at most two subtractions)
HD void enc_scalar_mod_r(Fr& k) {
#pragma unroll
  for (int rep = 0; rep < 2; ++rep) {
    Fr t;
    const uint32_t borrow = limbs_sub_const<8>(t, k, FR_R);
    limbs_select<8>(k, borrow == 0, k, t);
  }
}

// one table entry: [v] G1 by an 8-bit double-and-add, then 8w doublings
HD void enc_table_entry(EncPt& out, uint32_t w, uint32_t v) {
  fq_zero(out.x);
  fq_zero(out.y);
  if (v == 0) return;
  G1A g;
  fq_set(g.x, G1_GEN_X);
  fq_set(g.y, G1_GEN_Y);
  g.inf = 0;
  G1J acc;
  jac_set_inf(acc);
#pragma unroll 1
  for (int b = 7; b >= 0; --b) {
    jac_dbl(acc, acc);
    if ((v >> b) & 1u) jac_add_aff(acc, acc, g);
  }
#pragma unroll 1
  for (uint32_t d = 0; d < 8 * w; ++d) jac_dbl(acc, acc);
  // never infinity: 0 < v 2^(8w) < 2^256 < 3r, and neither r (odd) nor 2r (one factor 2, so
  // w = 0 and v = 2r >= 256) has the form v 2^(8w) with v < 256
  Fq zi, zi2, zi3;
  finv_fast(zi, acc.z);
  fq_sqr(zi2, zi);
  fq_mul(zi3, zi2, zi);
  fq_mul(out.x, acc.x, zi2);
  fq_mul(out.y, acc.y, zi3);
}

// [k] G1 for a canonical k (< r) from the window table: at most 32 mixed additions, no doublings.
// With k < r every prefix sum (k mod 2^(8w)) G1 has a scalar strictly between 0 and r once it is
// nonzero, and the next addend v 2^(8w) is larger than that prefix while their sum is still
// <= k < r: the mixed addition never meets its doubling or its inverse case; the only special
// case is the point at infinity (the prefix 0, all of k = 0), which jac_add_aff handles.
HD void enc_comb_mul(G1J& r, const EncPt* tab, const Fr& k) {
  G1J acc;
  jac_set_inf(acc);
  Fr kk = k;
#pragma unroll 1
  for (int wi = 0; wi < 8; ++wi) {
    uint32_t word = kk.v[0];
#pragma unroll
    for (int j = 0; j < 7; ++j) kk.v[j] = kk.v[j + 1];  // static indexing only
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
      const uint32_t v = word & 0xffu;
      word >>= 8;
      if (v) {
        const EncPt e = tab[(wi * 4 + b) * 256 + v];
        G1A t;
        t.x = e.x;
        t.y = e.y;
        t.inf = 0;
        jac_add_aff(acc, acc, t);
      }
    }
  }
  r = acc;
}

// k (canonical, < r, 8 little-endian limbs) = k1 x^2 + k0 with k0 < x^2 and k1 < 2^128 (k < r <
// x^4): binary long division by x^2 = 0xac45a4010001a4020000000100000000.
HD void enc_split_by_x2(const Fr& k, Limbs<4>& k0, Limbs<4>& k1) {
  const uint32_t X2_0 = 0x00000000u, X2_1 = 0x00000001u, X2_2 = 0x0001a402u, X2_3 = 0xac45a401u;
  uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
  Fr kk = k, q;
  limbs_zero<8>(q);
#pragma unroll 1
  for (int bit = 255; bit >= 0; --bit) {
    // rem = 2 rem + the top bit of kk; kk <<= 1; q <<= 1
    r4 = (r4 << 1) | (r3 >> 31);
    r3 = (r3 << 1) | (r2 >> 31);
    r2 = (r2 << 1) | (r1 >> 31);
    r1 = (r1 << 1) | (r0 >> 31);
    r0 = (r0 << 1) | (kk.v[7] >> 31);
#pragma unroll
    for (int j = 7; j > 0; --j) {
      kk.v[j] = (kk.v[j] << 1) | (kk.v[j - 1] >> 31);
      q.v[j] = (q.v[j] << 1) | (q.v[j - 1] >> 31);
    }
    kk.v[0] <<= 1;
    q.v[0] <<= 1;
    uint32_t b, d0, d1, d2, d3, d4;
    d0 = subb32(r0, X2_0, 0, &b);
    d1 = subb32(r1, X2_1, b, &b);
    d2 = subb32(r2, X2_2, b, &b);
    d3 = subb32(r3, X2_3, b, &b);
    d4 = subb32(r4, 0u, b, &b);
    if (b == 0) {  // rem >= x^2
      r0 = d0;
      r1 = d1;
      r2 = d2;
      r3 = d3;
      r4 = d4;
      q.v[0] |= 1u;
    }
  }
  k0.v[0] = r0;
  k0.v[1] = r1;
  k0.v[2] = r2;
  k0.v[3] = r3;
#pragma unroll
  for (int j = 0; j < 4; ++j) k1.v[j] = q.v[j];
}

// [k0] A + [k1] m(A) with m(A) = (c x, -y) = [x^2] A for A in the prime-order subgroup (G1: c =
// beta, G2: c = zeta; curve.h: (c X, Y) has the eigenvalue -x^2 on both): a joint 128-bit
// double-and-add with one (complete) mixed addition per bit from {A, m(A), A + m(A)}, selected
// without branches, so every lane of a wave runs the same instructions.
template <class F>
HD void enc_glv_mul(Jac<F>& r, const Aff<F>& A, const Fq& c, const Limbs<4>& k0, const Limbs<4>& k1) {
  Aff<F> m, am;
  {
    fmul_by_fq(m.x, A.x, c);
    fneg(m.y, A.y);
    m.inf = A.inf;
    Jac<F> s;
    jac_from_aff(s, A);
    jac_add_aff(s, s, m);  // [1 + x^2] A: O only for A = O
    am.inf = jac_is_inf(s) ? 1u : 0u;
    fzero(am.x);
    fzero(am.y);
    if (!am.inf) {
      F zi, zi2, zi3;
      finv_fast(zi, s.z);
      fsqr(zi2, zi);
      fmul(zi3, zi2, zi);
      fmul(am.x, s.x, zi2);
      fmul(am.y, s.y, zi3);
    }
  }
  Jac<F> acc;
  jac_set_inf(acc);
  Limbs<4> a = k0, b = k1;
#pragma unroll 1
  for (int wi = 0; wi < 4; ++wi) {
    const uint32_t wa = a.v[3], wb = b.v[3];
#pragma unroll
    for (int j = 3; j > 0; --j) {  // static indexing only
      a.v[j] = a.v[j - 1];
      b.v[j] = b.v[j - 1];
    }
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      jac_dbl(acc, acc);
      const bool ba = ((wa >> bit) & 1u) != 0, bb = ((wb >> bit) & 1u) != 0;
      Aff<F> t;
      F sx, sy;
      fsel(sx, ba, am.x, m.x);
      fsel(sy, ba, am.y, m.y);
      fsel(t.x, bb, sx, A.x);
      fsel(t.y, bb, sy, A.y);
      t.inf = bb ? (ba ? am.inf : m.inf) : A.inf;
      Jac<F> n;
      jac_add_aff(n, acc, t);
      const bool take = ba || bb;
      fsel(acc.x, take, n.x, acc.x);
      fsel(acc.y, take, n.y, acc.y);
      fsel(acc.z, take, n.z, acc.z);
    }
  }
  r = acc;
}

// Two Jacobian points -> affine with ONE inversion (either may be infinity).
HD void enc_to_aff2(G1A& a, G1A& b, const G1J& p, const G1J& q) {
  a.inf = jac_is_inf(p) ? 1u : 0u;
  b.inf = jac_is_inf(q) ? 1u : 0u;
  Fq one, zp, zq, prod, inv, ip, iq, i2;
  fq_one(one);
  fq_sel(zp, a.inf != 0, one, p.z);
  fq_sel(zq, b.inf != 0, one, q.z);
  fq_mul(prod, zp, zq);
  finv_fast(inv, prod);
  fq_mul(ip, inv, zq);  // 1 / zp
  fq_mul(iq, inv, zp);  // 1 / zq
  fq_zero(a.x);
  fq_zero(a.y);
  fq_zero(b.x);
  fq_zero(b.y);
  if (!a.inf) {
    fq_sqr(i2, ip);
    fq_mul(a.x, p.x, i2);
    fq_mul(i2, i2, ip);
    fq_mul(a.y, p.y, i2);
  }
  if (!b.inf) {
    fq_sqr(i2, iq);
    fq_mul(b.x, q.x, i2);
    fq_mul(i2, i2, iq);
    fq_mul(b.y, q.y, i2);
  }
}

// ---- the pad: hash_bytes(g, len) in counter mode
// The ChaCha seed of hash_bytes(g, .): sha3_256 of the 48 compressed bytes (12 words as the
// codec stores them, little-endian in memory).
HASH_HD void enc_pad_seed(uint32_t seed[8], const uint32_t g_words[12]) {
  // the one-block sponge written out on whole lanes (no byte buffers, so no scratch on the GPU):
  // 48 message bytes = lanes 0..5, the 0x06 pad byte at position 48, 0x80 at position 135
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) a[i] = (uint64_t)g_words[2 * i] | ((uint64_t)g_words[2 * i + 1] << 32);
  a[6] = 0x06ull;
  a[16] = 0x80ull << 56;
  keccak_f(a);
  // seed_of_digest: seed word i = the digest bytes 4 i .. 4 i + 3, big-endian
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t le = (uint32_t)(a[i >> 1] >> (32 * (i & 1)));
    seed[i] = (le << 24) | ((le & 0xff00u) << 8) | ((le >> 8) & 0xff00u) | (le >> 24);
  }
}
// Each pad byte is the low byte of one next_u32, so ChaCha block j (the 128-bit counter of rand
// 0.4's ChaChaRng = j) yields pad bytes [16 j, 16 j + 16).
HASH_HD uint64_t enc_pad_blocks(uint64_t len) { return (len + 15) / 16; }
HASH_HD void enc_pad_block(uint8_t out[16], const uint32_t seed[8], uint64_t block) {
  ChaCha04 rng(seed);
  rng.state[12] = (uint32_t)block;
  rng.state[13] = (uint32_t)(block >> 32);
  rng.refill();
  for (int i = 0; i < 16; ++i) out[i] = (uint8_t)rng.buf[i];
}

// One lane of the pad (k_enc_pad): block b of the batch belongs to the item i with blk_off[i] <=
// b < blk_off[i + 1] (blk_off[n] = the batch's block count); its up to 16 bytes of
// [offsets[i], offsets[i + 1]) become msg XOR pad, or zero when the item's gate is not 0 (ACCEPT).
HASH_HD void enc_pad_lane(uint32_t b, uint32_t n, const uint32_t* __restrict__ blk_off,
                          const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ seeds,
                          const int32_t* __restrict__ gate, const uint8_t* __restrict__ msgs,
                          uint8_t* __restrict__ out_v) {
  uint32_t lo = 0, hi = n;  // blk_off[lo] <= b < blk_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (blk_off[mid] <= b)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t i = lo, j = b - blk_off[i];
  const uint32_t start = offsets[i] + 16u * j, end = offsets[i + 1];
  const uint32_t cnt = end - start < 16u ? end - start : 16u;
  uint8_t pad[16];
  const bool ok = gate[i] == 0;
  if (ok) {
    uint32_t seed[8];
    for (int t = 0; t < 8; ++t) seed[t] = seeds[8 * (size_t)i + t];
    enc_pad_block(pad, seed, j);
  }
#pragma unroll
  for (uint32_t t = 0; t < 16; ++t)
    if (t < cnt) out_v[start + t] = ok ? (uint8_t)(msgs[start + t] ^ pad[t]) : (uint8_t)0;
}

// One item of k_dec_seed: the pad seed of a combined g (its 48 compressed bytes as 12 words; the
// infinity encoding 0xC0 00.. is hashed like any other, as the reference's hash_bytes does), or
// zeros for an item whose gate did not pass.  Returns the pad's gate: 0 (ACCEPT) or 1.
HASH_HD int32_t dec_seed_item(uint32_t seed[8], const uint32_t g_words[12], bool pass) {
  if (!pass) {
    for (int t = 0; t < 8; ++t) seed[t] = 0;
    return 1;
  }
  enc_pad_seed(seed, g_words);
  return 0;
}

// ---- Fr polynomials
// sum_k c[k] x^k by Horner; c (n >= 1 coefficients, constant term first) and x in Montgomery form
HD void enc_fr_horner(Fr& out, const Fr* c, uint32_t n, const Fr& x) {
  Fr acc = c[n - 1];
#pragma unroll 1
  for (uint32_t k = n - 1; k-- > 0;) {
    fr_mul(acc, acc, x);
    fr_add(acc, acc, c[k]);
  }
  out = acc;
}
// any 256-bit little-endian value -> Montgomery Fr of its residue
HD void enc_fr_load(Fr& out, const Fr& raw) {
  Fr k = raw;
  enc_scalar_mod_r(k);
  fr_to_mont(out, k);
}

}  // namespace hbtc
