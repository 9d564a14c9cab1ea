// The producing half of a SyncKeyGen era, the host/device pieces (kernels: hbtc_skgp.hip; the
// same functions run on the CPU in tests/native/hbtc_skgp_hosttest.cpp):
//
//   commit[k] = b[k] G1             two coefficients per lane from the generator's comb table
//                                   (enc.h), made affine with one shared inversion
//   row_x coefficient k             sum_j b[coeff_pos(k, j)] x^j by Horner over the packed triangle,
//                                   read in place; written as its FieldWrap inside row x's Poly frame
//   value (a, i) = row_a(i + 1)     Horner over row a, written as one FieldWrap frame
//
// bincode 1.0 frames (hbbft_amd/wire.py): FieldWrap = u64 LE 32 + the 32 bytes big-endian (40 B);
// Poly = u64 LE count + count FieldWraps.  Every frame starts on an 8-byte boundary of its message
// buffer, so the frames are written as little-endian 32-bit words.
#pragma once
#include "enc.h"

namespace hbtc {

constexpr uint32_t SKGP_FR_FRAME = 40;                  // bytes of one FieldWrap
constexpr uint32_t SKGP_FR_WORDS = SKGP_FR_FRAME / 4;
// bytes of the Poly frame of a row with t1 coefficients
HD uint64_t skgp_row_bytes(uint32_t t1) { return 8 + (uint64_t)SKGP_FR_FRAME * t1; }

// Index of coefficient (i, j) of a symmetric bivariate polynomial in its packed upper triangle
// (BivarPoly::coeff_pos; i, j < 2^16 here: the entry points bound the triangle at 2^26 entries).
HD uint32_t skgp_coeff_pos(uint32_t i, uint32_t j) {
  return j >= i ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j;
}

// The FieldWrap of a canonical scalar as 10 little-endian words.
HD void skgp_fr_frame(uint32_t w[SKGP_FR_WORDS], const Fr& c) {
  w[0] = 32;
  w[1] = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t le = c.v[7 - j];
    w[2 + j] = (le << 24) | ((le & 0xff00u) << 8) | ((le >> 8) & 0xff00u) | (le >> 24);
  }
}

// Coefficient k of row x (canonical): sum_j b[coeff_pos(k, j)] x^j, j = 0 .. t1 - 1; bm = the
// packed triangle in Montgomery form.
HD void skgp_row_coeff(Fr& out, const Fr* __restrict__ bm, uint32_t t1, uint32_t k, uint32_t x) {
  Fr xm;
  fr_from_u64(xm, x);
  Fr acc = bm[skgp_coeff_pos(k, t1 - 1)];
#pragma unroll 1
  for (uint32_t j = t1 - 1; j-- > 0;) {
    fr_mul(acc, acc, xm);
    fr_add(acc, acc, bm[skgp_coeff_pos(k, j)]);
  }
  fr_from_mont(out, acc);
}

// One lane of k_skgp_rows: lane `idx` = (row x - 1) * t1 + k writes coefficient k's FieldWrap into
// row x's Poly frame (and, for k = 0, the frame's count).  msgs = n_rows frames of skgp_row_bytes(t1).
HD void skgp_rows_lane(uint32_t idx, const Fr* __restrict__ bm, uint32_t t1, uint32_t* __restrict__ msgs) {
  const uint32_t row = idx / t1, k = idx - row * t1;
  Fr c;
  skgp_row_coeff(c, bm, t1, k, row + 1);
  uint32_t w[SKGP_FR_WORDS];
  skgp_fr_frame(w, c);
  const size_t row_words = (size_t)(skgp_row_bytes(t1) / 4);
  uint32_t* dst = msgs + (size_t)row * row_words;
  if (k == 0) {
    dst[0] = t1;
    dst[1] = 0;
  }
  dst += 2 + (size_t)k * SKGP_FR_WORDS;
#pragma unroll
  for (uint32_t j = 0; j < SKGP_FR_WORDS; ++j) dst[j] = w[j];
}

// One lane of k_skgp_vals: item a * n_nodes + i = the FieldWrap of row_a(i + 1); rows_m = the
// rows in Montgomery form (n_coeff each; n_coeff = 0: every value is 0).
HD void skgp_vals_lane(uint32_t a, uint32_t i, uint32_t n_nodes, const Fr* __restrict__ rows_m,
                       uint32_t n_coeff, uint32_t* __restrict__ msgs) {
  Fr c;
  limbs_zero<8>(c);
  if (n_coeff) {
    Fr xm, acc;
    fr_from_u64(xm, (uint64_t)i + 1);
    enc_fr_horner(acc, rows_m + (size_t)a * n_coeff, n_coeff, xm);
    fr_from_mont(c, acc);
  }
  uint32_t w[SKGP_FR_WORDS];
  skgp_fr_frame(w, c);
  uint32_t* dst = msgs + ((size_t)a * n_nodes + i) * SKGP_FR_WORDS;
#pragma unroll
  for (uint32_t j = 0; j < SKGP_FR_WORDS; ++j) dst[j] = w[j];
}

// One lane of k_skgp_commit: the commitments of coefficients 2 l and 2 l + 1 (the second only
// when it exists) as compressed words; k0 / k1 = any 256-bit values.
HD void skgp_commit_pair(uint32_t w0[12], uint32_t w1[12], const EncPt* __restrict__ tab, const Fr& k0,
                         const Fr& k1, bool have1) {
  Fr a = k0, b = k1;
  enc_scalar_mod_r(a);
  enc_scalar_mod_r(b);
  G1J p, q;
  enc_comb_mul(p, tab, a);
  jac_set_inf(q);
  if (have1) enc_comb_mul(q, tab, b);
  G1A pa, qa;
  enc_to_aff2(pa, qa, p, q);
  g1_compress(w0, pa);
  g1_compress(w1, qa);
}

}  // namespace hbtc
