// Host build of enc.h (the arithmetic of hbtc_enc.hip's kernels) behind a tiny C ABI, so the
// CPU suite can check the generator's window table, the comb and GLV multiplications, the pad's
// block addressing and the Fr Horner evaluation without a GPU (tests/test_enc_host.py).  Test
// infrastructure only: never linked into the product library.
#include <cstring>
#include <vector>

#include "enc.h"

using namespace hbtc;

namespace {

void load_words(uint32_t* w, const uint8_t* b, int nwords) {
  for (int i = 0; i < nwords; ++i)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
}
void store_words(uint8_t* b, const uint32_t* w, int nwords) {
  for (int i = 0; i < nwords; ++i)
    for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w[i] >> (8 * j));
}

const EncPt* table() {
  static std::vector<EncPt> tab;
  if (tab.empty()) {
    tab.resize(ENC_TAB_ENTRIES);
    for (int i = 0; i < ENC_TAB_ENTRIES; ++i) enc_table_entry(tab[i], (uint32_t)i >> 8, (uint32_t)i & 255u);
  }
  return tab.data();
}

template <class F>
void ref_mul_compress(uint32_t* w, const Aff<F>& p, const Fr& k);
template <>
void ref_mul_compress<Fq>(uint32_t* w, const G1A& p, const Fr& k) {
  G1J j;
  jac_mul_fr(j, p, k);
  G1A a;
  jac_to_aff(a, j);
  g1_compress(w, a);
}
template <>
void ref_mul_compress<Fq2>(uint32_t* w, const G2A& p, const Fr& k) {
  G2J j;
  jac_mul_fr(j, p, k);
  G2A a;
  jac_to_aff(a, j);
  g2_compress(w, a);
}

}  // namespace

extern "C" {

// Table entry (w, v) as x || y (big-endian, canonical); v = 0 gives zeros.
void eh_table_entry(uint32_t w, uint32_t v, uint8_t* out96) {
  const EncPt e = table()[w * 256 + v];
  Fq c;
  uint32_t ww[12];
  fq_from_mont(c, e.x);
  fq_to_be_words(ww, c);
  store_words(out96, ww, 12);
  fq_from_mont(c, e.y);
  fq_to_be_words(ww, c);
  store_words(out96 + 48, ww, 12);
}

// k_enc_g1's arithmetic for one item: u = r G1 by the comb, g = r pk by the GLV split, one shared
// inversion; ref_u / ref_g: the same two products by jac_mul_fr.  -1: pk does not decode.
int eh_enc_g1(const uint8_t* pk48, const uint8_t* r_le32, uint8_t* out_u48, uint8_t* out_g48,
              uint8_t* ref_u48, uint8_t* ref_g48) {
  uint32_t w[12];
  load_words(w, pk48, 12);
  G1A A;
  if (!g1_decompress(A, w)) return -1;
  Fr k;
  load_words(k.v, r_le32, 8);
  enc_scalar_mod_r(k);
  G1J uj, gj;
  enc_comb_mul(uj, table(), k);
  Limbs<4> k0, k1;
  enc_split_by_x2(k, k0, k1);
  Fq beta;
  fq_set(beta, G1_BETA);
  enc_glv_mul(gj, A, beta, k0, k1);
  G1A ua, ga;
  enc_to_aff2(ua, ga, uj, gj);
  g1_compress(w, ua);
  store_words(out_u48, w, 12);
  g1_compress(w, ga);
  store_words(out_g48, w, 12);
  G1A gen;
  fq_set(gen.x, G1_GEN_X);
  fq_set(gen.y, G1_GEN_Y);
  gen.inf = 0;
  ref_mul_compress<Fq>(w, gen, k);
  store_words(ref_u48, w, 12);
  ref_mul_compress<Fq>(w, A, k);
  store_words(ref_g48, w, 12);
  return 0;
}

// k_enc_w's multiplication on the one-lane Fq2 type: [r] H by the GLV split with m(H) = (zeta x, -y)
// against jac_mul_fr.  -1: H does not decode.
int eh_g2_glv(const uint8_t* h96, const uint8_t* r_le32, uint8_t* out96, uint8_t* ref96) {
  uint32_t w[24];
  load_words(w, h96, 24);
  G2A H;
  if (!g2_decompress(H, w)) return -1;
  Fr k;
  load_words(k.v, r_le32, 8);
  enc_scalar_mod_r(k);
  Limbs<4> k0, k1;
  enc_split_by_x2(k, k0, k1);
  Fq zeta;
  fq_set(zeta, G2_ZETA);
  G2J acc;
  enc_glv_mul(acc, H, zeta, k0, k1);
  G2A a;
  jac_to_aff(a, acc);
  g2_compress(w, a);
  store_words(out96, w, 24);
  ref_mul_compress<Fq2>(w, H, k);
  store_words(ref96, w, 24);
  return 0;
}

// k0 (16 bytes LE) and k1 (16 bytes LE) of r mod the order
void eh_split(const uint8_t* r_le32, uint8_t* k0_le16, uint8_t* k1_le16) {
  Fr k;
  load_words(k.v, r_le32, 8);
  enc_scalar_mod_r(k);
  Limbs<4> k0, k1;
  enc_split_by_x2(k, k0, k1);
  store_words(k0_le16, k0.v, 4);
  store_words(k1_le16, k1.v, 4);
}

// hash_bytes(g, len) block by block, as k_enc_pad addresses it (each block from the seed alone)
void eh_pad_blocks(const uint8_t* g48, uint64_t len, uint8_t* out) {
  uint32_t w[12], seed[8];
  load_words(w, g48, 12);
  enc_pad_seed(seed, w);
  const uint64_t nb = enc_pad_blocks(len);
  for (uint64_t j = nb; j-- > 0;) {  // any order: blocks are independent
    uint8_t pad[16];
    enc_pad_block(pad, seed, j);
    for (uint64_t t = 0; t < 16 && 16 * j + t < len; ++t) out[16 * j + t] = pad[t];
  }
}
// the serial stream of the host hash_bytes (hbtc_hash.hip): one next_u32 per byte
void eh_pad_serial(const uint8_t* g48, uint64_t len, uint8_t* out) {
  uint8_t d[32];
  uint32_t seed[8];
  sha3_256(g48, 48, d);
  seed_of_digest(d, seed);
  ChaCha04 rng(seed);
  for (uint64_t i = 0; i < len; ++i) out[i] = (uint8_t)rng.next_u32();
}

// k_fr_to_mont + k_fr_poly_eval for one (polynomial, point) pair
void eh_fr_horner(uint32_t n_coeff, const uint8_t* coeffs_le32, const uint8_t* x_le32, uint8_t* out_le32) {
  std::vector<Fr> c(n_coeff);
  for (uint32_t k = 0; k < n_coeff; ++k) {
    Fr raw;
    load_words(raw.v, coeffs_le32 + 32 * (size_t)k, 8);
    enc_fr_load(c[k], raw);
  }
  Fr raw, x, acc, out;
  load_words(raw.v, x_le32, 8);
  enc_fr_load(x, raw);
  enc_fr_horner(acc, c.data(), n_coeff, x);
  fr_from_mont(out, acc);
  store_words(out_le32, out.v, 8);
}

}  // extern "C"
