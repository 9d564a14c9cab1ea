// Host build of skgp.h (the item bodies of hbtc_skgp.hip's kernels) behind a tiny C ABI, so the CPU
// suite can check the paired commitment, the Horner over the packed triangle and the Poly /
// FieldWrap frames without a GPU (tests/test_skgp_host.py).  Every kernel is replayed lane by lane
// over the launch's whole grid, on the same per-lane functions and with the same index arithmetic.
// Test infrastructure only: never linked into the product library.
#include <cstring>
#include <vector>

#include "skgp.h"

using namespace hbtc;

namespace {

void load_words(uint32_t* w, const uint8_t* b, int nwords) {
  for (int i = 0; i < nwords; ++i)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
}
void store_words(uint8_t* b, const uint32_t* w, size_t nwords) {
  for (size_t i = 0; i < nwords; ++i)
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

// k_fr_to_mont over n scalars
void to_mont(std::vector<Fr>& out, const uint8_t* le32, size_t n) {
  out.resize(n);
  for (size_t i = 0; i < n; ++i) {
    Fr raw;
    load_words(raw.v, le32 + 32 * i, 8);
    enc_fr_load(out[i], raw);
  }
}

}  // namespace

extern "C" {

uint32_t sh_coeff_pos(uint32_t i, uint32_t j) { return skgp_coeff_pos(i, j); }
uint64_t sh_row_bytes(uint32_t t1) { return skgp_row_bytes(t1); }

// k_skgp_commit over n coefficients (lane l: coefficients 2 l, 2 l + 1): out = n compressed points;
// ref = the same by jac_mul_fr on the generator.
void sh_commit(uint32_t n, const uint8_t* bcoef_le32, uint8_t* out48, uint8_t* ref48) {
  for (uint32_t l = 0; 2 * l < n; ++l) {
    const uint32_t i0 = 2 * l, i1 = i0 + 1;
    const bool have1 = i1 < n;
    Fr k0, k1;
    load_words(k0.v, bcoef_le32 + 32 * (size_t)i0, 8);
    load_words(k1.v, bcoef_le32 + 32 * (size_t)(have1 ? i1 : i0), 8);
    uint32_t w0[12], w1[12];
    skgp_commit_pair(w0, w1, table(), k0, k1, have1);
    store_words(out48 + 48 * (size_t)i0, w0, 12);
    if (have1) store_words(out48 + 48 * (size_t)i1, w1, 12);
  }
  G1A g;
  fq_set(g.x, G1_GEN_X);
  fq_set(g.y, G1_GEN_Y);
  g.inf = 0;
  for (uint32_t i = 0; i < n; ++i) {
    Fr k;
    load_words(k.v, bcoef_le32 + 32 * (size_t)i, 8);
    enc_scalar_mod_r(k);
    G1J j;
    jac_mul_fr(j, g, k);
    G1A a;
    jac_to_aff(a, j);
    uint32_t w[12];
    g1_compress(w, a);
    store_words(ref48 + 48 * (size_t)i, w, 12);
  }
}

// k_fr_to_mont + k_skgp_rows: the Poly frames of rows 1 .. n_rows (n_rows * sh_row_bytes(t1) bytes)
void sh_rows(uint32_t n_rows, uint32_t t1, const uint8_t* bcoef_le32, uint8_t* out) {
  std::vector<Fr> bm;
  to_mont(bm, bcoef_le32, (size_t)t1 * (t1 + 1) / 2);
  std::vector<uint32_t> msgs((size_t)n_rows * (skgp_row_bytes(t1) / 4), 0xAAAAAAAAu);
  for (uint32_t idx = 0; idx < n_rows * t1; ++idx) skgp_rows_lane(idx, bm.data(), t1, msgs.data());
  store_words(out, msgs.data(), msgs.size());
}

// k_fr_to_mont + k_skgp_vals: the FieldWrap frames of row_a(i + 1), item a * n_nodes + i
void sh_vals(uint32_t n_rows, uint32_t n_nodes, uint32_t n_coeff, const uint8_t* rows_le32, uint8_t* out) {
  std::vector<Fr> rm;
  to_mont(rm, rows_le32, (size_t)n_rows * n_coeff);
  std::vector<uint32_t> msgs((size_t)n_rows * n_nodes * SKGP_FR_WORDS, 0xAAAAAAAAu);
  for (uint32_t a = 0; a < n_rows; ++a)
    for (uint32_t i = 0; i < n_nodes; ++i) skgp_vals_lane(a, i, n_nodes, rm.data(), n_coeff, msgs.data());
  store_words(out, msgs.data(), msgs.size());
}

}  // extern "C"
