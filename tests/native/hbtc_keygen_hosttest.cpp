// Host build of keygen.h (the arithmetic of hbtc_keygen.hip's kernels) behind a tiny C ABI, so the
// CPU suite can check the column sum, the interpolation at 0, the Horner evaluation and the
// shared-inversion affine conversion without a GPU (tests/test_keygen_host.py).  The kernels'
// workgroups are replayed lane by lane: every step that a barrier separates on the device is a
// loop over the lanes here, on the same per-lane functions.  Test infrastructure only: never
// linked into the product library.
#include <cstring>
#include <vector>

#include "keygen.h"

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

// the scans of k_kg_affine / k_kg_fr_part over KG_BS lanes; inv_total = 1 / the product of all
template <class T, class Inv>
void sim_scan(std::vector<KgScan<T>>& sc, std::vector<T>& C, std::vector<T>& S, T& inv_total, Inv inv) {
  for (uint32_t tid = 0; tid < KG_BS; ++tid) {
    sc[tid].sp = sc[tid].cp;
    C[tid] = S[tid] = sc[tid].cp;
  }
  std::vector<KgScanIn<T>> in(KG_BS);
  for (uint32_t off = 1; off < KG_BS; off <<= 1) {
    for (uint32_t tid = 0; tid < KG_BS; ++tid) kg_scan_read(in[tid], tid, off, C.data(), S.data());
    for (uint32_t tid = 0; tid < KG_BS; ++tid) kg_scan_write(sc[tid], in[tid], tid, off, C.data(), S.data());
  }
  inv(inv_total, C[KG_BS - 1]);
}

// k_kg_affine for up to KG_BS points (n_seg = 1)
void sim_affine(uint32_t n, const G1J* in, uint8_t* out48) {
  std::vector<KgScan<Fq>> sc(KG_BS);
  std::vector<Fq> C(KG_BS), S(KG_BS);
  std::vector<G1J> p(KG_BS);
  for (uint32_t tid = 0; tid < KG_BS; ++tid) {
    jac_set_inf(p[tid]);
    if (tid < n) p[tid] = in[tid];
    kg_affine_factor(sc[tid].cp, p[tid]);
  }
  Fq inv_total;
  sim_scan(sc, C, S, inv_total, [](Fq& r, const Fq& a) { finv_fast(r, a); });
  for (uint32_t tid = 0; tid < n; ++tid) {
    Fq zinv, e_excl, incl;
    kg_scan_inverse(zinv, e_excl, incl, tid, C.data(), S.data(), inv_total);
    G1A a;
    kg_affine_finish(a, p[tid], zinv);
    uint32_t w[12];
    g1_compress(w, a);
    store_words(out48 + 48 * (size_t)tid, w, 12);
  }
}

bool decode_all(std::vector<G1A>& out, const uint8_t* c48, size_t n) {
  out.resize(n);
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[12];
    load_words(w, c48 + 48 * i, 12);
    if (!g1_decompress(out[i], w)) return false;
  }
  return true;
}

}  // namespace

extern "C" {

uint32_t kh_block_size(void) { return KG_BS; }
uint32_t kh_segment_len(void) { return KG_SEG; }

// k_kg_fr_prep + k_kg_fr_part for one Part of m values: out = L(0), canonical.  Returns 1 when an
// x repeats (the output is meaningless then), else 0.
int kh_interp(uint32_t m, const uint32_t* x, const uint8_t* vals_le32, uint8_t* out_le32) {
  std::vector<Fr> xm(m), ym(m), q(m), pre(m), wy(m);
  for (uint32_t i = 0; i < m; ++i) {
    Fr raw;
    load_words(raw.v, vals_le32 + 32 * (size_t)i, 8);
    kg_fr_prep(xm[i], ym[i], x[i], raw);
  }
  std::vector<KgScan<Fr>> sc(KG_BS);
  std::vector<Fr> C(KG_BS), S(KG_BS);
  bool dup = false;
  for (uint32_t tid = 0; tid < KG_BS; ++tid)
    dup |= kg_lane_products(sc[tid].cp, tid, m, x, xm.data(), ym.data(), q.data(), pre.data(), wy.data());
  Fr inv_total;
  sim_scan(sc, C, S, inv_total, [](Fr& r, const Fr& a) { fr_inv(r, a); });
  std::vector<Fr> sum(KG_BS);
  for (uint32_t tid = 0; tid < KG_BS; ++tid) {
    Fr own_inv, e_excl, incl;
    kg_scan_inverse(own_inv, e_excl, incl, tid, C.data(), S.data(), inv_total);
    kg_lane_dot(sum[tid], tid, m, e_excl, incl, q.data(), pre.data(), wy.data());
  }
  for (uint32_t off = KG_BS / 2; off > 0; off >>= 1)
    for (uint32_t tid = 0; tid < KG_BS; ++tid) kg_fr_tree_step(sum.data(), tid, off);
  Fr c;
  fr_from_mont(c, sum[0]);
  store_words(out_le32, c.v, 8);
  return dup ? 1 : 0;
}

// k_kg_horner + k_kg_affine: sum_j xs[k]^j commit[j] for n_x <= KG_BS points x >= 1, the segments
// joined as the kernel joins them.  -1: a coefficient does not decode.
int kh_eval(uint32_t t1, const uint8_t* commit_c48, uint32_t n_x, const uint32_t* xs, uint8_t* out48) {
  std::vector<G1A> C;
  if (n_x > KG_BS || !decode_all(C, commit_c48, t1)) return -1;
  std::vector<G1J> pts(n_x);
  const uint32_t n_seg = kg_segments(t1);
  for (uint32_t k = 0; k < n_x; ++k) {
    G1J p;
    kg_eval_segment(p, C.data(), t1, 0, xs[k]);
    for (uint32_t s = 1; s < n_seg; ++s) {
      G1J q;
      kg_eval_segment(q, C.data(), t1, s, xs[k]);
      jac_add(p, p, q);
    }
    pts[k] = p;
  }
  sim_affine(n_x, pts.data(), out48);
  return 0;
}

// k_kg_colsum + k_kg_affine: out[j] = sum_p row0[p][j].  -1: a point does not decode.
int kh_colsum(uint32_t n_parts, uint32_t t1, const uint8_t* row0_c48, uint8_t* out48) {
  std::vector<G1A> dec;
  if (!decode_all(dec, row0_c48, (size_t)n_parts * t1)) return -1;
  std::vector<G1J> col(t1);
  for (uint32_t j = 0; j < t1; ++j) {
    std::vector<G1J> sh(KG_COL);
    for (uint32_t tid = 0; tid < KG_COL; ++tid) kg_col_lane(sh[tid], dec.data(), n_parts, t1, j, tid);
    for (uint32_t off = KG_COL / 2; off > 0; off >>= 1)
      for (uint32_t tid = 0; tid < KG_COL; ++tid) kg_tree_step(sh.data(), tid, off);
    col[j] = sh[0];
  }
  for (uint32_t j0 = 0; j0 < t1; j0 += KG_BS)
    sim_affine(t1 - j0 < KG_BS ? t1 - j0 : KG_BS, col.data() + j0, out48 + 48 * (size_t)j0);
  return 0;
}

}  // extern "C"
