// Host build of rlc_tree.h (the body of hbtc_rlc.hip's k_rlc_tree) behind a tiny C ABI, so the CPU
// suite can check the lane-dense tile tree without a GPU (tests/test_rlc_tree_host.py).  The
// workgroup is replayed merge by merge: every level is a loop over its merges, the barrier is the
// end of the loop.  Every output is compared, as an affine point, with a plain restatement of the
// sums.  Test infrastructure only: never linked into the product library.
#include <cstring>
#include <vector>

#include "rlc_tree.h"

using namespace hbtc;

namespace {

void store_words(uint8_t* b, const uint32_t* w, int nwords) {
  for (int i = 0; i < nwords; ++i)
    for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w[i] >> (8 * j));
}

// [k] G, Jacobian (the identity for k = 0)
void point_of(G1J& r, uint64_t k) {
  G1A g;
  fq_set(g.x, G1_GEN_X);
  fq_set(g.y, G1_GEN_Y);
  g.inf = 0;
  jac_mul_u64(r, g, k);
}

void compress(uint8_t* out48, const G1J& p) {
  G1A a;
  jac_to_aff(a, p);
  uint32_t w[12];
  g1_compress(w, a);
  store_words(out48, w, 12);
}

uint32_t bitrev(uint32_t i, uint32_t k) {
  uint32_t r = 0;
  for (uint32_t b = 0; b < k; ++b) r |= ((i >> b) & 1u) << (k - 1 - b);
  return r;
}

// the plain restatement: A = sum q_i and B = sum bitrev_k(i - lo) q_i over positions [lo, lo + 2^k)
void plain_sums(G1J& A, G1J& B, const std::vector<G1J>& q, uint32_t lo, uint32_t k) {
  jac_set_inf(A);
  jac_set_inf(B);
  for (uint32_t i = 0; i < (1u << k); ++i) {
    const G1J& p = q[lo + i];
    jac_add(A, A, p);
    G1J wp;  // [w] p by double-and-add
    jac_set_inf(wp);
    const uint32_t w = bitrev(i, k);
    for (int b = (int)k - 1; b >= 0; --b) {
      jac_dbl(wp, wp);
      if ((w >> b) & 1u) jac_add(wp, wp, p);
    }
    jac_add(B, B, wp);
  }
}

}  // namespace

extern "C" {

uint32_t th_group_tiles(void) { return TREE_G; }
uint32_t th_sums_points(void) { return TS_G1J; }

// The tree of one group of n_tiles <= TREE_G tiles.  counts / masks: per tile; s_scal: per item,
// the S input is [s_scal] G (0: the identity); idx: per item, the sender; p_scal: per sender, the
// sender table entry is [p_scal] G.  reverse != 0 walks the merges of every level backwards (they
// are independent).  out48: TS_G1J compressed points per tile, in TileSums order.  Returns the
// number of outputs that differ from the plain restatement, or -1 for bad arguments.
int th_run(uint32_t n_tiles, const uint32_t* counts, const uint64_t* masks, const uint64_t* s_scal,
           const uint32_t* idx, uint32_t n_pk, const uint64_t* p_scal, int reverse, uint8_t* out48) {
  if (n_tiles == 0 || n_tiles > TREE_G) return -1;
  std::vector<TreeTile> tt(n_tiles);
  uint32_t n_items = 0;
  for (uint32_t t = 0; t < n_tiles; ++t) {
    if (counts[t] == 0 || counts[t] > 64) return -1;
    if (counts[t] < 64 && (masks[t] >> counts[t]) != 0) return -1;
    tt[t] = TreeTile{n_items, counts[t], masks[t]};
    n_items += counts[t];
  }
  // every array a heap allocation of exactly its size
  std::vector<G1J> t1s(n_items), rpk(n_pk), pnodes((size_t)n_tiles * TREE_P_SLOTS), sums((size_t)n_tiles * TS_G1J);
  for (uint32_t i = 0; i < n_items; ++i) {
    if (idx[i] >= n_pk) return -1;
    point_of(t1s[i], s_scal[i]);
  }
  for (uint32_t i = 0; i < n_pk; ++i) point_of(rpk[i], p_scal[i]);
  const std::vector<G1J> s_in = t1s;
  for (uint32_t level = 1; level <= TREE_LEVELS; ++level) {
    const uint32_t n = tree_level_merges(TREE_G, level);
    for (uint32_t k = 0; k < n; ++k)
      tree_merge(level, reverse ? n - 1 - k : k, n_tiles, tt.data(), t1s.data(), pnodes.data(), rpk.data(),
                 idx, sums.data());
  }
  int bad = 0;
  for (uint32_t t = 0; t < n_tiles; ++t) {
    std::vector<G1J> qs(64), qp(64);
    for (uint32_t i = 0; i < 64; ++i) {
      jac_set_inf(qs[i]);
      jac_set_inf(qp[i]);
      if (i < tt[t].count) qs[i] = s_in[tt[t].first + i];
      if ((tt[t].mask >> i) & 1u) qp[i] = rpk[idx[tt[t].first + i]];
    }
    const G1J* ts = sums.data() + (size_t)t * TS_G1J;
    uint8_t* o = out48 + (size_t)t * TS_G1J * 48;
    for (uint32_t j = 0; j < TS_G1J; ++j) compress(o + 48 * j, ts[j]);
    auto check = [&](const std::vector<G1J>& q, uint32_t lo, uint32_t k, uint32_t a_slot, uint32_t b_slot) {
      G1J A, B;
      plain_sums(A, B, q, lo, k);
      uint8_t e[48];
      compress(e, A);
      if (memcmp(e, o + 48 * a_slot, 48) != 0) ++bad;
      compress(e, B);
      if (memcmp(e, o + 48 * b_slot, 48) != 0) ++bad;
    };
    for (uint32_t j = 0; j < 8; ++j) {
      check(qs, 8 * j, 3, TS_S + j, TS_SW + j);
      check(qp, 8 * j, 3, TS_P + j, TS_PW + j);
    }
    for (uint32_t j = 0; j < 2; ++j) {
      check(qs, 32 * j, 4, TS_SQ + j, TS_SQW + j);
      check(qp, 32 * j, 4, TS_PQ + j, TS_PQW + j);
      check(qs, 32 * j, 5, TS_SH + j, TS_SHW + j);
      check(qp, 32 * j, 5, TS_PH + j, TS_PHW + j);
    }
    check(qs, 0, 6, TS_S + 8, TS_SW + 8);
    check(qp, 0, 6, TS_P + 8, TS_PW + 8);
  }
  return bad;
}

}  // extern "C"
