// Host build of msm_walk.h (the lane-uniform bucket walk of hbtc_msm.hip's k_msm_buckets) behind a
// tiny C ABI, so the CPU suite can check it without a GPU (tests/test_msm_walk_host.py).  One wave
// is replayed in lockstep: up to 64 lane states, one (window, segment) slice each, advance together
// through the loop of the kernel, and the wave votes are loops over the lanes.  Two groups:
//   toy  integers modulo 2^61 - 1 (a "point" is a residue, addition is addition), so the caller
//        checks sum b P exactly with plain arithmetic;
//   g1   curve.h's G1 on the host, every lane compared after normalisation with the nested loops of
//        rounds 1-9 restated here, and every window's sum returned compressed.
// The digits are sorted here the way k_msm_sort leaves them (largest bucket first, rank offsets
// ro[0 .. B]); inside a bucket the terms stay in index order.  Test infrastructure only: never
// linked into the product library.
#include <cstring>
#include <vector>

#include "curve.h"
#include "msm_walk.h"

namespace hbtc {

// ------------------------------------------------------------------ the toy group
constexpr uint64_t TOY_P = (1ull << 61) - 1;
struct ToyJ {
  uint64_t v;
};
struct ToyA {
  uint64_t v;
  uint32_t inf;
};
static inline void jac_set_inf(ToyJ& r) { r.v = 0; }
static inline void jac_add(ToyJ& r, const ToyJ& a, const ToyJ& b) { r.v = (a.v + b.v) % TOY_P; }
static inline void jac_dbl(ToyJ& r, const ToyJ& a) { r.v = (a.v + a.v) % TOY_P; }
static inline void jac_add_aff(ToyJ& r, const ToyJ& a, const ToyA& b) { r.v = b.inf ? a.v : (a.v + b.v) % TOY_P; }
static inline void aff_neg(ToyA& r, const ToyA& a) {
  r.v = (TOY_P - a.v) % TOY_P;
  r.inf = a.inf;
}

}  // namespace hbtc

using namespace hbtc;

namespace {

// the snapshot slots as one heap allocation of exactly lanes * slots points
template <class J>
struct HostSlots {
  J* base;  // the lane's slots
  uint32_t slots;
  int* overrun;
  void put(uint32_t k, const J& p) {
    if (k >= slots) {
      ++*overrun;
      return;
    }
    base[k] = p;
  }
  void get(J& p, uint32_t k) const {
    if (k >= slots) {
      ++*overrun;
      return;
    }
    p = base[k];
  }
};

struct Sorted {
  std::vector<uint32_t> ro, list;  // [n_win][B + 1], [n_win][n]
};

// k_msm_sort on the host: rank r = B - |d|, list entry = index | sign << 31
bool sort_digits(Sorted& so, uint32_t n_win, uint32_t n, uint32_t B, const int16_t* digits) {
  so.ro.assign((size_t)n_win * (B + 1), 0);
  so.list.assign((size_t)n_win * n, 0);
  for (uint32_t w = 0; w < n_win; ++w) {
    const int16_t* d = digits + (size_t)w * n;
    uint32_t* ro = so.ro.data() + (size_t)w * (B + 1);
    std::vector<uint32_t> cnt(B, 0);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t a = (uint32_t)(d[i] < 0 ? -d[i] : d[i]);
      if (a > B) return false;
      if (a) ++cnt[B - a];
    }
    uint32_t acc = 0;
    for (uint32_t r = 0; r < B; ++r) {
      ro[r] = acc;
      acc += cnt[r];
      cnt[r] = ro[r];
    }
    ro[B] = acc;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t a = (uint32_t)(d[i] < 0 ? -d[i] : d[i]);
      if (a) so.list[(size_t)w * n + cnt[B - a]++] = i | (d[i] < 0 ? 0x80000000u : 0u);
    }
  }
  return true;
}

template <class A>
void term_of(A& q, const A* pts, uint32_t v) {
  q = pts[v & 0x7fffffffu];
  if (v >> 31) aff_neg(q, q);
}

// One wave of n_win * S lanes through the loop of k_msm_buckets.  stats: [0] loop iterations with a
// step, [1] flushes inside the loop, [2] flush rounds in all (full additions the wave issues),
// [3] slot overruns (must stay 0).
template <class J, class A>
void wave_walk(std::vector<J>& part, uint32_t n_win, uint32_t n, uint32_t B, uint32_t S, uint32_t slots,
               const Sorted& so, const A* pts, uint32_t* stats) {
  const uint32_t lanes = n_win * S;
  std::vector<J> snap((size_t)lanes * slots), run(lanes), tot(lanes);
  std::vector<MsmWalk> w(lanes);
  std::vector<HostSlots<J>> st;
  int overrun = 0;
  for (uint32_t l = 0; l < lanes; ++l) {
    st.push_back(HostSlots<J>{snap.data() + (size_t)l * slots, slots, &overrun});
    jac_set_inf(run[l]);
    jac_set_inf(tot[l]);
    walk_begin(w[l], so.ro.data() + (size_t)(l / S) * (B + 1), B, S, l % S);
  }
  auto flush = [&]() {
    for (uint32_t k = 0; k < slots; ++k) {
      bool any = false;
      for (uint32_t l = 0; l < lanes; ++l) any |= walk_pending(w[l]) > k;
      if (!any) break;
      ++stats[2];
      for (uint32_t l = 0; l < lanes; ++l) walk_flush(w[l], k, tot[l], st[l]);
    }
    for (uint32_t l = 0; l < lanes; ++l) walk_flush_done(w[l]);
  };
  for (;;) {
    bool need = false, active = false;
    for (uint32_t l = 0; l < lanes; ++l)
      need |= walk_boundary(w[l], so.ro.data() + (size_t)(l / S) * (B + 1), run[l], st[l], slots);
    if (need) {
      ++stats[1];
      flush();
      continue;
    }
    for (uint32_t l = 0; l < lanes; ++l) active |= walk_active(w[l]);
    if (!active) break;
    ++stats[0];
    for (uint32_t l = 0; l < lanes; ++l)
      if (walk_active(w[l])) {
        A q;
        term_of(q, pts, so.list[(size_t)(l / S) * n + walk_step(w[l])]);
        jac_add_aff(run[l], run[l], q);
      }
  }
  flush();
  for (uint32_t l = 0; l < lanes; ++l) walk_finish(tot[l], run[l], w[l], B);
  stats[3] = (uint32_t)overrun;
  part = tot;
}

// the nested loops of rounds 1-9 (k_msm_buckets with HBTC_MSM_WALK=0), one lane
template <class J, class A>
void nested_walk(J& tot, uint32_t n, uint32_t B, uint32_t S, uint32_t s, const uint32_t* ro, const uint32_t* L,
                 const A* pts) {
  J run;
  jac_set_inf(run);
  jac_set_inf(tot);
  const uint32_t total = ro[B];
  const uint32_t p0 = (uint32_t)((uint64_t)total * s / S);
  const uint32_t p1 = (uint32_t)((uint64_t)total * (s + 1) / S);
  if (p0 >= p1) return;
  const uint32_t r_last = msm_rank(ro, B, p1 - 1);
  uint32_t e = p0;
  for (uint32_t r = msm_rank(ro, B, p0); r <= r_last; ++r) {
    const uint32_t end = ro[r + 1] < p1 ? ro[r + 1] : p1;
    for (; e < end; ++e) {
      A q;
      term_of(q, pts, L[e]);
      jac_add_aff(run, run, q);
    }
    jac_add(tot, tot, run);
  }
  for (uint32_t k = B - r_last - 1; k; --k) jac_add(tot, tot, run);
}

bool shape_ok(uint32_t n_win, uint32_t B, uint32_t S, uint32_t slots) {
  return n_win && S && slots && B >= S && n_win * S <= 64 && B <= 1024;
}

void store_words(uint8_t* b, const uint32_t* w, int nwords) {
  for (int i = 0; i < nwords; ++i)
    for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w[i] >> (8 * j));
}
void compress(uint8_t* out48, const G1J& p) {
  G1A a;
  jac_to_aff(a, p);
  uint32_t w[12];
  g1_compress(w, a);
  store_words(out48, w, 12);
}

}  // namespace

extern "C" {

uint64_t mh_toy_modulus(void) { return TOY_P; }

// Toy group.  digits [n_win][n] in [-B, B]; vals [n] residues (the "points"; inf[i] != 0: the
// identity); out [n_win * S]: every lane's share of sum_b b B_b.  Returns 0, or -1 for bad
// arguments, or -2 if a lane overran its slots.
int mh_toy(uint32_t n_win, uint32_t n, uint32_t B, uint32_t S, uint32_t slots, const int16_t* digits,
           const uint64_t* vals, const uint8_t* inf, uint64_t* out, uint32_t* stats) {
  if (!shape_ok(n_win, B, S, slots)) return -1;
  Sorted so;
  if (!sort_digits(so, n_win, n, B, digits)) return -1;
  std::vector<ToyA> pts(n);
  for (uint32_t i = 0; i < n; ++i) pts[i] = ToyA{vals[i] % TOY_P, inf[i]};
  std::vector<ToyJ> part;
  memset(stats, 0, 4 * sizeof(uint32_t));
  wave_walk(part, n_win, n, B, S, slots, so, pts.data(), stats);
  for (uint32_t l = 0; l < n_win * S; ++l) out[l] = part[l].v;
  return stats[3] ? -2 : 0;
}

// G1.  Term i is [scal[i]] G (0: the point at infinity, as the decoder leaves an infinity
// encoding).  out48 [n_win]: the window sums (the sum of the window's lanes), compressed.  Returns
// the number of lanes whose result differs, as an affine point, from the nested loops' result; -1
// for bad arguments, -2 for a slot overrun.
int mh_g1(uint32_t n_win, uint32_t n, uint32_t B, uint32_t S, uint32_t slots, const int16_t* digits,
          const uint64_t* scal, uint8_t* out48, uint32_t* stats) {
  if (!shape_ok(n_win, B, S, slots)) return -1;
  Sorted so;
  if (!sort_digits(so, n_win, n, B, digits)) return -1;
  G1A g;
  fq_set(g.x, G1_GEN_X);
  fq_set(g.y, G1_GEN_Y);
  g.inf = 0;
  std::vector<G1A> pts(n);
  for (uint32_t i = 0; i < n; ++i) {
    G1J j;
    jac_mul_u64(j, g, scal[i]);
    jac_to_aff(pts[i], j);
  }
  std::vector<G1J> part;
  memset(stats, 0, 4 * sizeof(uint32_t));
  wave_walk(part, n_win, n, B, S, slots, so, pts.data(), stats);
  if (stats[3]) return -2;
  int bad = 0;
  for (uint32_t w = 0; w < n_win; ++w) {
    G1J sum;
    jac_set_inf(sum);
    for (uint32_t s = 0; s < S; ++s) {
      G1J old;
      nested_walk(old, n, B, S, s, so.ro.data() + (size_t)w * (B + 1), so.list.data() + (size_t)w * n,
                  pts.data());
      uint8_t a[48], b[48];
      compress(a, old);
      compress(b, part[w * S + s]);
      if (memcmp(a, b, 48) != 0) ++bad;
      jac_add(sum, sum, part[w * S + s]);
    }
    compress(out48 + 48 * (size_t)w, sum);
  }
  return bad;
}

}  // extern "C"
