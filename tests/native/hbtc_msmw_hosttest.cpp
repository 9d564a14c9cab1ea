// Host build of the G1 bucket walk on the redundant 13 x 30 form (msm_walk.h over curve.h's JacW, as
// hbtc_msm.hip's k_msm_buckets<Fq> runs it under HBTC_MSM_WALKW) with HBTC_RR_ASSERT: every FqW carries
// its per-limb and value bounds and every operation asserts them.  One wave is replayed in lockstep
// (up to 64 lane states, the wave votes as loops over the lanes) twice, over JacW and over the
// 12 x 32 G1J, from the same sorted lists; every lane's two results are compared as affine points.
// Behind a C interface for tests/test_msm_walkw_host.py (ctypes).  Test infrastructure only: never
// linked into the product library.
#define HBTC_RR_ASSERT 1
#include <cstring>
#include <vector>

#include "curve.h"
#include "msm_walk.h"

using namespace hbtc;

namespace {

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

// k_msm_sort on the host: rank r = B - |d|, list entry = index | sign << 31, index order in a bucket
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

// the step of the kernel for each point type
void walk_add(G1J& run, const G1A& q) { jac_add_aff(run, run, q); }
void walk_add(JacW& run, const G1A& q) { jacw_add_g1a(run, run, q); }

// One wave of n_win * S lanes through the loop of k_msm_buckets.  stats: [0] steps, [1] flushes
// inside the loop, [2] flush rounds, [3] slot overruns (must stay 0).
template <class J>
void wave_walk(std::vector<J>& part, uint32_t n_win, uint32_t n, uint32_t B, uint32_t S, uint32_t slots,
               const Sorted& so, const G1A* pts, uint32_t* stats) {
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
        const uint32_t v = so.list[(size_t)(l / S) * n + walk_step(w[l])];
        G1A q = pts[v & 0x7fffffffu];
        if (v >> 31) fneg(q.y, q.y);
        walk_add(run[l], q);
      }
  }
  flush();
  for (uint32_t l = 0; l < lanes; ++l) walk_finish(tot[l], run[l], w[l], B);
  stats[3] = (uint32_t)overrun;
  part = tot;
}

void compress(uint8_t* out48, const G1J& p) {
  G1A a;
  jac_to_aff(a, p);
  uint32_t w[12];
  g1_compress(w, a);
  for (int i = 0; i < 12; ++i)
    for (int j = 0; j < 4; ++j) out48[4 * i + j] = (uint8_t)(w[i] >> (8 * j));
}

}  // namespace

extern "C" {

// Term i is [scal[i]] G (0: the point at infinity).  digits [n_win][n] in [-B, B].  lanes48
// [n_win * S]: every lane's result of the JacW walk after jacw_to_jac, compressed; win48 [n_win]: the
// window sums.  Returns the number of lanes whose JacW result differs, as an affine point, from the
// 12 x 32 walk's; -1 for bad arguments, -2 for a slot overrun, -3 if a coordinate that leaves through
// jacw_to_jac is not below 2p.
int mhw_g1(uint32_t n_win, uint32_t n, uint32_t B, uint32_t S, uint32_t slots, const int16_t* digits,
           const uint64_t* scal, uint8_t* lanes48, uint8_t* win48, uint32_t* stats) {
  if (!(n_win && S && slots && B >= S && n_win * S <= 64 && B <= 1024)) return -1;
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
  std::vector<JacW> pw;
  std::vector<G1J> p32;
  uint32_t s32[4] = {0, 0, 0, 0};
  memset(stats, 0, 4 * sizeof(uint32_t));
  wave_walk(pw, n_win, n, B, S, slots, so, pts.data(), stats);
  wave_walk(p32, n_win, n, B, S, slots, so, pts.data(), s32);
  if (stats[3] || s32[3]) return -2;
  for (int i = 0; i < 3; ++i)
    if (stats[i] != s32[i]) return -2;
  Fq two_p;
  fq_set(two_p, FQ_2P);
  int bad = 0;
  for (uint32_t w = 0; w < n_win; ++w) {
    G1J sum;
    jac_set_inf(sum);
    for (uint32_t s = 0; s < S; ++s) {
      G1J out;
      jacw_to_jac(out, pw[w * S + s]);
      for (const Fq* c : {&out.x, &out.y, &out.z}) {
        Fq t;
        if (limbs_sub<12>(t, *c, two_p) == 0) return -3;
      }
      uint8_t a[48];
      compress(a, p32[w * S + s]);
      compress(lanes48 + 48 * (size_t)(w * S + s), out);
      if (memcmp(a, lanes48 + 48 * (size_t)(w * S + s), 48) != 0) ++bad;
      jac_add(sum, sum, out);
    }
    compress(win48 + 48 * (size_t)w, sum);
  }
  return bad;
}

}  // extern "C"
