// The bucket walk of the Pippenger reduction, one (msm, window, segment) slice per lane (kernels:
// hbtc_msm.hip k_msm_buckets; the same functions run on the CPU in
// tests/native/hbtc_msm_hosttest.cpp).
//
// A lane owns the sorted positions [p0, p1) of its window's list and returns
//     sum_r (B - r) B'_r         (B'_r = the slice's part of bucket rank r, bucket b = B - r)
// as  tot + [B - r_last] run  with  run = sum_r B'_r  and  tot = sum_{r < r_last} (r_last - r) B'_r,
// i.e. tot is the sum of the values `run` had each time the walk left a rank.
//
// The form of rounds 1-9 (HBTC_MSM_WALK=0 still builds it) is a loop over the ranks around a loop
// over the rank's positions, with tot += run after each.  On a wave the inner trip count is per lane
// (bucket sizes are about Poisson(n / B)), so every rank step costs the longest bucket of the 64
// lanes, and the full addition is issued once per rank step for everybody.
//
// The lane-uniform walk is ONE loop over the positions: every lane with positions left does one
// mixed addition per iteration, and the slices of a wave have the same length to within a few
// terms, so the lanes finish together.  Leaving a rank adds nothing: the lane stores `run` in
// the next of its MSM_SLOTS snapshot slots (a store, cheap even when only a few lanes do it) and
// goes on; leaving an empty rank stores the same `run` again.  When a lane needs a slot and has
// none, the whole wave flushes: for k = 0, 1, ... the lanes with more than k snapshots pending do
// tot += snapshot[k] together.  One more flush follows the loop, then the multiple of run.
//
// The pieces below are the per-lane state machine (begin, boundary, step, flush, finish) over any
// group that provides jac_set_inf / jac_add / jac_dbl on its point type J (Jac<F>, the lane-pair
// G2Jp, and curve.h's JacW for the G1 walk on 30-bit limbs); the snapshot store is a
// policy with put(k, J) / get(J, k); the caller owns the loop, loads the terms and takes the wave
// vote (the only device-only piece: `any lane needs a flush`, `any lane has positions left`):
//
//     walk_begin(w, ro, B, S, s);
//     for (;;) {
//       const bool need = walk_boundary(w, ro, run, st, slots);
//       if (any(need)) { walk_flush over k while any(walk_pending(w) > k); continue; }
//       if (!any(walk_active(w))) break;
//       if (walk_active(w)) run += term at walk_step(w);
//     }
//     walk_flush ...; walk_finish(tot, run, w, B);
#pragma once
#include <stdint.h>

#include "field.h"

namespace hbtc {

#ifndef HBTC_MSM_WALK
#define HBTC_MSM_WALK 1  // 0: the nested loops of rounds 1-9 (variant builds, tools/build_variant.sh)
#endif
#ifndef HBTC_MSM_SLOTS
#define HBTC_MSM_SLOTS 1  // snapshot slots per lane (1, 2 and 4 compared)
#endif
constexpr uint32_t MSM_SLOTS = HBTC_MSM_SLOTS;

// Rank whose bucket holds sorted position p: the largest r < B with ro[r] <= p (ro[0] = 0 and
// p < ro[B]).
HD uint32_t msm_rank(const uint32_t* ro, uint32_t B, uint32_t p) {
  uint32_t lo = 0, hi = B;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ro[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct MsmWalk {
  uint32_t e, p1;    // next position, end of the slice
  uint32_t r;        // rank of the bucket `run` is collecting
  uint32_t next;     // ro[r + 1]: the first position past that bucket
  uint32_t pending;  // snapshots stored and not yet added to tot
  uint32_t any;      // the slice is not empty
};

// Slice s of S of the window whose rank offsets are ro[0 .. B]
HD void walk_begin(MsmWalk& w, const uint32_t* ro, uint32_t B, uint32_t S, uint32_t s) {
  const uint32_t total = ro[B];
  w.e = (uint32_t)((uint64_t)total * s / S);
  w.p1 = (uint32_t)((uint64_t)total * (s + 1) / S);
  w.pending = 0;
  w.any = w.e < w.p1;
  w.r = 0;
  w.next = 0;
  if (w.any) {
    w.r = msm_rank(ro, B, w.e);
    w.next = ro[w.r + 1];
  }
}

HD bool walk_active(const MsmWalk& w) { return w.e < w.p1; }
HD uint32_t walk_pending(const MsmWalk& w) { return w.pending; }

// Before the step at position e: leave every rank that ends at or before e, one snapshot of `run`
// each.  Returns true when a snapshot is due and the lane's slots are full: the caller flushes
// (the whole wave) and calls again.  e < p1 <= ro[B], so r + 1 <= B throughout.
template <class J, class St>
HD bool walk_boundary(MsmWalk& w, const uint32_t* ro, const J& run, St& st, uint32_t slots) {
  while (w.e < w.p1 && w.next <= w.e) {
    if (w.pending == slots) return true;
    st.put(w.pending, run);
    ++w.pending;
    ++w.r;
    w.next = ro[w.r + 1];
  }
  return false;
}

// The position whose term the caller adds to `run` now (walk_active lanes only)
HD uint32_t walk_step(MsmWalk& w) { return w.e++; }

// Round k of a flush: tot += snapshot[k] on the lanes that have one.  walk_flush_done after the
// last round.
template <class J, class St>
HD void walk_flush(const MsmWalk& w, uint32_t k, J& tot, const St& st) {
  if (k < w.pending) {
    J sn;
    st.get(sn, k);
    jac_add(tot, tot, sn);
  }
}
HD void walk_flush_done(MsmWalk& w) { w.pending = 0; }

// [k] p for 1 <= k < 2^16, MSB-first from p itself
template <class J>
HD void walk_mul_small(J& r, const J& p, uint32_t k) {
  J acc = p;
  for (int b = 30 - __builtin_clz(k); b >= 0; --b) {
    jac_dbl(acc, acc);
    if ((k >> b) & 1u) jac_add(acc, acc, p);
  }
  r = acc;
}

// After the last flush: the last rank's own sum and the ranks below the slice in one multiple,
// tot += [B - r_last] run
template <class J>
HD void walk_finish(J& tot, const J& run, const MsmWalk& w, uint32_t B) {
  if (!w.any) return;
  J m;
  walk_mul_small(m, run, B - w.r);
  jac_add(tot, tot, m);
}

}  // namespace hbtc
