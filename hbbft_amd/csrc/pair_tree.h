// The tile tree of G2 sums on lane pairs (pair.h): the LDS layouts and the one-wave reduction
// shared by the SignatureShare item pass, the pair batches (hbtc_sig.hip) and the signed-message
// batches (hbtc_sv.hip).
#pragma once
#include "pair.h"

namespace hbtc {

// The wave-local form of a __syncthreads between LDS writes and reads of ONE wave: a wave's LDS
// operations execute in order, so only the compiler's reordering and the outstanding counters
// need fencing.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS layout of the G2 reduction: word w of item m's point component e at w * 128 + 2 m + e
// (36 words) -- a wave's stores are conflict-free.
__device__ __forceinline__ void g2p_lds_put(uint32_t* lds, uint32_t m, const G2Jp& a) {
  const uint32_t o = 2 * m + (pair_odd() ? 1u : 0u);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&a);
#pragma unroll
  for (int w = 0; w < 36; ++w) lds[w * 128 + o] = src[w];
}
__device__ __forceinline__ void g2p_lds_get(G2Jp& a, const uint32_t* lds, uint32_t m) {
  const uint32_t o = 2 * m + (pair_odd() ? 1u : 0u);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&a);
#pragma unroll
  for (int w = 0; w < 36; ++w) dst[w] = lds[w * 128 + o];
}
// 36 words of one lane at w * 64 + l (the B area of the G2 tree)
template <class J>
__device__ __forceinline__ void g1w_put36(uint32_t* lds, uint32_t l, const J& x) {
  static_assert(sizeof(J) == 144, "36 words");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&x);
#pragma unroll
  for (int w = 0; w < 36; ++w) lds[w * 64 + l] = src[w];
}
template <class J>
__device__ __forceinline__ void g1w_get36(J& x, const uint32_t* lds, uint32_t l) {
  static_assert(sizeof(J) == 144, "36 words");
  uint32_t* dst = reinterpret_cast<uint32_t*>(&x);
#pragma unroll
  for (int w = 0; w < 36; ++w) dst[w] = lds[w * 64 + l];
}

// The tile's G2 tree (rlc_reduce's merges: A = A_l + A_r, B = 2 (B_l + B_r) + A_r) on ONE wave of
// 32 lane pairs: pair j owns node m = 2 j.  A and B both in LDS (B at w * 64 + lane: the right
// node's B is the one of pair j + s / 2, i.e. lane + s), so at most two points are live beside the
// product's fixed registers (B in registers left a 848 B/lane frame).
__device__ __forceinline__ void rlc_reduce_g2p(uint32_t* lds, uint32_t* ldsB, uint32_t lane, G2J* outA, G2J* outB) {
  const uint32_t j = lane >> 1, m = 2 * j;
  {  // level 1: the leaves' B are infinity, so B = A_r
    G2Jp a, ar;
    g2p_lds_get(ar, lds, m + 1);
    g1w_put36(ldsB, lane, ar);
    g2p_lds_get(a, lds, m);
    jac_add_lean(a, ar);
    g2p_lds_put(lds, m, a);
    wave_lds_sync();
  }
#pragma unroll 1
  for (uint32_t s = 2; s < 64; s <<= 1) {
    if ((j & (s - 1)) == 0) {  // active pairs read only inactive pairs' entries besides their own
      G2Jp b, x;
      g1w_get36(b, ldsB, lane);
      g1w_get36(x, ldsB, lane + s);
      jac_add_lean(b, x);
      jac_dbl(b, b);
      g2p_lds_get(x, lds, m + s);  // A_r
      jac_add_lean(b, x);
      g1w_put36(ldsB, lane, b);
      g2p_lds_get(b, lds, m);
      jac_add_lean(b, x);
      g2p_lds_put(lds, m, b);
    }
    wave_lds_sync();
    if (s == 4 && (j & 3u) == 0) {
      G2Jp x;
      g2p_lds_get(x, lds, m);
      g2p_store_jac(outA + (m >> 3), x);
      g1w_get36(x, ldsB, lane);
      g2p_store_jac(outB + (m >> 3), x);
    }
  }
  if (j == 0) {
    G2Jp x;
    g2p_lds_get(x, lds, 0);
    g2p_store_jac(outA + 8, x);
    g1w_get36(x, ldsB, lane);
    g2p_store_jac(outB + 8, x);
  }
}

// The plain sum of 64 G2 points in the layout above on ONE wave of 32 lane pairs (pair j owns node
// m = 2 j): six levels of one addition each, no weighted sums.  Pair 0 stores the sum at out.
__device__ __forceinline__ void g2p_tree_sum(uint32_t* lds, uint32_t lane, G2J* out) {
  const uint32_t m = 2 * (lane >> 1);
#pragma unroll 1
  for (uint32_t s = 1; s < 64; s <<= 1) {
    if ((m & (2 * s - 1)) == 0) {  // active pairs read only inactive pairs' entries besides their own
      G2Jp a, x;
      g2p_lds_get(a, lds, m);
      g2p_lds_get(x, lds, m + s);
      jac_add_lean(a, x);
      g2p_lds_put(lds, m, a);
    }
    wave_lds_sync();
  }
  if (m == 0) {
    G2Jp a;
    g2p_lds_get(a, lds, 0);
    g2p_store_jac(out, a);
  }
}

}  // namespace hbtc
