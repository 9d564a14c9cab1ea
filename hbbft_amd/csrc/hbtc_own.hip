// SecretKeyShare::sign on gfx950 (threshold_crypto @ 0.1.0-rng-fix; Coin::get_coin's own share),
// device-resident between the hash and the multiplication:
//
//   msg ------k_hash_cand---> the first on-curve candidate of hash_g2(msg)        [hbtc_hash.hip]
//   cand, sk -k_sig_share---> H = [h2] cand and sigma = [sk] H on lane pairs, both compressed
//
// H stays in registers between the cofactor clearing and the multiplication, as in k_enc_w: it is
// never compressed and decompressed (one Fq2 square root and one subgroup test per item less than
// hash + hbtc_g2_mul).
//
// The secret scalar is one per call: the host reduces it and splits it into its four base-|x|
// digits (curve.h gls_u_digits) and passes them as kernel arguments.  They are the same on every
// lane, so the bit tests are scalar and a bit pair (0, 0) skips its addition.
#include "enc.h"
#include "hbtc_kernels.h"
#include "pair.h"

namespace hbtc {

namespace {
// the pair's affine point -> its 24 compressed words (valid on the even lane; the exchange runs
// on both)
__device__ __forceinline__ void own_compress_pair(uint32_t* w, const G2Ap& p) {
  G2A a;
  a.inf = p.inf;
  if (p.inf) {  // pair-uniform
    fq2_zero(a.x);
    fq2_zero(a.y);
  } else {
    Fq px, py;
    fq_xchg(px, p.x.v);
    fq_xchg(py, p.y.v);
    a.x.c0 = p.x.v;
    a.x.c1 = px;
    a.y.c0 = p.y.v;
    a.y.c1 = py;
  }
  g2_compress(w, a);
}
}  // namespace

// Item i on lanes 2i, 2i + 1 (pair.h): H = [h2] cand, made affine, and sigma = [sk] H by the
// four-term psi split: sk = sum_j d_j u^j with d_j < u = |x| < 2^64,
//   [sk] H = d0 H + d1 [u]H + d2 [u^2]H + d3 [u^3]H,  [u]H = -psi(H), [u^2]H = psi^2(H), [u^3]H = -psi^3(H)
// (the decomposition of k_msm_gls_g2): 64 doublings, and per bit at most one mixed addition from
// each of {P0, P1, P0 + P1} and {P2, P3, P2 + P3}; the two table sums share one inversion.  Both
// encodings are written by the even lane.  flag[i] = 1 when [h2] cand = O (never observed; both
// outputs are zero bytes then, and the host continues G2::rand's loop itself and multiplies that
// item on its own).  Every branch is pair-uniform.  The x^2 split of k_enc_w (128 doublings, one
// addition per bit) was built and measured beside this form and was slower at n = 10 and at
// n = 1000 (DESIGN.md "Own shares").
__global__ void __launch_bounds__(64, 1) k_sig_share(uint32_t n, const G2A* __restrict__ cand,
                                                     uint64_t d0, uint64_t d1, uint64_t d2, uint64_t d3,
                                                     uint32_t* __restrict__ out_h,
                                                     uint32_t* __restrict__ out_sig,
                                                     uint32_t* __restrict__ flag) {
  const uint32_t i = (blockIdx.x * 64 + threadIdx.x) >> 1;
  if (i >= n) return;  // pair-uniform, as every branch below
  const bool even = !pair_odd();
  uint32_t wh[24], wsig[24];
  for (int j = 0; j < 24; ++j) wh[j] = wsig[j] = 0;
  G2Ap p;
  g2p_load_aff(p, cand + i);
  G2Jp q;
  g2p_clear_cofactor(q, p);
  const bool redo = jac_is_inf(q);
  if (!redo) {
    G2Ap P0, P1, P2, P3, S01, S23;
    jac_to_aff(P0, q);
    own_compress_pair(wh, P0);
    g2p_psi(P1.x, P1.y, P0);
    P1.inf = 0;
    g2p_psi(P2.x, P2.y, P1);
    P2.inf = 0;
    g2p_psi(P3.x, P3.y, P2);
    P3.inf = 0;
    fneg(P1.y, P1.y);  // -psi(H); psi^2(H) above came from psi(H) before the sign
    fneg(P3.y, P3.y);  // -psi^3(H)
    {
      // P0 + P1 = [1 + u] H and P2 + P3 = [u^2 (1 + u)] H: not O (1 + u and u are units mod r),
      // made affine with one inversion
      G2Jp a, b;
      jac_from_aff(a, P0);
      jac_add_aff(a, a, P1);
      jac_from_aff(b, P2);
      jac_add_aff(b, b, P3);
      Fq2p prod, inv, ia, ib, i2;
      fmul(prod, a.z, b.z);
      finv_fast(inv, prod);
      fmul(ia, inv, b.z);
      fmul(ib, inv, a.z);
      fsqr(i2, ia);
      fmul(S01.x, a.x, i2);
      fmul(i2, i2, ia);
      fmul(S01.y, a.y, i2);
      fsqr(i2, ib);
      fmul(S23.x, b.x, i2);
      fmul(i2, i2, ib);
      fmul(S23.y, b.y, i2);
      S01.inf = S23.inf = 0;
    }
    G2Jp acc;
    jac_set_inf(acc);
#pragma unroll 1
    for (int bit = 63; bit >= 0; --bit) {
      jac_dbl(acc, acc);
      const bool b0 = ((d0 >> bit) & 1ull) != 0, b1 = ((d1 >> bit) & 1ull) != 0;  // wave-uniform
      const bool b2 = ((d2 >> bit) & 1ull) != 0, b3 = ((d3 >> bit) & 1ull) != 0;
      if (b0 || b1) {
        G2Ap t;
        Fq2p sx, sy;
        fsel(sx, b0, S01.x, P1.x);
        fsel(sy, b0, S01.y, P1.y);
        fsel(t.x, b1, sx, P0.x);
        fsel(t.y, b1, sy, P0.y);
        t.inf = 0;
        jac_add_aff(acc, acc, t);
      }
      if (b2 || b3) {
        G2Ap t;
        Fq2p sx, sy;
        fsel(sx, b2, S23.x, P3.x);
        fsel(sy, b2, S23.y, P3.y);
        fsel(t.x, b3, sx, P2.x);
        fsel(t.y, b3, sy, P2.y);
        t.inf = 0;
        jac_add_aff(acc, acc, t);
      }
    }
    G2Ap sg;
    jac_to_aff(sg, acc);
    own_compress_pair(wsig, sg);
  }
  if (!even) return;
  uint4* oh = reinterpret_cast<uint4*>(out_h + 24 * (size_t)i);
  uint4* os = reinterpret_cast<uint4*>(out_sig + 24 * (size_t)i);
  for (int j = 0; j < 6; ++j) {
    oh[j] = make_uint4(wh[4 * j], wh[4 * j + 1], wh[4 * j + 2], wh[4 * j + 3]);
    os[j] = make_uint4(wsig[4 * j], wsig[4 * j + 1], wsig[4 * j + 2], wsig[4 * j + 3]);
  }
  flag[i] = redo ? 1u : 0u;
}

hipError_t launch_sig_share(hipStream_t s, uint32_t n, const G2A* cand, const uint64_t* d,
                            uint8_t* out_h_c96, uint8_t* out_sig_c96, uint32_t* flag) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sig_share, dim3((uint32_t)((2 * (uint64_t)n + 63) / 64)), dim3(64), 0, s, n, cand,
                     d[0], d[1], d[2], d[3], reinterpret_cast<uint32_t*>(out_h_c96),
                     reinterpret_cast<uint32_t*>(out_sig_c96), flag);
  return hipGetLastError();
}

// g_i (48 compressed bytes, 12 words) := zero bytes where gate[i] is not ACCEPT: one lane per word
__global__ void __launch_bounds__(256) k_gate_c48(uint32_t n, const int32_t* __restrict__ gate,
                                                  uint32_t* __restrict__ g_w) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= (uint64_t)12 * n) return;
  if (gate[j / 12] != HBTC_ACCEPT) g_w[j] = 0;
}

hipError_t launch_gate_c48(hipStream_t s, uint32_t n, const int32_t* gate, uint8_t* g_c48) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gate_c48, dim3((uint32_t)(((uint64_t)12 * n + 255) / 256)), dim3(256), 0, s, n, gate,
                     reinterpret_cast<uint32_t*>(g_c48));
  return hipGetLastError();
}

}  // namespace hbtc
