// SyncKeyGen::generate + NetworkInfo::new on the device, the host/device pieces (kernels:
// hbtc_keygen.hip; the same functions run on the CPU in tests/native/hbtc_keygen_hosttest.cpp).
//
//   commit[j] = sum_p row0[p][j]                 lanes add their Parts with the complete mixed
//                                                addition, a tree of jac_add joins the lanes
//   sk = sum_p L_p(0)                            L_p through Part p's (x, value) pairs: per item the
//                                                numerator and denominator products, one batched
//                                                inversion per Part (prefix / suffix products over
//                                                the lanes), the dot product with the values
//   pk_share[i] = sum_j (i + 1)^j commit[j]      Horner acc = x acc + C_j with x acc a short
//                                                double-and-add, per segment of KG_SEG coefficients;
//                                                segment s is scaled by x^(s KG_SEG) and the
//                                                segments are added
//   Jacobian -> affine                           one inversion per KG_BS points
//
// Everything that runs across lanes is written as a read step and a write step per lane, with a
// barrier between them on the device and a loop over the lanes on the host.
#pragma once
#include "enc.h"

namespace hbtc {

constexpr uint32_t KG_BS = 256;  // lanes of one interpolation workgroup and of one affine batch
constexpr uint32_t KG_COL = 64;  // lanes of one column sum
#ifndef HBTC_KG_SEG
#define HBTC_KG_SEG 8  // measured at N = 1000 against 16, 32 and 64 (DESIGN.md "Key generation")
#endif
constexpr uint32_t KG_SEG = HBTC_KG_SEG;  // commitment coefficients per Horner segment

HD void kg_fmul(Fr& r, const Fr& a, const Fr& b) { fr_mul(r, a, b); }
HD void kg_fmul(Fq& r, const Fq& a, const Fq& b) { fq_mul(r, a, b); }
HD void kg_fone(Fr& r) { limbs_set_const<8>(r, FR_ONE); }
HD void kg_fone(Fq& r) { fq_one(r); }

// ---- prefix and suffix products over the KG_BS lanes of a workgroup (log-step scans)
// Before the first step lane u stores its own value in C[u] and S[u] and keeps it in st.cp and
// st.sp.  After the steps off = 1, 2, .., KG_BS / 2: C[u] = the product over lanes 0..u and
// S[u] = the product over lanes u..KG_BS - 1.
template <class T>
struct KgScan {
  T cp, sp;
};
template <class T>
struct KgScanIn {
  T a, d;
};
template <class T>
HD void kg_scan_read(KgScanIn<T>& in, uint32_t tid, uint32_t off, const T* C, const T* S) {
  if (tid >= off) in.a = C[tid - off];
  if (tid + off < KG_BS) in.d = S[tid + off];
}
template <class T>
HD void kg_scan_write(KgScan<T>& st, const KgScanIn<T>& in, uint32_t tid, uint32_t off, T* C, T* S) {
  if (tid >= off) {
    kg_fmul(st.cp, st.cp, in.a);
    C[tid] = st.cp;
  }
  if (tid + off < KG_BS) {
    kg_fmul(st.sp, st.sp, in.d);
    S[tid] = st.sp;
  }
}
// 1 / (lane tid's own value) from the scans and the inverse of the total: the product of every
// other lane's value times inv_total.  incl = 1 / (the product over lanes 0..tid).
template <class T>
HD void kg_scan_inverse(T& own_inv, T& e_excl, T& incl, uint32_t tid, const T* C, const T* S,
                        const T& inv_total) {
  T s_excl;
  kg_fone(e_excl);
  kg_fone(s_excl);
  if (tid > 0) e_excl = C[tid - 1];
  if (tid + 1 < KG_BS) s_excl = S[tid + 1];
  kg_fmul(incl, inv_total, s_excl);
  kg_fmul(own_inv, incl, e_excl);
}

// ---- column sum
// The sum of column j over the Parts p = lane, lane + KG_COL, ..: the mixed addition is the
// complete one (equal operands double, opposite ones cancel, infinity is neutral).
HD void kg_col_lane(G1J& acc, const G1A* dec, uint32_t n_parts, uint32_t t1, uint32_t j, uint32_t lane) {
  jac_set_inf(acc);
#pragma unroll 1
  for (uint32_t p = lane; p < n_parts; p += KG_COL) {
    const G1A a = dec[(size_t)p * t1 + j];
    jac_add_aff(acc, acc, a);
  }
}
// one level of the tree over the lanes' sums: sh[tid] += sh[tid + off]
HD void kg_tree_step(G1J* sh, uint32_t tid, uint32_t off) {
  if (tid < off) jac_add(sh[tid], sh[tid], sh[tid + off]);
}

// ---- Fr interpolation at 0
// (x, value) -> Montgomery forms; the value is any 256-bit integer, taken mod r
HD void kg_fr_prep(Fr& xm, Fr& ym, uint32_t x, const Fr& raw) {
  fr_from_u64(xm, x);
  enc_fr_load(ym, raw);
}
// num = prod_{j != i} x_j and den = prod_{j != i} (x_j - x_i) of item i among the m of its Part;
// returns whether another item repeats x_i (den is 0 then)
HD bool kg_num_den(Fr& num, Fr& den, uint32_t i, uint32_t m, const uint32_t* x, const Fr* xm) {
  const Fr xi = xm[i];
  const uint32_t xr = x[i];
  kg_fone(num);
  kg_fone(den);
  bool dup = false;
#pragma unroll 1
  for (uint32_t j = 0; j < m; ++j) {
    if (j == i) continue;
    const Fr xj = xm[j];
    dup |= x[j] == xr;
    Fr d;
    fr_sub(d, xj, xi);
    fr_mul(den, den, d);
    fr_mul(num, num, xj);
  }
  return dup;
}
// Lane tid's items i = tid, tid + KG_BS, ..: den_i to q[i], the product of the lane's earlier
// denominators to pre[i], value_i num_i to wy[i]; prod = the product of the lane's denominators
// (1 for a lane without items).  Returns whether one of the items' x repeats.
HD bool kg_lane_products(Fr& prod, uint32_t tid, uint32_t m, const uint32_t* x, const Fr* xm,
                         const Fr* ym, Fr* q, Fr* pre, Fr* wy) {
  kg_fone(prod);
  bool dup = false;
#pragma unroll 1
  for (uint32_t i = tid; i < m; i += KG_BS) {
    Fr num, den, w;
    dup |= kg_num_den(num, den, i, m, x, xm);
    fr_mul(w, num, ym[i]);
    q[i] = den;
    pre[i] = prod;
    wy[i] = w;
    fr_mul(prod, prod, den);
  }
  return dup;
}
// sum over the lane's items of wy_i / den_i (Montgomery), walking them backwards: e_excl = the
// product of the denominators of the lanes before tid, incl = 1 / (that product times the lane's)
HD void kg_lane_dot(Fr& sum, uint32_t tid, uint32_t m, const Fr& e_excl, const Fr& incl, const Fr* q,
                    const Fr* pre, const Fr* wy) {
  limbs_zero<8>(sum);
  if (tid >= m) return;
  Fr inv_incl = incl;
  uint32_t i = tid + ((m - 1 - tid) / KG_BS) * KG_BS;
#pragma unroll 1
  for (;;) {
    Fr excl, qi_inv, term;
    fr_mul(excl, e_excl, pre[i]);       // the denominators before item i
    fr_mul(qi_inv, inv_incl, excl);     // 1 / den_i
    fr_mul(inv_incl, inv_incl, q[i]);
    fr_mul(term, wy[i], qi_inv);
    fr_add(sum, sum, term);
    if (i == tid) break;
    i -= KG_BS;
  }
}
// one level of the sum over lanes (and over Parts): sh[tid] += sh[tid + off]
HD void kg_fr_tree_step(Fr* sh, uint32_t tid, uint32_t off) {
  if (tid < off) fr_add(sh[tid], sh[tid], sh[tid + off]);
}

// ---- commitment evaluation
// [x] p for x >= 1 by an MSB-first double-and-add over the bits of x (p Jacobian, any point)
HD void kg_mul_small(G1J& r, const G1J& p, uint32_t x) {
  G1J acc = p;
  const int top = 31 - __builtin_clz(x | 1u);
#pragma unroll 1
  for (int b = top - 1; b >= 0; --b) {
    jac_dbl(acc, acc);
    if ((x >> b) & 1u) jac_add(acc, acc, p);
  }
  r = acc;
}
// sum_{j in [lo, hi)} x^(j - lo) C_j by Horner: acc = x acc + C_j
HD void kg_horner_seg(G1J& acc, const G1A* C, uint32_t lo, uint32_t hi, uint32_t x) {
  jac_set_inf(acc);
#pragma unroll 1
  for (uint32_t j = hi; j-- > lo;) {
    if (!jac_is_inf(acc)) kg_mul_small(acc, acc, x);
    const G1A c = C[j];
    jac_add_aff(acc, acc, c);
  }
}
// x^e mod r, canonical
HD void kg_pow_u32(Fr& out, uint32_t x, uint32_t e) {
  Fr b, acc;
  fr_from_u64(b, x);
  kg_fone(acc);
#pragma unroll 1
  for (int bit = 31 - __builtin_clz(e | 1u); bit >= 0; --bit) {
    fr_mul(acc, acc, acc);
    if ((e >> bit) & 1u) fr_mul(acc, acc, b);
  }
  fr_from_mont(out, acc);
}
// [k] p for a canonical k (p Jacobian): MSB-first double-and-add with the complete addition
HD void kg_mul_fr(G1J& r, const G1J& p, const Fr& k) {
  G1J acc;
  jac_set_inf(acc);
  Fr kk = k;
#pragma unroll 1
  for (int wi = 0; wi < 8; ++wi) {
    const uint32_t word = kk.v[7];
#pragma unroll
    for (int j = 7; j > 0; --j) kk.v[j] = kk.v[j - 1];  // static indexing only
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      jac_dbl(acc, acc);
      if ((word >> bit) & 1u) jac_add(acc, acc, p);
    }
  }
  r = acc;
}
// Segment s of x's evaluation, scaled to its place: x^(s KG_SEG) sum_{j in segment} x^(j - lo) C_j
HD void kg_eval_segment(G1J& out, const G1A* C, uint32_t t1, uint32_t s, uint32_t x) {
  const uint32_t lo = s * KG_SEG, hi = lo + KG_SEG < t1 ? lo + KG_SEG : t1;
  G1J acc;
  kg_horner_seg(acc, C, lo, hi, x);
  if (s != 0 && !jac_is_inf(acc)) {
    Fr k;
    kg_pow_u32(k, x, lo);
    kg_mul_fr(acc, acc, k);
  }
  out = acc;
}
HD uint32_t kg_segments(uint32_t t1) { return (t1 + KG_SEG - 1) / KG_SEG; }

// ---- Jacobian -> affine with a shared inversion
// the factor a point contributes to the batch's product: its z, or 1 for the point at infinity
HD void kg_affine_factor(Fq& z, const G1J& p) {
  Fq one;
  fq_one(one);
  fq_sel(z, jac_is_inf(p), one, p.z);
}
// the affine point from 1 / z, in the canonical form g1_decompress produces (infinity: zeros)
HD void kg_affine_finish(G1A& a, const G1J& p, const Fq& zinv) {
  fq_zero(a.x);
  fq_zero(a.y);
  a.inf = jac_is_inf(p) ? 1u : 0u;
  if (a.inf) return;
  Fq i2, t;
  fq_sqr(i2, zinv);
  fq_mul(t, p.x, i2);
  fq_canon(a.x, t);
  fq_mul(i2, i2, zinv);
  fq_mul(t, p.y, i2);
  fq_canon(a.y, t);
}

}  // namespace hbtc
