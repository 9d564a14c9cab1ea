// PublicKey::encrypt_with_rng on gfx950 (threshold_crypto @ 0.1.0-rng-fix; the producing half of
// HoneyBadger::propose and of every SyncKeyGen Part row and Ack value), device-resident between
// its stages, and the Fr polynomial evaluations that make those rows and values:
//
//   pk bytes --k_g1_decode--> pk (affine, subgroup-checked)          [hbtc_kernels.hip]
//   r, pk ----k_enc_g1------> u = r G1 (comb table), seed = sha3_256(compressed r pk) (GLV)
//   seed, msg -k_enc_pad----> v = msg XOR hash_bytes(r pk), one lane per 16-byte ChaCha block
//   g --------k_dec_seed----> seed = sha3_256(compressed g) of a combined / multiplied g: the
//                             consuming half (decryption), which then runs the same k_enc_pad
//   u, v -----k_hash_cand---> the first on-curve candidate of hash_g1_g2(u, v)   [hbtc_hash.hip]
//   cand, r --k_enc_w-------> w = [r] [h2] cand on lane pairs, compressed
//
// H = [h2] cand stays in registers between the cofactor clearing and the multiplication: it is
// never compressed and decompressed (one Fq2 square root and one subgroup test per item less than
// hash + hbtc_g2_mul).  The arithmetic is enc.h's, which tests/native/hbtc_enc_hosttest.cpp runs
// on the CPU.
#include "enc.h"
#include "hbtc_kernels.h"
#include "pair.h"

namespace hbtc {

namespace {
__device__ __forceinline__ void enc_load_words(uint32_t* w, const uint8_t* base, size_t item, int nwords) {
  const uint4* q = reinterpret_cast<const uint4*>(base + item * (size_t)(nwords * 4));
  for (int i = 0; i < nwords / 4; ++i) {
    const uint4 v = q[i];
    w[4 * i] = v.x;
    w[4 * i + 1] = v.y;
    w[4 * i + 2] = v.z;
    w[4 * i + 3] = v.w;
  }
}
__device__ __forceinline__ void enc_store_words(uint32_t* base, size_t item, const uint32_t* w, int nwords) {
  uint4* q = reinterpret_cast<uint4*>(base + item * (size_t)nwords);
  for (int i = 0; i < nwords / 4; ++i) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
inline uint32_t enc_blocks(uint64_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }
}  // namespace

// The window table of the generator, one lane per entry (built once per context).
__global__ void __launch_bounds__(64) k_enc_table(EncPt* __restrict__ tab) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= (uint32_t)ENC_TAB_ENTRIES) return;
  EncPt e;
  enc_table_entry(e, i >> 8, i & 255u);
  tab[i] = e;
}

// One lane per item: u = r G1 from the table, g = r pk by the GLV split, both made affine with
// one shared inversion; u is stored compressed, g only as the ChaCha seed of its pad.
// (item i with the key at index pi: the body of k_enc_g1 and k_enc_g1_rcpt)
__device__ __forceinline__ void enc_g1_item(uint32_t i, size_t pi, const G1A* __restrict__ pk,
                                            const int32_t* __restrict__ pk_st,
                                            const uint8_t* __restrict__ r_le32,
                                            const EncPt* __restrict__ tab, uint32_t* __restrict__ out_u,
                                            uint32_t* __restrict__ seeds, int32_t* __restrict__ status) {
  uint32_t w[12], seed[8];
  if (pk_st[pi] != HBTC_ACCEPT) {
    for (int j = 0; j < 12; ++j) w[j] = 0;
    enc_store_words(out_u, i, w, 12);
    enc_store_words(seeds, i, w, 8);
    status[i] = HBTC_DECODE_ERR;
    return;
  }
  Fr k;
  enc_load_words(k.v, r_le32, i, 8);
  enc_scalar_mod_r(k);
  G1J uj, gj;
  enc_comb_mul(uj, tab, k);
  {
    Limbs<4> k0, k1;
    enc_split_by_x2(k, k0, k1);
    const G1A A = pk[pi];
    Fq beta;
    fq_set(beta, G1_BETA);
    enc_glv_mul(gj, A, beta, k0, k1);
  }
  G1A ua, ga;
  enc_to_aff2(ua, ga, uj, gj);
  g1_compress(w, ua);
  enc_store_words(out_u, i, w, 12);
  g1_compress(w, ga);
  enc_pad_seed(seed, w);
  enc_store_words(seeds, i, seed, 8);
  status[i] = HBTC_ACCEPT;
}

__global__ void __launch_bounds__(64) k_enc_g1(uint32_t n, const G1A* __restrict__ pk,
                                               const int32_t* __restrict__ pk_st, uint32_t pk_stride,
                                               const uint8_t* __restrict__ r_le32,
                                               const EncPt* __restrict__ tab,
                                               uint32_t* __restrict__ out_u,
                                               uint32_t* __restrict__ seeds,
                                               int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  enc_g1_item(i, (size_t)i * pk_stride, pk, pk_st, r_le32, tab, out_u, seeds, status);
}

// The recipient-indexed form (hbtc_skg_part / hbtc_skg_acks): item i goes to key i % n_keys of a
// loaded key set, whose decoded points and statuses are read in place.
__global__ void __launch_bounds__(64) k_enc_g1_rcpt(uint32_t n, const G1A* __restrict__ pk,
                                                    const int32_t* __restrict__ pk_st, uint32_t n_keys,
                                                    const uint8_t* __restrict__ r_le32,
                                                    const EncPt* __restrict__ tab,
                                                    uint32_t* __restrict__ out_u,
                                                    uint32_t* __restrict__ seeds,
                                                    int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  enc_g1_item(i, i % n_keys, pk, pk_st, r_le32, tab, out_u, seeds, status);
}

// v = msg XOR hash_bytes(g, |msg|): one lane per 16-byte block of the pad, so a long message (a
// Part row is 13 KB at t = 333) spreads over many lanes.  blk_off[i] = the first block of item i
// (blk_off[n] = n_blocks); a rejected item's v is zero.
__global__ void __launch_bounds__(256) k_enc_pad(uint32_t n, uint32_t n_blocks,
                                                 const uint32_t* __restrict__ blk_off,
                                                 const uint32_t* __restrict__ offsets,
                                                 const uint32_t* __restrict__ seeds,
                                                 const int32_t* __restrict__ status,
                                                 const uint8_t* __restrict__ msgs,
                                                 uint8_t* __restrict__ out_v) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_blocks) return;
  enc_pad_lane(b, n, blk_off, offsets, seeds, status, msgs, out_v);
}

// The consuming half (PublicKeySet::decrypt / SecretKey::decrypt after g is known): one lane per
// ciphertext turns the compressed g into the seed of its pad, seeds[i] = sha3_256(g_i), gated on
// the statuses that produced g (a combine's inst_status, or a verification's and a
// multiplication's; either may be null = passes).  gate_out[i] is the status of the item: ACCEPT,
// the first gate's failure, or DECODE_ERR where only the second failed; k_enc_pad reads it as its
// gate and zero-fills the others' ranges.
__global__ void __launch_bounds__(64) k_dec_seed(uint32_t n, const uint8_t* __restrict__ g_c48,
                                                 const int32_t* __restrict__ gate,
                                                 const int32_t* __restrict__ gate2,
                                                 uint32_t* __restrict__ seeds,
                                                 int32_t* __restrict__ gate_out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int32_t s1 = gate ? gate[i] : HBTC_ACCEPT, s2 = gate2 ? gate2[i] : HBTC_ACCEPT;
  const bool pass = s1 == HBTC_ACCEPT && s2 == HBTC_ACCEPT;
  uint32_t w[12], seed[8];
  for (int j = 0; j < 12; ++j) w[j] = 0;
  if (pass) enc_load_words(w, g_c48, i, 12);
  const int32_t closed = dec_seed_item(seed, w, pass);
  enc_store_words(seeds, i, seed, 8);
  gate_out[i] = closed == 0 ? HBTC_ACCEPT : (s1 != HBTC_ACCEPT ? s1 : HBTC_DECODE_ERR);
}

// w = [r] hash_g1_g2(u, v) from the hash candidate, on lane pairs (pair.h; item i on lanes 2i,
// 2i + 1): H = [h2] cand, made affine, then [r] H by the GLV split of r with m(H) = (zeta x, -y)
// = [x^2] H on G2, then the encoding on the even lane.  flag[i] = 1 when [h2] cand = O (never
// observed; the host then continues G2::rand's loop itself and multiplies that item on its own).
__global__ void __launch_bounds__(64, 1) k_enc_w(uint32_t n, const G2A* __restrict__ cand,
                                                 const uint8_t* __restrict__ r_le32,
                                                 const int32_t* __restrict__ status,
                                                 uint32_t* __restrict__ out_w,
                                                 uint32_t* __restrict__ flag) {
  const uint32_t i = (blockIdx.x * 64 + threadIdx.x) >> 1;
  if (i >= n) return;  // pair-uniform, as every branch below
  const bool even = !pair_odd();
  uint32_t w[24];
  for (int j = 0; j < 24; ++j) w[j] = 0;
  bool redo = false, have = false;
  G2Ap wa;
  wa.inf = 1;
  if (status[i] == HBTC_ACCEPT) {
    G2Ap p;
    g2p_load_aff(p, cand + i);
    G2Jp q;
    g2p_clear_cofactor(q, p);
    if (jac_is_inf(q)) {
      redo = true;
    } else {
      G2Ap h;
      {
        Fq2p zi, zi2, zi3;
        finv_fast(zi, q.z);
        fsqr(zi2, zi);
        fmul(zi3, zi2, zi);
        fmul(h.x, q.x, zi2);
        fmul(h.y, q.y, zi3);
        h.inf = 0;
      }
      Fr k;
      enc_load_words(k.v, r_le32, i, 8);
      enc_scalar_mod_r(k);
      Limbs<4> k0, k1;
      enc_split_by_x2(k, k0, k1);
      Fq zeta;
      fq_set(zeta, G2_ZETA);
      G2Jp acc;
      enc_glv_mul(acc, h, zeta, k0, k1);
      have = true;
      if (!jac_is_inf(acc)) {
        Fq2p zi, zi2, zi3;
        finv_fast(zi, acc.z);
        fsqr(zi2, zi);
        fmul(zi3, zi2, zi);
        fmul(wa.x, acc.x, zi2);
        fmul(wa.y, acc.y, zi3);
        wa.inf = 0;
      }
    }
  }
  if (have) {
    G2A a;
    a.inf = wa.inf;
    if (wa.inf) {
      fq2_zero(a.x);
      fq2_zero(a.y);
    } else {
      Fq px, py;
      fq_xchg(px, wa.x.v);
      fq_xchg(py, wa.y.v);
      a.x.c0 = wa.x.v;  // the even lane's view (the odd lane's is discarded)
      a.x.c1 = px;
      a.y.c0 = wa.y.v;
      a.y.c1 = py;
    }
    g2_compress(w, a);
  }
  if (!even) return;
  enc_store_words(out_w, i, w, 24);
  flag[i] = redo ? 1u : 0u;
}

// any 256-bit value -> the Montgomery form of its residue mod r
__global__ void __launch_bounds__(256) k_fr_to_mont(uint64_t n, const Fr* __restrict__ in,
                                                    Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fr m;
  enc_fr_load(m, in[i]);
  out[i] = m;
}

// out[p][j] = poly_p(x_j) (canonical): one lane per (polynomial, point) pair by Horner.  A
// workgroup handles 256 points of ONE polynomial, so the coefficient address is uniform over the
// wave and each coefficient is one load for all its lanes.
__global__ void __launch_bounds__(256) k_fr_poly_eval(uint32_t n_coeff, const Fr* __restrict__ coeffs,
                                                      uint32_t n_x, uint32_t blocks_per_poly,
                                                      const Fr* __restrict__ xs,
                                                      Fr* __restrict__ out) {
  const uint32_t p = blockIdx.x / blocks_per_poly;
  const uint32_t j = (blockIdx.x % blocks_per_poly) * 256 + threadIdx.x;
  if (j >= n_x) return;
  const Fr x = xs[j];
  Fr acc, c;
  enc_fr_horner(acc, coeffs + (size_t)p * n_coeff, n_coeff, x);
  fr_from_mont(c, acc);
  out[(size_t)p * n_x + j] = c;
}

hipError_t launch_enc_table(hipStream_t s, EncPt* tab) {
  hipLaunchKernelGGL(k_enc_table, dim3(enc_blocks(ENC_TAB_ENTRIES, 64)), dim3(64), 0, s, tab);
  return hipGetLastError();
}

hipError_t launch_enc_g1(hipStream_t s, uint32_t n, const G1A* pk, const int32_t* pk_st,
                         uint32_t pk_stride, const uint8_t* r_le32, const EncPt* tab, uint8_t* out_u,
                         uint32_t* seeds, int32_t* status) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_enc_g1, dim3(enc_blocks(n, 64)), dim3(64), 0, s, n, pk, pk_st, pk_stride, r_le32,
                     tab, reinterpret_cast<uint32_t*>(out_u), seeds, status);
  return hipGetLastError();
}

hipError_t launch_enc_g1_rcpt(hipStream_t s, uint32_t n, const G1A* pk, const int32_t* pk_st,
                              uint32_t n_keys, const uint8_t* r_le32, const EncPt* tab, uint8_t* out_u,
                              uint32_t* seeds, int32_t* status) {
  if (n == 0 || n_keys == 0) return hipSuccess;
  hipLaunchKernelGGL(k_enc_g1_rcpt, dim3(enc_blocks(n, 64)), dim3(64), 0, s, n, pk, pk_st, n_keys, r_le32,
                     tab, reinterpret_cast<uint32_t*>(out_u), seeds, status);
  return hipGetLastError();
}

hipError_t launch_enc_pad(hipStream_t s, uint32_t n, uint32_t n_blocks, const uint32_t* blk_off,
                          const uint32_t* offsets, const uint32_t* seeds, const int32_t* status,
                          const uint8_t* msgs, uint8_t* out_v) {
  if (n == 0 || n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_enc_pad, dim3(enc_blocks(n_blocks, 256)), dim3(256), 0, s, n, n_blocks, blk_off,
                     offsets, seeds, status, msgs, out_v);
  return hipGetLastError();
}

hipError_t launch_dec_seed(hipStream_t s, uint32_t n, const uint8_t* g_c48, const int32_t* gate,
                           const int32_t* gate2, uint32_t* seeds, int32_t* gate_out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dec_seed, dim3(enc_blocks(n, 64)), dim3(64), 0, s, n, g_c48, gate, gate2, seeds,
                     gate_out);
  return hipGetLastError();
}

hipError_t launch_enc_w(hipStream_t s, uint32_t n, const G2A* cand, const uint8_t* r_le32,
                        const int32_t* status, uint8_t* out_w, uint32_t* flag) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_enc_w, dim3(enc_blocks(2 * (uint64_t)n, 64)), dim3(64), 0, s, n, cand, r_le32,
                     status, reinterpret_cast<uint32_t*>(out_w), flag);
  return hipGetLastError();
}

hipError_t launch_fr_to_mont(hipStream_t s, uint64_t n, const uint8_t* in_le32, Fr* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fr_to_mont, dim3(enc_blocks(n, 256)), dim3(256), 0, s, n,
                     reinterpret_cast<const Fr*>(in_le32), out);
  return hipGetLastError();
}

hipError_t launch_fr_poly_eval(hipStream_t s, uint32_t n_poly, uint32_t n_coeff, const Fr* coeffs,
                               uint32_t n_x, const Fr* xs, uint8_t* out_le32) {
  if (n_poly == 0 || n_x == 0 || n_coeff == 0) return hipSuccess;
  const uint32_t bpp = enc_blocks(n_x, 256);
  hipLaunchKernelGGL(k_fr_poly_eval, dim3(n_poly * bpp), dim3(256), 0, s, n_coeff, coeffs, n_x, bpp, xs,
                     reinterpret_cast<Fr*>(out_le32));
  return hipGetLastError();
}

}  // namespace hbtc
