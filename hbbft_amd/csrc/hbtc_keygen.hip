// SyncKeyGen::generate followed by NetworkInfo::new on gfx950 (src/sync_key_gen.rs:428-447,
// src/messaging.rs:253-256), device-resident between its stages:
//
//   row0 bytes --k_kg_decode--> row0 points (affine, subgroup-checked), flags[0] on a bad encoding
//   points -----k_kg_colsum---> commit[j] = sum_p row0[p][j] (Jacobian), one wave per column
//   commit -----k_kg_affine---> commit affine (the Horner coefficients) + compressed
//   (x, value) -k_kg_fr_prep--> Montgomery forms
//   ...         k_kg_fr_part--> L_p(0) per Part, one workgroup per Part, flags[1] on a repeated x
//   ...         k_kg_fr_sum---> sk = sum_p L_p(0), canonical
//   commit -----k_kg_horner---> segment (s, i) of pk_share[i], scaled to its place (Jacobian)
//   segments ---k_kg_affine---> pk_share[i] = the sum of its segments, affine (the key set's
//                               resident form) + compressed
//
// The arithmetic is keygen.h's, which tests/native/hbtc_keygen_hosttest.cpp runs on the CPU.
#include "keygen.h"
#include "hbtc_kernels.h"

namespace hbtc {

namespace {
__device__ __forceinline__ void kg_load_words(uint32_t* w, const uint8_t* base, size_t item, int nwords) {
  const uint4* q = reinterpret_cast<const uint4*>(base + item * (size_t)(nwords * 4));
  for (int i = 0; i < nwords / 4; ++i) {
    const uint4 v = q[i];
    w[4 * i] = v.x;
    w[4 * i + 1] = v.y;
    w[4 * i + 2] = v.z;
    w[4 * i + 3] = v.w;
  }
}
__device__ __forceinline__ void kg_store_words(uint8_t* base, size_t item, const uint32_t* w, int nwords) {
  uint4* q = reinterpret_cast<uint4*>(base + item * (size_t)(nwords * 4));
  for (int i = 0; i < nwords / 4; ++i) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
inline uint32_t kg_blocks(uint64_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }
}  // namespace

// One lane per row0 point: k_g1_decode's rule (decompression + subgroup check); a point that does
// not decode raises flags[0] (its slot holds the zero point g1_decompress leaves).
__global__ void __launch_bounds__(64) k_kg_decode(uint32_t n, const uint8_t* __restrict__ in,
                                                  G1A* __restrict__ out, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[12];
  kg_load_words(w, in, i, 12);
  G1A p;
  const bool ok = g1_decompress(p, w);
  out[i] = p;
  if (!ok) atomicOr(&flags[0], 1u);
}

// One wave per column j: every lane adds its Parts, then a tree of jac_add over the lanes.
__global__ void __launch_bounds__(KG_COL) k_kg_colsum(uint32_t n_parts, uint32_t t1,
                                                      const G1A* __restrict__ dec,
                                                      G1J* __restrict__ col) {
  __shared__ G1J sh[KG_COL];
  const uint32_t j = blockIdx.x, tid = threadIdx.x;
  G1J acc;
  kg_col_lane(acc, dec, n_parts, t1, j, tid);
  sh[tid] = acc;
  __syncthreads();
  for (uint32_t off = KG_COL / 2; off > 0; off >>= 1) {
    kg_tree_step(sh, tid, off);
    __syncthreads();
  }
  if (tid == 0) col[j] = sh[0];
}

// Point i = the sum of in[i + s * stride], s < n_seg, made affine with one inversion per KG_BS
// points: aff[i] (canonical, as k_g1_decode leaves a point) and / or its 48 compressed bytes.
// With a flag raised (the call is not ACCEPTed) the bytes are zeros and aff[i] is the point at
// infinity with st[i] = DECODE_ERR, so nothing downstream computes with it.
__global__ void __launch_bounds__(KG_BS) k_kg_affine(uint32_t n, uint32_t n_seg, uint32_t stride,
                                                     const G1J* __restrict__ in,
                                                     const uint32_t* __restrict__ flags,
                                                     G1A* __restrict__ aff, int32_t* __restrict__ st,
                                                     uint8_t* __restrict__ out_c48) {
  __shared__ Fq C[KG_BS];
  __shared__ Fq S[KG_BS];
  __shared__ Fq INV_TOTAL;
  const uint32_t tid = threadIdx.x, i = blockIdx.x * KG_BS + tid;
  const bool live = i < n;
  G1J p;
  jac_set_inf(p);
  if (live) {
    p = in[i];
#pragma unroll 1
    for (uint32_t s = 1; s < n_seg; ++s) {
      const G1J q = in[(size_t)s * stride + i];
      jac_add(p, p, q);
    }
  }
  KgScan<Fq> sc;
  kg_affine_factor(sc.cp, p);
  sc.sp = sc.cp;
  C[tid] = sc.cp;
  S[tid] = sc.cp;
  __syncthreads();
  for (uint32_t off = 1; off < KG_BS; off <<= 1) {
    KgScanIn<Fq> nb;
    kg_scan_read(nb, tid, off, C, S);
    __syncthreads();
    kg_scan_write(sc, nb, tid, off, C, S);
    __syncthreads();
  }
  if (tid == 0) {
    Fq inv;
    finv_fast(inv, C[KG_BS - 1]);  // the one inversion
    INV_TOTAL = inv;
  }
  __syncthreads();
  Fq zinv, e_excl, incl;
  kg_scan_inverse(zinv, e_excl, incl, tid, C, S, INV_TOTAL);
  if (!live) return;
  const bool closed = flags[0] != 0 || flags[1] != 0;
  G1A a;
  kg_affine_finish(a, p, zinv);
  uint32_t w[12];
  if (closed) {
    fq_zero(a.x);
    fq_zero(a.y);
    a.inf = 1;
    for (int k = 0; k < 12; ++k) w[k] = 0;
  } else {
    g1_compress(w, a);
  }
  if (aff) aff[i] = a;
  if (st) st[i] = closed ? HBTC_DECODE_ERR : HBTC_ACCEPT;
  if (out_c48) kg_store_words(out_c48, i, w, 12);
}

// One lane per stored value: x and the value in Montgomery form.
__global__ void __launch_bounds__(256) k_kg_fr_prep(uint32_t n, const uint32_t* __restrict__ x,
                                                    const Fr* __restrict__ vals, Fr* __restrict__ xm,
                                                    Fr* __restrict__ ym) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  Fr a, b;
  kg_fr_prep(a, b, x[g], vals[g]);
  xm[g] = a;
  ym[g] = b;
}

// One workgroup per Part: L_p(0) through its m = off[p + 1] - off[p] values (any m, any distinct
// x), Montgomery, to part[p].  q / pre / wy: one Fr of workspace per value each.
__global__ void __launch_bounds__(KG_BS) k_kg_fr_part(const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ x,
                                                      const Fr* __restrict__ xm,
                                                      const Fr* __restrict__ ym, Fr* __restrict__ q,
                                                      Fr* __restrict__ pre, Fr* __restrict__ wy,
                                                      Fr* __restrict__ part,
                                                      uint32_t* __restrict__ flags) {
  __shared__ Fr C[KG_BS];
  __shared__ Fr S[KG_BS];
  __shared__ Fr INV_TOTAL;
  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  const uint32_t lo = off[p], m = off[p + 1] - lo;
  KgScan<Fr> sc;
  const bool dup = kg_lane_products(sc.cp, tid, m, x + lo, xm + lo, ym + lo, q + lo, pre + lo, wy + lo);
  if (dup) atomicOr(&flags[1], 1u);
  sc.sp = sc.cp;
  C[tid] = sc.cp;
  S[tid] = sc.cp;
  __syncthreads();
  for (uint32_t o = 1; o < KG_BS; o <<= 1) {
    KgScanIn<Fr> nb;
    kg_scan_read(nb, tid, o, C, S);
    __syncthreads();
    kg_scan_write(sc, nb, tid, o, C, S);
    __syncthreads();
  }
  if (tid == 0) {
    Fr inv;
    fr_inv(inv, C[KG_BS - 1]);  // the one inversion (0 for a Part with a repeated x: flagged)
    INV_TOTAL = inv;
  }
  __syncthreads();
  Fr own_inv, e_excl, incl, sum;
  kg_scan_inverse(own_inv, e_excl, incl, tid, C, S, INV_TOTAL);
  kg_lane_dot(sum, tid, m, e_excl, incl, q + lo, pre + lo, wy + lo);
  __syncthreads();  // every lane has read C and S
  C[tid] = sum;
  __syncthreads();
  for (uint32_t o = KG_BS / 2; o > 0; o >>= 1) {
    kg_fr_tree_step(C, tid, o);
    __syncthreads();
  }
  if (tid == 0) part[p] = C[0];
}

// One workgroup: sk = sum_p part[p], canonical little-endian words; zeros when the call is not
// ACCEPTed.
__global__ void __launch_bounds__(KG_BS) k_kg_fr_sum(uint32_t n_parts, const Fr* __restrict__ part,
                                                     const uint32_t* __restrict__ flags,
                                                     Fr* __restrict__ out) {
  __shared__ Fr C[KG_BS];
  const uint32_t tid = threadIdx.x;
  Fr acc;
  limbs_zero<8>(acc);
  for (uint32_t p = tid; p < n_parts; p += KG_BS) fr_add(acc, acc, part[p]);
  C[tid] = acc;
  __syncthreads();
  for (uint32_t o = KG_BS / 2; o > 0; o >>= 1) {
    kg_fr_tree_step(C, tid, o);
    __syncthreads();
  }
  if (tid == 0) {
    Fr c;
    fr_from_mont(c, C[0]);
    if (flags[0] != 0 || flags[1] != 0) limbs_zero<8>(c);
    out[0] = c;
  }
}

// One lane per (segment s = blockIdx.y, node i): segment s of commit.evaluate(i + 1), scaled to
// its place, to seg[s * n_nodes + i].  A wave holds one segment of 64 nodes, so the coefficient
// address is uniform over the wave.
__global__ void __launch_bounds__(64) k_kg_horner(uint32_t n_nodes, uint32_t t1,
                                                  const G1A* __restrict__ C, G1J* __restrict__ seg) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (i >= n_nodes) return;
  G1J acc;
  kg_eval_segment(acc, C, t1, s, i + 1);
  seg[(size_t)s * n_nodes + i] = acc;
}

hipError_t launch_kg_decode(hipStream_t s, uint32_t n, const uint8_t* in_c48, G1A* out, uint32_t* flags) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_kg_decode, dim3(kg_blocks(n, 64)), dim3(64), 0, s, n, in_c48, out, flags);
  return hipGetLastError();
}

hipError_t launch_kg_colsum(hipStream_t s, uint32_t n_parts, uint32_t t1, const G1A* dec, G1J* col) {
  if (t1 == 0) return hipSuccess;
  hipLaunchKernelGGL(k_kg_colsum, dim3(t1), dim3(KG_COL), 0, s, n_parts, t1, dec, col);
  return hipGetLastError();
}

hipError_t launch_kg_affine(hipStream_t s, uint32_t n, uint32_t n_seg, uint32_t stride, const G1J* in,
                            const uint32_t* flags, G1A* aff, int32_t* st, uint8_t* out_c48) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_kg_affine, dim3(kg_blocks(n, KG_BS)), dim3(KG_BS), 0, s, n, n_seg, stride, in,
                     flags, aff, st, out_c48);
  return hipGetLastError();
}

hipError_t launch_kg_fr(hipStream_t s, uint32_t n_parts, uint32_t n_vals, const uint32_t* off,
                        const uint32_t* x, const uint8_t* vals_le32, Fr* ws, Fr* part,
                        uint32_t* flags, uint8_t* out_sk_le32) {
  Fr *xm = ws, *ym = ws + n_vals, *q = ws + 2 * (size_t)n_vals, *pre = ws + 3 * (size_t)n_vals,
     *wy = ws + 4 * (size_t)n_vals;
  if (n_vals)
    hipLaunchKernelGGL(k_kg_fr_prep, dim3(kg_blocks(n_vals, 256)), dim3(256), 0, s, n_vals, x,
                       reinterpret_cast<const Fr*>(vals_le32), xm, ym);
  hipLaunchKernelGGL(k_kg_fr_part, dim3(n_parts), dim3(KG_BS), 0, s, off, x, xm, ym, q, pre, wy, part, flags);
  hipLaunchKernelGGL(k_kg_fr_sum, dim3(1), dim3(KG_BS), 0, s, n_parts, part, flags,
                     reinterpret_cast<Fr*>(out_sk_le32));
  return hipGetLastError();
}

uint32_t kg_segment_count(uint32_t t1) { return kg_segments(t1); }

hipError_t launch_kg_horner(hipStream_t s, uint32_t n_nodes, uint32_t t1, const G1A* C, G1J* seg) {
  if (n_nodes == 0 || t1 == 0) return hipSuccess;
  hipLaunchKernelGGL(k_kg_horner, dim3(kg_blocks(n_nodes, 64), kg_segments(t1)), dim3(64), 0, s, n_nodes,
                     t1, C, seg);
  return hipGetLastError();
}

}  // namespace hbtc
