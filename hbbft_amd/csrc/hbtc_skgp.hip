// SyncKeyGen::new's Part and the Acks of verified Parts on gfx950 (hbtc_skg_part / hbtc_skg_acks):
// the stages in front of the encryption's, device-resident like them:
//
//   bcoef ----k_skgp_commit--> commit[k] = bcoef[k] G1 (comb table), compressed
//   bcoef ----k_skgp_rows----> the Poly frames of rows 1 .. N, straight into the pad's message buffer
//   rows -----k_skgp_vals----> the FieldWrap frames of row_a(1 .. N), likewise
//   r, key set -k_enc_g1_rcpt-> [hbtc_enc.hip] then k_enc_pad, k_hash_cand, k_enc_w unchanged
//
// The arithmetic is skgp.h's, which tests/native/hbtc_skgp_hosttest.cpp runs on the CPU.
#include "skgp.h"
#include "hbtc_kernels.h"

namespace hbtc {

namespace {
inline uint32_t skgp_blocks(uint64_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }
__device__ __forceinline__ void skgp_load_fr(Fr& k, const uint8_t* base, size_t item) {
  const uint4* q = reinterpret_cast<const uint4*>(base + item * 32);
  const uint4 a = q[0], b = q[1];
  k.v[0] = a.x;
  k.v[1] = a.y;
  k.v[2] = a.z;
  k.v[3] = a.w;
  k.v[4] = b.x;
  k.v[5] = b.y;
  k.v[6] = b.z;
  k.v[7] = b.w;
}
__device__ __forceinline__ void skgp_store_c48(uint32_t* base, size_t item, const uint32_t* w) {
  uint4* q = reinterpret_cast<uint4*>(base + item * 12);
  for (int i = 0; i < 3; ++i) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
}  // namespace

// One lane per pair of coefficients: both comb multiplications, one shared inversion.
__global__ void __launch_bounds__(64) k_skgp_commit(uint32_t n, const uint8_t* __restrict__ bcoef_le32,
                                                    const EncPt* __restrict__ tab,
                                                    uint32_t* __restrict__ out_c48) {
  const uint32_t l = blockIdx.x * 64 + threadIdx.x;
  const uint32_t i0 = 2 * l, i1 = i0 + 1;
  if (i0 >= n) return;
  const bool have1 = i1 < n;
  Fr k0, k1;
  skgp_load_fr(k0, bcoef_le32, i0);
  skgp_load_fr(k1, bcoef_le32, have1 ? i1 : i0);
  uint32_t w0[12], w1[12];
  skgp_commit_pair(w0, w1, tab, k0, k1, have1);
  skgp_store_c48(out_c48, i0, w0);
  if (have1) skgp_store_c48(out_c48, i1, w1);
}

// One lane per (row, coefficient): Horner over the packed triangle, the FieldWrap into the row's frame.
__global__ void __launch_bounds__(256) k_skgp_rows(uint32_t n_lanes, const Fr* __restrict__ bm, uint32_t t1,
                                                   uint32_t* __restrict__ msgs) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_lanes) return;
  skgp_rows_lane(idx, bm, t1, msgs);
}

// One lane per (row, node).  A workgroup handles 256 nodes of ONE row, so the coefficient address
// is uniform over the wave and each coefficient is one load for all its lanes (as k_fr_poly_eval).
__global__ void __launch_bounds__(256) k_skgp_vals(uint32_t n_nodes, uint32_t blocks_per_row,
                                                   const Fr* __restrict__ rows_m, uint32_t n_coeff,
                                                   uint32_t* __restrict__ msgs) {
  const uint32_t a = blockIdx.x / blocks_per_row;
  const uint32_t i = (blockIdx.x % blocks_per_row) * 256 + threadIdx.x;
  if (i >= n_nodes) return;
  skgp_vals_lane(a, i, n_nodes, rows_m, n_coeff, msgs);
}

hipError_t launch_skgp_commit(hipStream_t s, uint32_t n, const uint8_t* bcoef_le32, const EncPt* tab,
                              uint8_t* out_c48) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_skgp_commit, dim3(skgp_blocks(((uint64_t)n + 1) / 2, 64)), dim3(64), 0, s, n, bcoef_le32,
                     tab, reinterpret_cast<uint32_t*>(out_c48));
  return hipGetLastError();
}

hipError_t launch_skgp_rows(hipStream_t s, uint32_t n_rows, uint32_t t1, const Fr* bm, uint8_t* msgs) {
  const uint64_t lanes = (uint64_t)n_rows * t1;
  if (lanes == 0) return hipSuccess;
  hipLaunchKernelGGL(k_skgp_rows, dim3(skgp_blocks(lanes, 256)), dim3(256), 0, s, (uint32_t)lanes, bm, t1,
                     reinterpret_cast<uint32_t*>(msgs));
  return hipGetLastError();
}

hipError_t launch_skgp_vals(hipStream_t s, uint32_t n_rows, uint32_t n_nodes, uint32_t n_coeff,
                            const Fr* rows_m, uint8_t* msgs) {
  if (n_rows == 0 || n_nodes == 0) return hipSuccess;
  const uint32_t bpr = skgp_blocks(n_nodes, 256);
  hipLaunchKernelGGL(k_skgp_vals, dim3(n_rows * bpr), dim3(256), 0, s, n_nodes, bpr, rows_m, n_coeff,
                     reinterpret_cast<uint32_t*>(msgs));
  return hipGetLastError();
}

}  // namespace hbtc
