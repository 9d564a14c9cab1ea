// Test-only device harness of the DecryptionShare tile tree (tests/test_gpu_rlc_tree.py): the
// product's k_rlc_tree (this file includes hbtc_rlc.hip, built with the flags of hbtc_rlc.p6.o)
// beside rlc_common.h rlc_reduce_sp on one wave per tile, on the same inputs, so the test can
// compare the TileSums BYTES of the two.  Never linked into the product library.
#include <hip/hip_runtime.h>

#include <vector>

#include "hbtc_rlc.hip"  // every part: rlc_reduce_sp's users and k_rlc_tree

using namespace hbtc;

namespace {

// out[i] = [scal[i]] G (the identity for 0)
__global__ void __launch_bounds__(64) k_td_points(uint32_t n, const uint64_t* __restrict__ scal,
                                                  G1J* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  G1A g;
  fq_set(g.x, G1_GEN_X);
  fq_set(g.y, G1_GEN_Y);
  g.inf = 0;
  G1J r;
  jac_mul_u64(r, g, scal[i]);
  out[i] = r;
}

// the tile's sums as k_rlc_items formed them before the tree kernel: one wave per tile
__global__ void __launch_bounds__(64) k_td_reduce_sp(const Tile* __restrict__ tiles,
                                                     const uint64_t* __restrict__ masks,
                                                     const uint32_t* __restrict__ idx,
                                                     const G1J* __restrict__ t1s,
                                                     const G1J* __restrict__ rpk,
                                                     TileSums* __restrict__ sums) {
  __shared__ G1J red[128];
  const Tile tile = tiles[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  G1J S, P;
  jac_set_inf(S);
  jac_set_inf(P);
  if (lane < tile.count) S = t1s[tile.first + lane];
  if ((masks[blockIdx.x] >> lane) & 1u) P = rpk[idx[tile.first + lane]];
  TileSums* ts = sums + blockIdx.x;
  rlc_reduce_sp(red, red + 64, S, P, lane, ts->S, ts->SW, ts->P, ts->PW, ts->SH, ts->SHW, ts->PH, ts->PHW,
                ts->SQ, ts->SQW, ts->PQ, ts->PQW);
}

struct Dev {
  std::vector<void*> bufs;
  hipError_t err = hipSuccess;
  template <class T>
  T* up(const void* host, size_t bytes) {  // host == nullptr: zero-filled
    if (err != hipSuccess) return nullptr;
    void* p = nullptr;
    err = hipMalloc(&p, bytes ? bytes : 4);
    if (err != hipSuccess) return nullptr;
    bufs.push_back(p);
    if (bytes) err = host ? hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
    return static_cast<T*>(p);
  }
  void down(void* host, const void* dev, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
  }
  void launched() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  int done() {
    for (void* p : bufs) {
      const hipError_t e = hipFree(p);
      if (err == hipSuccess) err = e;
    }
    return (int)err;
  }
};

}  // namespace

extern "C" {

int td_devices() {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  return e == hipSuccess ? n : -(int)e;
}
uint32_t td_group_tiles() { return TREE_G; }
uint32_t td_sums_bytes() { return (uint32_t)sizeof(TileSums); }

// n_tiles consecutive tiles of counts[t] items and masks[t]; the S input of item i is [s_scal[i]] G,
// the sender table entry j is [p_scal[j]] G.  out_ref / out_tree: n_tiles TileSums each, from
// rlc_reduce_sp and from k_rlc_tree.  Returns 0, -1 for a malformed request, or the first failing
// HIP call's status.
int td_tile_sums(uint32_t n_tiles, const uint32_t* counts, const uint64_t* masks, const uint64_t* s_scal,
                 const uint32_t* idx, uint32_t n_pk, const uint64_t* p_scal, uint8_t* out_ref,
                 uint8_t* out_tree) {
  if (n_tiles == 0 || n_pk == 0) return -1;
  std::vector<Tile> tiles(n_tiles);
  uint32_t n_items = 0;
  for (uint32_t t = 0; t < n_tiles; ++t) {
    if (counts[t] == 0 || counts[t] > 64) return -1;
    if (counts[t] < 64 && (masks[t] >> counts[t]) != 0) return -1;
    tiles[t] = Tile{0, n_items, counts[t], 0};
    n_items += counts[t];
  }
  for (uint32_t i = 0; i < n_items; ++i)
    if (idx[i] >= n_pk) return -1;
  Dev d;
  const Tile* d_tiles = d.up<Tile>(tiles.data(), sizeof(Tile) * n_tiles);
  const uint64_t* d_masks = d.up<uint64_t>(masks, 8 * (size_t)n_tiles);
  const uint64_t* d_ss = d.up<uint64_t>(s_scal, 8 * (size_t)n_items);
  const uint64_t* d_ps = d.up<uint64_t>(p_scal, 8 * (size_t)n_pk);
  const uint32_t* d_idx = d.up<uint32_t>(idx, 4 * (size_t)n_items);
  G1J* t1s = d.up<G1J>(nullptr, sizeof(G1J) * (size_t)n_items);
  G1J* rpk = d.up<G1J>(nullptr, sizeof(G1J) * (size_t)n_pk);
  G1J* pnodes = d.up<G1J>(nullptr, sizeof(G1J) * rlc_tree_pnodes(n_tiles));
  TileSums* s_ref = d.up<TileSums>(nullptr, sizeof(TileSums) * (size_t)n_tiles);
  TileSums* s_tree = d.up<TileSums>(nullptr, sizeof(TileSums) * (size_t)n_tiles);
  if (d.err == hipSuccess) {
    hipLaunchKernelGGL(k_td_points, dim3((n_items + 63) / 64), dim3(64), 0, 0, n_items, d_ss, t1s);
    hipLaunchKernelGGL(k_td_points, dim3((n_pk + 63) / 64), dim3(64), 0, 0, n_pk, d_ps, rpk);
    hipLaunchKernelGGL(k_td_reduce_sp, dim3(n_tiles), dim3(64), 0, 0, d_tiles, d_masks, d_idx, t1s, rpk, s_ref);
    d.launched();
  }
  if (d.err == hipSuccess) {  // the tree works in place on t1s: after the reference
    hipLaunchKernelGGL(k_rlc_tree, dim3((n_tiles + TREE_G - 1) / TREE_G), dim3(TREE_BS), 0, 0, n_tiles, d_tiles,
                       d_idx, d_masks, t1s, pnodes, rpk, s_tree);
    d.launched();
  }
  d.down(out_ref, s_ref, sizeof(TileSums) * (size_t)n_tiles);
  d.down(out_tree, s_tree, sizeof(TileSums) * (size_t)n_tiles);
  return d.done();
}

}  // extern "C"
