// Batch verification of signed messages grouped by signer -- the fast path behind
// hbtc_verify_signed_msgs: the non-threshold PublicKey::verify(sig, bytes) that
// DynamicHoneyBadger runs on every signed vote (dynamic_honey_badger/votes.rs:150-155) and every
// signed key-generation message (dynamic_honey_badger.rs:425-440).  The items of a call are signed
// by only a few keys (the validators' and one candidate's), so for signer j with key P_j and
// per-item scalars r_i (rlc_common.h rlc_digits, ChaCha20 under a fresh key per chunk):
//     every item of j valid  =>  e(P_j, sum_{i in j} r_i H_i) == e(G1, sum_{i in j} r_i sigma_i)
// one pair of G2 sums per signer and n_signers + 1 Miller loops instead of n (DESIGN.md §4
// "Signed messages grouped by signer").  It is the dual of k_sig_items_pair (one H, many keys).
// Measured slower than the pair batch at 1,000 signers, so hbtc_verify_signed_msgs
// takes this path only under hbtc_set_exact_below(ctx, 0).
//
//   msgs ----k_hash_cand-------> the first on-curve candidate of hash_g2(msg_i)     [hbtc_hash.hip]
//   sigma ---k_sig_decode_pair-> the decoded sigma_i, psi subgroup test             [hbtc_sig.hip]
//   k_sv_items   per item on a lane pair: H = [h2] cand in registers (never compressed), r H, then
//                r sigma, one after the other; the tile's two sums S = sum r H, T = sum r sigma
//   k_sv_sums    a signer's tile sums -> (S_j, T_j): a tree in passes of fan-in 64, one workgroup
//                per group of 64 nodes, so no workgroup walks a long signer's list
//   k_sv_signers the signers as the items of a pair batch with pre-scaled input (A = P_j, Q = S_j,
//                W = T_j): affine S_j, the 8- and 64-signer sums of T_j; the checks themselves are
//                the pair batch's (k_pb_lines, k_pb_ml, k_plines modes 3 / 4, k_pb_fe)
//   k_sv_finish  the items' statuses from their signer's verdict; the items of failing signers
//                are listed for the exact per-item route
#include "hbtc_kernels.h"
#include "pair.h"
#include "pair_tree.h"
#include "rlc_common.h"

namespace hbtc {

#ifndef HBTC_SV_WAVES
// k_sv_items: minimum waves per SIMD of the register allocation.  One, as k_sig_share: the cofactor
// clearing holds four Jacobian points beside the product's fixed registers (256 VGPRs + 192 AGPRs,
// no scratch; at two waves 904 B/lane of scratch, past the 256 B bound for G2 curve kernels)
#define HBTC_SV_WAVES 1
#endif

namespace {
// [r] P on the pair's lanes by the x-adic two-addition loop of k_pb_wsum_pair: [x] P = psi(P),
// m = -psi^2 = (zeta x, y); the three table points in the caller's LDS columns.  P not infinity.
__device__ __forceinline__ void sv_scale(G2Jp& S, const G2Ap& P, const XDigits& xd, uint32_t* lds) {
  G2Ap xp, pxp;
  g2p_psi(xp.x, xp.y, P);
  xp.inf = 0;
  G2Jp xj;
  jac_from_aff(xj, xp);
  xadic_table(xp, pxp, P, xj);
  Fq zeta;
  fq_set(zeta, G2_ZETA);
  xy_lds_put_aff<Fq2p, 128>(lds, threadIdx.x, 0, P);
  xy_lds_put_aff<Fq2p, 128>(lds, threadIdx.x, 1, xp);
  xy_lds_put_aff<Fq2p, 128>(lds, threadIdx.x, 2, pxp);
  xadic_mul_uniform_lds<Fq2p, 128>(S, lds, threadIdx.x, zeta, xd.d[0], xd.d[1], xd.d[2], xd.d[3], xd.nbits);
}

__device__ __forceinline__ void sv_store_aff(G2A* o, const G2Ap& p) {
  fq2p_store(&o->x, p.x);
  fq2p_store(&o->y, p.y);
  if (!pair_odd()) o->inf = p.inf;
}
}  // namespace

// One workgroup of two waves per tile of at most 64 items of ONE signer, item m of the tile on
// lanes (2m, 2m + 1).  The items are sorted by signer: signer[] and dec[] / status[] (written by
// the decode kernel) are in that order, perm[] gives the item's place in the caller's order,
// which is the order of the hash candidates.  Per item:
//   signer past the key set: UNKNOWN_SENDER; key not loaded: DECODE_ERR; sigma failed to decode:
//   DECODE_ERR (set by the decode kernel); key at infinity, or [h2] cand = O (G2::rand's loop
//   goes on: the host finishes the hash, as in hbtc_sign_shares): RLC_LEAF, the exact route.
//   Every other item stays PENDING and adds r_i H_i to S and r_i sigma_i to T (sigma = O adds
//   nothing to T: the signer's check then fails and the exact route rejects the item).
// The two multiplications run one after the other through the same table columns, accumulator
// and tree (rlc_reduce_g2p): the live state is one table and one accumulator.  leaf_items counts
// the RLC_LEAF items of the call.
__global__ void __launch_bounds__(128, HBTC_SV_WAVES) k_sv_items(
    const Tile* __restrict__ tiles, const uint32_t* __restrict__ signer, const uint32_t* __restrict__ perm,
    const G2A* __restrict__ cand, const G2A* __restrict__ dec, const G1A* __restrict__ pk,
    const int32_t* __restrict__ pk_status, uint32_t n_pk, RlcKey key, SvTileSums* __restrict__ sums,
    int32_t* __restrict__ status, uint32_t* __restrict__ leaf_items) {
  // the table ([entry][word][lane], 36 KB) while a multiplication runs, then the tree's arrays
  // (A 18 KB, B 9 KB behind a 9 KB gap: k_sig_items_pair's layout)
  __shared__ uint32_t lds[72 * 128];
  uint32_t* ldsB = lds + 36 * 128 + 36 * 64;
  const Tile tile = tiles[blockIdx.x];
  const uint32_t m = threadIdx.x >> 1;
  const bool even = (threadIdx.x & 1u) == 0;
  const size_t item = (size_t)tile.first + m;
  bool pend = false;  // pair-uniform, as every branch below
  int32_t st = HBTC_RLC_PENDING;
  if (m < tile.count) {
    const uint32_t id = signer[item];
    if (id >= n_pk) {
      st = HBTC_UNKNOWN_SENDER;
    } else if (pk_status[id] != HBTC_ACCEPT) {
      st = HBTC_DECODE_ERR;
    } else if (status[item] == HBTC_DECODE_ERR) {  // the decode kernel ran first
      st = HBTC_DECODE_ERR;
    } else if (pk[id].inf) {
      st = HBTC_RLC_LEAF;
    } else {
      pend = true;
    }
  }
  XDigits xd;
  xd.d[0] = xd.d[1] = xd.d[2] = xd.d[3] = 0;
  xd.nbits = 0;
  if (pend) xd = rlc_digits(key, item);
  SvTileSums* ts = sums + blockIdx.x;
#pragma unroll 1
  for (int ph = 0; ph < 2; ++ph) {
    G2Jp S;
    jac_set_inf(S);
    if (pend) {
      G2Ap P;
      if (ph == 0) {
        G2Ap cd;
        g2p_load_aff(cd, cand + perm[item]);
        G2Jp q;
        g2p_clear_cofactor(q, cd);
        jac_to_aff(P, q);  // P.inf: [h2] cand = O
        if (P.inf) {
          pend = false;
          st = HBTC_RLC_LEAF;
        }
      } else {
        g2p_load_aff(P, dec + item);
      }
      if (!P.inf) sv_scale(S, P, xd, lds);
    }
    __syncthreads();  // every lane's table reads are over before the tree's arrays are written
    g2p_lds_put(lds, m, S);
    __syncthreads();
    if (threadIdx.x < 64) {
      if (ph == 0)
        rlc_reduce_g2p(lds, ldsB, threadIdx.x, ts->S, ts->SW);
      else
        rlc_reduce_g2p(lds, ldsB, threadIdx.x, ts->T, ts->TW);
    }
    __syncthreads();  // the tree's reads are over before the next table is written
  }
  if (m < tile.count && even) {
    status[item] = st;
    if (st == HBTC_RLC_LEAF) atomicAdd(leaf_items, 1u);
  }
}

// One pass of the signers' trees: group g sums the `count` consecutive nodes from `first` of ONE
// signer (a Tile of nodes) into node g of the next level, S and T one after the other.  Input
// node k of S at inS[k * stride] (the tile sums: stride = sizeof(SvTileSums) / sizeof(G2J) from
// S[8]; later levels: 1).
__global__ void __launch_bounds__(128) k_sv_sums(const Tile* __restrict__ groups, const G2J* __restrict__ inS,
                                                 const G2J* __restrict__ inT, uint32_t stride,
                                                 G2J* __restrict__ outS, G2J* __restrict__ outT) {
  __shared__ uint32_t lds[36 * 128];
  const Tile grp = groups[blockIdx.x];
  const uint32_t m = threadIdx.x >> 1;
#pragma unroll 1
  for (int ph = 0; ph < 2; ++ph) {
    G2Jp x;
    jac_set_inf(x);
    if (m < grp.count) g2p_load_jac(x, (ph ? inT : inS) + ((size_t)grp.first + m) * stride);
    g2p_lds_put(lds, m, x);
    __syncthreads();
    if (threadIdx.x < 64) g2p_tree_sum(lds, threadIdx.x, (ph ? outT : outS) + blockIdx.x);
    __syncthreads();
  }
}

// The signers as the items of a pair batch whose input is already scaled: slot s holds signer
// slot_signer[s] (SV_NONE: empty) whose sums are node slot_node[s] of nodeS / nodeT.  A slot with
// a loaded, finite key becomes PENDING with rA = P_j and Qdec = S_j (affine; S_j = O: the pair is
// unused, rA = O); every other slot is ACCEPT, which the checks pass over.  The 8- and 64-slot
// sums of T_j go to sums[tile].S (rlc_reduce_g2p, as k_pb_wsum_pair's): nothing is multiplied
// again.
__global__ void __launch_bounds__(128) k_sv_signers(uint32_t n_slots, const uint32_t* __restrict__ slot_signer,
                                                    const uint32_t* __restrict__ slot_node,
                                                    const G2J* __restrict__ nodeS, const G2J* __restrict__ nodeT,
                                                    uint32_t stride, const G1A* __restrict__ pk,
                                                    const int32_t* __restrict__ pk_status, G1A* __restrict__ rA,
                                                    G2A* __restrict__ Qdec, int32_t* __restrict__ sst,
                                                    SigTileSums* __restrict__ sums) {
  __shared__ uint32_t lds[36 * 128 + 2 * 36 * 64];
  uint32_t* ldsB = lds + 36 * 128 + 36 * 64;
  const uint32_t m = threadIdx.x >> 1;
  const uint32_t slot = blockIdx.x * 64u + m;
  const bool even = (threadIdx.x & 1u) == 0;
  G2Jp T;
  jac_set_inf(T);
  if (slot < n_slots) {  // pair-uniform
    const uint32_t j = slot_signer[slot];
    const bool use = j != SV_NONE && pk_status[j] == HBTC_ACCEPT && !pk[j].inf;
    G2Ap Q;
    fzero(Q.x);
    fzero(Q.y);
    Q.inf = 1;
    if (use) {
      const size_t node = (size_t)slot_node[slot] * stride;
      G2Jp S;
      g2p_load_jac(S, nodeS + node);
      g2p_load_jac(T, nodeT + node);
      jac_to_aff(Q, S);
    }
    sv_store_aff(Qdec + slot, Q);
    if (even) {
      G1A a;
      if (use && !Q.inf) {
        a = pk[j];
      } else {
        fq_zero(a.x);
        fq_zero(a.y);
        a.inf = 1;
      }
      rA[slot] = a;
      sst[slot] = use ? HBTC_RLC_PENDING : HBTC_ACCEPT;
    }
  }
  g2p_lds_put(lds, m, T);
  __syncthreads();
  if (threadIdx.x < 64) {
    SigTileSums* ts = sums + blockIdx.x;
    rlc_reduce_g2p(lds, ldsB, threadIdx.x, ts->S, ts->SW);
  }
}

// Final statuses of the chunk's items: a PENDING item of a signer that passed its check is
// ACCEPT; the PENDING items of the signers flagged in sbad (null: none) and the RLC_LEAF items
// of the item pass go on the list for the exact per-item route.
__global__ void __launch_bounds__(64) k_sv_finish(uint32_t n, const uint32_t* __restrict__ signer,
                                                  const uint32_t* __restrict__ sbad, int32_t* __restrict__ status,
                                                  uint32_t* __restrict__ count, uint32_t* __restrict__ list) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  int32_t st = status[i];
  if (st == HBTC_RLC_PENDING) {
    st = (sbad && sbad[signer[i]]) ? HBTC_RLC_LEAF : HBTC_ACCEPT;
    status[i] = st;
  }
  if (st == HBTC_RLC_LEAF && list) list[atomicAdd(count, 1u)] = i;
}

// The listed items, gathered for the exact route: the signer's decoded key and its status, the
// hash candidate, the signature bytes.
__global__ void __launch_bounds__(64) k_sv_gather(uint32_t n, const uint32_t* __restrict__ list,
                                                  const uint32_t* __restrict__ signer,
                                                  const uint32_t* __restrict__ perm, const G2A* __restrict__ cand,
                                                  const uint8_t* __restrict__ sig, const G1A* __restrict__ pk,
                                                  const int32_t* __restrict__ pk_status, uint32_t n_pk,
                                                  G1A* __restrict__ ga, int32_t* __restrict__ gast,
                                                  G2A* __restrict__ gcand, uint8_t* __restrict__ gsig) {
  const uint32_t g = blockIdx.x * 64u + threadIdx.x;
  if (g >= n) return;
  const size_t i = list[g];
  const uint32_t id = signer[i];
  if (id < n_pk) {
    ga[g] = pk[id];
    gast[g] = pk_status[id];
  } else {  // not listed by any caller; kept in bounds
    G1A a;
    fq_zero(a.x);
    fq_zero(a.y);
    a.inf = 1;
    ga[g] = a;
    gast[g] = HBTC_DECODE_ERR;
  }
  gcand[g] = cand[perm[i]];
  const uint4* s = reinterpret_cast<const uint4*>(sig + 96 * i);
  uint4* d = reinterpret_cast<uint4*>(gsig + (size_t)96 * g);
  for (int k = 0; k < 6; ++k) d[k] = s[k];
}

// The key set's keys as compressed bytes, for the composed pair-batch route (which decodes its G1
// arguments itself): a loaded key's encoding, 48 zero bytes (no compression flag: a decode error)
// for a key that failed to load.
__global__ void __launch_bounds__(64) k_sv_pk_c48(uint32_t n, const G1A* __restrict__ pk,
                                                  const int32_t* __restrict__ pk_status,
                                                  uint32_t* __restrict__ out_w) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  uint32_t w[12];
  for (int j = 0; j < 12; ++j) w[j] = 0;
  if (pk_status[i] == HBTC_ACCEPT) {
    const G1A a = pk[i];
    g1_compress(w, a);
  }
  uint4* o = reinterpret_cast<uint4*>(out_w + 12 * (size_t)i);
  for (int k = 0; k < 3; ++k) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// gc48[g] = the compressed key of listed item g's signer
__global__ void __launch_bounds__(64) k_sv_gather_c48(uint32_t n, const uint32_t* __restrict__ list,
                                                      const uint32_t* __restrict__ signer,
                                                      const uint8_t* __restrict__ pk_c48, uint32_t n_pk,
                                                      uint8_t* __restrict__ gc48) {
  const uint32_t g = blockIdx.x * 64u + threadIdx.x;
  if (g >= n) return;
  const uint32_t id = signer[list[g]];
  uint4* d = reinterpret_cast<uint4*>(gc48 + (size_t)48 * g);
  if (id < n_pk) {
    const uint4* s = reinterpret_cast<const uint4*>(pk_c48 + (size_t)48 * id);
    for (int k = 0; k < 3; ++k) d[k] = s[k];
  } else {
    for (int k = 0; k < 3; ++k) d[k] = make_uint4(0, 0, 0, 0);
  }
}

hipError_t launch_sv_pk_c48(hipStream_t s, uint32_t n, const G1A* pk, const int32_t* pk_status, uint8_t* out_c48) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sv_pk_c48, dim3((n + 63) / 64), dim3(64), 0, s, n, pk, pk_status,
                     reinterpret_cast<uint32_t*>(out_c48));
  return hipGetLastError();
}
hipError_t launch_sv_gather_c48(hipStream_t s, uint32_t n, const uint32_t* list, const uint32_t* signer,
                                const uint8_t* pk_c48, uint32_t n_pk, uint8_t* gc48) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sv_gather_c48, dim3((n + 63) / 64), dim3(64), 0, s, n, list, signer, pk_c48, n_pk, gc48);
  return hipGetLastError();
}

hipError_t launch_sv_items(hipStream_t s, uint32_t n_tiles, const Tile* tiles, const uint32_t* signer,
                           const uint32_t* perm, const G2A* cand, const G2A* dec, const G1A* pk,
                           const int32_t* pk_status, uint32_t n_pk, RlcKey key, SvTileSums* sums,
                           int32_t* status, uint32_t* leaf_items) {
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sv_items, dim3(n_tiles), dim3(128), 0, s, tiles, signer, perm, cand, dec, pk, pk_status,
                     n_pk, key, sums, status, leaf_items);
  return hipGetLastError();
}

hipError_t launch_sv_sums(hipStream_t s, uint32_t n_groups, const Tile* groups, const G2J* inS, const G2J* inT,
                          uint32_t stride, G2J* outS, G2J* outT) {
  if (n_groups == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sv_sums, dim3(n_groups), dim3(128), 0, s, groups, inS, inT, stride, outS, outT);
  return hipGetLastError();
}

hipError_t launch_sv_signers(hipStream_t s, uint32_t n_slots, const uint32_t* slot_signer,
                             const uint32_t* slot_node, const G2J* nodeS, const G2J* nodeT, uint32_t stride,
                             const G1A* pk, const int32_t* pk_status, G1A* rA, G2A* Qdec, int32_t* sst,
                             SigTileSums* sums) {
  if (n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sv_signers, dim3((n_slots + 63) / 64), dim3(128), 0, s, n_slots, slot_signer, slot_node,
                     nodeS, nodeT, stride, pk, pk_status, rA, Qdec, sst, sums);
  return hipGetLastError();
}

hipError_t launch_sv_finish(hipStream_t s, uint32_t n, const uint32_t* signer, const uint32_t* sbad,
                            int32_t* status, uint32_t* count, uint32_t* list) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sv_finish, dim3((n + 63) / 64), dim3(64), 0, s, n, signer, sbad, status, count, list);
  return hipGetLastError();
}

hipError_t launch_sv_gather(hipStream_t s, uint32_t n, const uint32_t* list, const uint32_t* signer,
                            const uint32_t* perm, const G2A* cand, const uint8_t* sig, const G1A* pk,
                            const int32_t* pk_status, uint32_t n_pk, G1A* ga, int32_t* gast, G2A* gcand,
                            uint8_t* gsig) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sv_gather, dim3((n + 63) / 64), dim3(64), 0, s, n, list, signer, perm, cand, sig, pk,
                     pk_status, n_pk, ga, gast, gcand, gsig);
  return hipGetLastError();
}

}  // namespace hbtc
