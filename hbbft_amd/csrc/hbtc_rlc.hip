// Random-linear-combination (RLC) batch verification of DecryptionShares with hierarchical
// fallback and single-error location — the fast path behind hbtc_verify_dec_shares
// (PublicKeyShare::verify_decryption_share, /root/reference/src/threshold_decryption.rs:159,
// called once per share by the reference).
//
// For a group G of shares of ONE ciphertext (u, v, w), H = hash_g1_g2(u, v), and
// E_i = e(d_i, H) / e(pk_i, w) (E_i == 1 iff share i is valid):
//     every share valid  =>  e(sum_G r_i d_i, H) * e(-sum_G r_i pk_i, w) == prod E_i^r_i == 1
// and, for r_i drawn uniformly from a set of 2^k scalars AFTER the shares are fixed (a ChaCha20
// stream under a fresh 256-bit host key per call; k = 128 by default, 64 optional), an invalid
// share makes the equation fail except with probability <= 2^-k per check (every point is in the
// prime-order subgroup: decode checks it, so E_i has order 1 or r).
//
// Scalars per sender.  r_i is a function of (call key, sender id) -- rlc_digits(key, idx[i]), not
// of the item index: a check is over one tile of one ciphertext, and its bound needs only that
// the scalars of the shares INSIDE that tile are independent, uniform, secret and drawn after the
// shares are fixed; which scalars other tiles and other ciphertexts use does not enter it, and
// the call's bound is the union bound over its checks as before.  So R_id = [r_id] pk_id is
// computed once per call for the key set's n_pk senders (k_rlc_rpk) instead of once per share,
// and a share loads its 144-byte point.  Two entries of ONE sender inside one tile would share
// a scalar (valid + D and valid - D would cancel): the duplicate guard of k_rlc_items keeps the
// first such entry in the sums and sends every later one to the exact leaf checks, the tracked
// senders' path.  Copies in different tiles are in different checks and need nothing.
//
// Single-error location.  Next to the plain sum the item pass also forms the position-weighted
// sum (weights p_i distinct in [0, |G|): p_i = bitrev_k(i) for share i of a group of 2^k, which
// the reduction tree forms with one doubling per level, rlc_common.h), so each group yields
//     T = prod E_i^r_i      and      T_w = prod E_i^(p_i r_i).
// If exactly one share b is wrong, T_w == T^(p_b): the search over p = 0..|G|-1 finds it with
// |G|-1 GT multiplications instead of per-share pairings, and the rest of the group is valid.
// With two or more wrong shares, T_w == T^p holds for some p only if prod_i E_i^(r_i (p_i - p))
// == 1 with a nonzero exponent on a wrong share, i.e. with probability <= 2^-k per p (the same
// argument as the plain check), <= |G| 2^-k per located group; such groups are split.
//
// This file holds the per-item pass (k_rlc_decode: decode; k_rlc_items: r_i d_i, left in the
// share's workspace slot with the tile's mask of summed lanes; k_rlc_tree: the tile and sub-tile
// sums of 8 tiles per workgroup, every level's merges dense over the threads, rlc_tree.h)
// and the final decision (k_rlc_finalize); the pairing-product checks of those sums run on
// the cooperative GT arithmetic in hbtc_check.hip:
//     k_chk_plain / k_chk_pair   plain (and weighted) checks of every 64-share tile; a failing
//                   tile with one wrong share is located right there, the others are listed
//     k_chk_split   listed tiles split in halves, quarters, eighths (left child checked, right
//                   child derived), single wrong shares located at every level
//     k_chk_leaves  the exact per-share check for eighths with >= 2 wrong shares
// Work per share in the honest case: decode + r_i d_i (the x-adic joint double-and-add, curve.h
// xadic_mul_uniform) + a load of r_i pk_i from the call's sender table + a share of the tile's
// reduction tree; the pairing work is per group.
#include "rlc_common.h"
#include "rlc_tree.h"

#ifndef HBTC_PART
#define HBTC_PART 0
#endif
#define HBTC_IN_PART(n) (HBTC_PART == 0 || HBTC_PART == (n))

// The item pass as two kernels: the decode half at three waves per SIMD (332 B/lane), the scalar
// half at two (its x-adic table) -- C3 13.6 -> 14.1 M shares/s against the single two-wave kernel
// (profiles/r05/run12/)
#ifndef HBTC_RLC_SPLIT
#define HBTC_RLC_SPLIT 1
#endif
// The tile sums in a kernel of their own (k_rlc_tree, rlc_tree.h) instead of a tree on every
// tile's wave at the end of k_rlc_items (rlc_common.h rlc_reduce_sp; HBTC_RLC_TREE=0 builds that
// form for comparisons).  Needs the split pass: S_i takes the share's [|x|] d slot.
#ifndef HBTC_RLC_TREE
#define HBTC_RLC_TREE 1
#endif
#if HBTC_RLC_TREE && !HBTC_RLC_SPLIT
#error "HBTC_RLC_TREE needs HBTC_RLC_SPLIT (S_i is left in the t1 workspace)"
#endif
#ifndef HBTC_TREE_WAVES
#define HBTC_TREE_WAVES 2  // minimum waves per SIMD of k_rlc_tree's register allocation
#endif
#ifndef HBTC_TREE_PRIO
#define HBTC_TREE_PRIO 0  // wave priority of k_rlc_tree (experiments)
#endif

namespace hbtc {

#if HBTC_IN_PART(6)
// ------------------------------------------------------------------------------ per item
// One wave per tile: decode every share (the subgroup test yields [|x|] d on the way), draw the
// sender's x-adic scalar r_i = d0 + d1 x + d2 mu + d3 mu x (four ChaCha20 digits of key.bits / 4
// bits, mu = -x^2 the eigenvalue of phi: 2^key.bits distinct residues mod r, rlc_common.h),
// compute r_i d_i by one joint double-and-add over the digits' bits (curve.h xadic_mul_uniform),
// and hand r_i d_i and the tile's mask of summed lanes to k_rlc_tree, which loads r_i pk_i from
// the call's sender table and forms the plain and weighted group sums (HBTC_RLC_TREE=0: both
// here, on the tile's own wave).  Items
// that cannot be checked (decode error, unknown sender) get their final status
// here and contribute the identity; a ciphertext whose own H / w failed to decode is resolved
// by k_rlc_finalize.  Needs nothing from the per-ciphertext preparation, so it runs
// concurrently with k_g2_prepare on another stream.
#ifndef HBTC_ITEMS_PRIO
#define HBTC_ITEMS_PRIO 0  // wave priority of the item pass (experiments: 3 = above the check levels)
#endif
#ifndef HBTC_SAC8_LDS
#define HBTC_SAC8_LDS 1  // three of the eight entries in LDS (the reduction's arrays, unused then)
#endif
#ifndef HBTC_ITEMS_WAVES
// minimum waves per SIMD the register allocation must allow (round 5, C3 shares/s: one wave with
// the whole 8-entry table in registers + AGPRs 11.7 M, two waves with the table partly spilled
// 13.4 M, profiles/r05/run1/)
#define HBTC_ITEMS_WAVES 2
#endif
#ifndef HBTC_RLC_DEC_WAVES
#define HBTC_RLC_DEC_WAVES 3
#endif
#if HBTC_RLC_SPLIT
// The decode half (HBTC_RLC_SPLIT): zcash G1 decode with the endomorphism subgroup test, whose
// first half [|x|] d is kept (t1) for the x-adic table; DECODE_ERR into status, everything else
// RLC_PENDING for k_rlc_items.
__global__ void __launch_bounds__(64, HBTC_RLC_DEC_WAVES) k_rlc_decode(
    const Tile* __restrict__ tiles, const uint32_t* __restrict__ idx, const uint8_t* __restrict__ shares,
    const int32_t* __restrict__ pk_status, uint32_t n_pk, G1A* __restrict__ dec, G1J* __restrict__ t1s,
    int32_t* __restrict__ status) {
  const Tile tile = tiles[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  if (lane >= tile.count) return;
  const size_t item = (size_t)tile.first + lane;
  const uint32_t id = idx[item];
  int32_t st = HBTC_RLC_PENDING;
  if (id < n_pk && pk_status[id] == HBTC_ACCEPT) {
    uint32_t w[12];
    rlc_load_words(w, shares, item, 12);
    G1A d;
    if (!g1_decompress<HBTC_FQ_RR != 0>(d, w, false)) {
      st = HBTC_DECODE_ERR;
    } else if (!d.inf) {
      // the subgroup test (curve.h g1_in_subgroup_t1) with its operands parked in the outputs:
      // d and t1 = [|x|] d go to memory as soon as they exist and d is read back for the final
      // comparison, so the second multiplication runs with only t1 live beside its accumulator
      // (332 -> 192 B/lane of scratch at three waves per SIMD)
      dec[item] = d;
#if HBTC_FQ_RR >= 2
      // both chains on the redundant 13 x 30 form (curve.h jacw_*): d goes into it once, t1 comes out
      // to 12 x 32 Montgomery for t1s (a congruent Jacobian representative of the 12 x 32 chain's; the
      // layout and every reader are unchanged) and stays, 13-limb, the second chain's base; the final
      // comparison runs in the same form against the re-read d
      JacW t1, t2;
      {
        AffW q;
        affw_from_aff(q, d);
        jacw_mul_x(t1, q);
      }
      {
        G1J t1o;
        jacw_to_jac(t1o, t1);
        t1s[item] = t1o;
      }
      jacw_mul_x_jac(t2, t1);             // [x^2] d
      __asm__ volatile("" ::: "memory");  // d is re-read, not kept in registers
      const G1A dd = dec[item];
      FqW bx, ny;
      {
        Fq fb;
        FqW beta, x, y;
        fq_set(fb, G1_BETA);
        fw_from_fq(beta, fb);
        fw_from_fq(x, dd.x);
        fw_from_fq(y, dd.y);
        fw_mul(bx, x, beta);
        fw_neg(ny, y);  // phi(d) == -[x^2] d  <=>  (beta x, -y) == [x^2] d
      }
      if (jacw_is_inf(t2) || !jacw_eq_aff(t2, bx, ny)) st = HBTC_DECODE_ERR;
#else
      G1J t1, t2;
      jac_mul_u64(t1, d, BLS_X_ABS);
      t1s[item] = t1;
      jac_mul_u64_jac(t2, t1, BLS_X_ABS);  // [x^2] d
      __asm__ volatile("" ::: "memory");   // d is re-read, not kept in registers
      const G1A dd = dec[item];
      Fq bx, ny, beta;
      fq_set(beta, G1_BETA);
      fq_mul(bx, dd.x, beta);
      fq_neg(ny, dd.y);  // phi(d) == -[x^2] d  <=>  (beta x, -y) == [x^2] d
      if (jac_is_inf(t2) || !jac_eq_aff(t2, bx, ny)) st = HBTC_DECODE_ERR;
#endif
    } else {
      G1J t1;
      jac_set_inf(t1);
      dec[item] = d;
      t1s[item] = t1;
    }
  }
  status[item] = st;
}
#endif

// The call's sender table R_id = [r_id] pk_id (rlc_common.h rlc_sender_point), 64 senders per
// workgroup, on the call's stream ahead of the item pass.  A kernel of its own: as tail
// workgroups of k_rlc_decode it cost that kernel 8 B/lane of scratch (192 -> 200).
__global__ void __launch_bounds__(64) k_rlc_rpk(const G1A* __restrict__ pk,
                                                const int32_t* __restrict__ pk_status,
                                                const PtXY* __restrict__ pk_tab, uint32_t n_pk,
                                                RlcKey key, G1J* __restrict__ rpk) {
  const uint32_t id = blockIdx.x * 64u + threadIdx.x;
  if (id >= n_pk) return;
  G1J r;
  rlc_sender_point(r, id, pk, pk_status, pk_tab, key);
  rpk[id] = r;
}

__global__ void __launch_bounds__(64, HBTC_ITEMS_WAVES) k_rlc_items(
    const Tile* __restrict__ tiles, const uint32_t* __restrict__ idx,
    const uint8_t* __restrict__ shares, const int32_t* __restrict__ pk_status, uint32_t n_pk,
    RlcKey key, Suspects sus, TileSums* __restrict__ sums, G1A* __restrict__ dec,
    int32_t* __restrict__ status, G1J* __restrict__ t1s, const G1J* __restrict__ rpk,
    uint64_t* __restrict__ masks) {
#if HBTC_ITEMS_PRIO > 0
  __builtin_amdgcn_s_setprio(HBTC_ITEMS_PRIO);
#endif
  // the x-adic table's three LDS entries (18 KB: 3 x 24 words x 64 lanes, curve.h
  // xadic_mul_sac8<LDS3>); with HBTC_RLC_TREE=0 also the reduction's two arrays after them: one
  // wave per block, so the table reads are over before the reduction writes
  __shared__ G1J red[128];
  const Tile tile = tiles[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const size_t item = (size_t)tile.first + lane;
  G1J S;
  jac_set_inf(S);
#if !HBTC_RLC_TREE
  G1J P;
  jac_set_inf(P);
#endif
  int32_t st = HBTC_RLC_PENDING;
  uint32_t id = 0;
  bool sum = false;  // this share enters the group sums
#if !HBTC_RLC_SPLIT
  G1A d;
  G1J t1;
#endif
  if (lane < tile.count) {
    id = idx[item];
    if (id >= n_pk) {
      st = HBTC_UNKNOWN_SENDER;
    } else if (pk_status[id] != HBTC_ACCEPT) {
      st = HBTC_DECODE_ERR;
    } else {
#if HBTC_RLC_SPLIT
      const bool dec_ok = status[item] != HBTC_DECODE_ERR;  // k_rlc_decode ran first
#else
      uint32_t w[12];
      rlc_load_words(w, shares, item, 12);
      const bool dec_ok = g1_decompress_t1(d, t1, w);
      if (dec_ok) dec[item] = d;  // for the exact leaf checks and the combine (no second decode)
#endif
      if (!dec_ok) {
        st = HBTC_DECODE_ERR;
      } else if (is_suspect(sus, id)) {
        st = HBTC_RLC_LEAF;  // straight to an exact check, outside the group sums
      } else {
        sum = true;
      }
    }
  }
  // Duplicate guard.  The scalar is keyed by the sender, so two entries of one sender in this
  // tile would share it and a pair valid + D, valid - D would cancel in the sums: every later
  // copy among the entries that enter the sums takes the tracked senders' path (the identity
  // here, an exact check in k_chk_leaves); the first stays.  Wave-uniform: all 64 lanes shuffle.
  {
    const uint32_t mine = sum ? id : 0xffffffffu;
    bool dup = false;
#pragma unroll 1
    for (uint32_t j = 0; j < 63; ++j) {
      const uint32_t other = (uint32_t)__shfl((int)mine, (int)j);
      dup |= j < lane && other == mine;
    }
    if (sum && dup) {
      sum = false;
      st = HBTC_RLC_LEAF;
    }
  }
  // statuses and the leaf list first: nothing of them stays live across the multiplication
  if (lane < tile.count) status[item] = st;
  rlc_list_leaf(sus, st == HBTC_RLC_LEAF, (uint32_t)item, tile.inst, lane);
  if (sum) {
#if HBTC_RLC_SPLIT
    const G1A d = dec[item];
    G1J t1 = t1s[item];  // [|x|] d from the subgroup test: [x] d = -t1, the x-adic table's second entry
#endif
    if (!d.inf) {
      const XDigits xd = rlc_digits(key, id);
      jac_neg(t1, t1);
      Fq beta;
      fq_set(beta, G1_BETA);
#if HBTC_XADIC8
#if HBTC_ITEMS_WAVES >= 2 && HBTC_SAC8_LDS && HBTC_FQ_RR >= 3 && HBTC_RLC_SPLIT && HBTC_RLC_TREE
      // the same multiplication with its Fq products on the redundant 13 x 30 form and the table
      // packed on the same 24 words an entry (curve.h xadic_mul_sac8_w): S is another Jacobian
      // representative of the same point, on the same 12 x 32 Montgomery words
      (void)beta;
      xadic_mul_sac8_w(S, d, t1, xd.d[0], xd.d[1], xd.d[2], xd.d[3], xd.nbits,
                       reinterpret_cast<uint32_t*>(red), lane);
#elif HBTC_ITEMS_WAVES >= 2 && HBTC_SAC8_LDS
      xadic_mul_sac8<Fq, true>(S, d, t1, beta, xd.d[0], xd.d[1], xd.d[2], xd.d[3], xd.nbits,
                               reinterpret_cast<uint32_t*>(red), lane);
#else
      xadic_mul_sac8(S, d, t1, beta, xd.d[0], xd.d[1], xd.d[2], xd.d[3], xd.nbits);
#endif
#else
      G1A xp, pxp;
      xadic_table(xp, pxp, d, t1);
      xadic_mul_uniform(S, d, xp, pxp, beta, xd.d[0], xd.d[1], xd.d[2], xd.d[3], xd.nbits);
#endif
    }
#if !HBTC_RLC_TREE
    P = rpk[id];  // [r_id] pk_id, the identity for a key at infinity
#endif
  }
#if HBTC_RLC_TREE
  // S_i (the identity for a lane outside the sums) over the share's own [|x|] d slot, which is
  // dead now, and the tile's mask: k_rlc_tree forms the sums
  if (lane < tile.count) t1s[item] = S;
  const uint64_t m = __ballot(sum);
  if (lane == 0) masks[blockIdx.x] = m;
#else
  G1J* redA = red;
  G1J* redB = red + 64;
  TileSums* ts = sums + blockIdx.x;
  rlc_reduce_sp(redA, redB, S, P, lane, ts->S, ts->SW, ts->P, ts->PW, ts->SH, ts->SHW, ts->PH,
                ts->PHW, ts->SQ, ts->SQW, ts->PQ, ts->PQW);
#endif
}

#endif  // part 6

#if HBTC_IN_PART(6)
// Every item still pending passed some group check: ACCEPT.  Items of a ciphertext whose own
// H / w failed to decode: INSTANCE_ERR.  With sender tracking on, the REJECTs of every sender
// are counted (k_track_update turns the counts into tracking stamps).
__global__ void __launch_bounds__(64) k_rlc_finalize(const Tile* __restrict__ tiles,
                                                     const int32_t* __restrict__ h_status,
                                                     const int32_t* __restrict__ w_status,
                                                     int32_t* __restrict__ status,
                                                     const uint32_t* __restrict__ idx, uint32_t n_pk,
                                                     uint32_t* __restrict__ rejects) {
  const Tile tile = tiles[blockIdx.x];
  if (threadIdx.x >= tile.count) return;
  const uint32_t i = tile.first + threadIdx.x;
  if (h_status[tile.inst] != HBTC_ACCEPT || w_status[tile.inst] != HBTC_ACCEPT) {
    status[i] = HBTC_INSTANCE_ERR;
  } else {
    const int32_t st = status[i];
    if (st == HBTC_RLC_PENDING) {
      status[i] = HBTC_ACCEPT;
    } else if (st == HBTC_REJECT && rejects) {
      const uint32_t id = idx[i];
      if (id < n_pk) atomicAdd(rejects + id, 1u);
    }
  }
}

// status `from` -> `to` (the pair checks run through the SignatureShare path: a Q that fails to
// decode is the item's own DECODE_ERR there, not an instance error)
__global__ void __launch_bounds__(256) k_status_remap(uint32_t n, int32_t* __restrict__ status,
                                                      int32_t from, int32_t to) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && status[i] == from) status[i] = to;
}

// A sender whose REJECTs in this call reach `thresh` (1/8 of the call's average shares per
// sender: a liar, not a sender hit by a stray corrupted share) is stamped with the call number;
// the counts are cleared for the next call.
__global__ void __launch_bounds__(256) k_track_update(uint32_t n_pk, uint32_t* __restrict__ rejects,
                                                      uint32_t* __restrict__ last_bad, uint32_t now,
                                                      uint32_t thresh) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pk) return;
  const uint32_t r = rejects[i];
  if (r == 0) return;
  if (r >= thresh) last_bad[i] = now;
  rejects[i] = 0;
}
#endif  // part 6

#if HBTC_IN_PART(7) && HBTC_RLC_TREE
// The tile sums of TREE_G consecutive tiles per workgroup (rlc_tree.h): at every level the
// merges of all the group's tiles, both sides, densely over the threads; the nodes go through
// global memory (the S_i slots and pnodes) between barriers.  A thread's merges of one level
// are TREE_BS apart, so whole waves run out of work together and skip the level.  Two waves per
// workgroup: a wave that waits at a barrier holds its registers, and with four waves (16 tiles)
// the waiting ones kept the other lanes' kernels off the SIMDs -- the whole gain.
static_assert(sizeof(TileSums) == TS_G1J * sizeof(G1J) && offsetof(TileSums, P) == TS_P * sizeof(G1J) &&
                  offsetof(TileSums, SW) == TS_SW * sizeof(G1J) && offsetof(TileSums, PW) == TS_PW * sizeof(G1J) &&
                  offsetof(TileSums, SH) == TS_SH * sizeof(G1J) && offsetof(TileSums, SHW) == TS_SHW * sizeof(G1J) &&
                  offsetof(TileSums, PH) == TS_PH * sizeof(G1J) && offsetof(TileSums, PHW) == TS_PHW * sizeof(G1J) &&
                  offsetof(TileSums, SQ) == TS_SQ * sizeof(G1J) && offsetof(TileSums, SQW) == TS_SQW * sizeof(G1J) &&
                  offsetof(TileSums, PQ) == TS_PQ * sizeof(G1J) && offsetof(TileSums, PQW) == TS_PQW * sizeof(G1J),
              "rlc_tree.h addresses TileSums as an array of G1J");
__global__ void __launch_bounds__(TREE_BS, HBTC_TREE_WAVES) k_rlc_tree(
    uint32_t n_tiles, const Tile* __restrict__ tiles, const uint32_t* __restrict__ idx,
    const uint64_t* __restrict__ masks, G1J* t1s, G1J* pnodes, const G1J* __restrict__ rpk,
    TileSums* sums) {
#if HBTC_TREE_PRIO > 0
  __builtin_amdgcn_s_setprio(HBTC_TREE_PRIO);
#endif
  __shared__ TreeTile tt[TREE_G];
  const uint32_t t0 = blockIdx.x * TREE_G;
  const uint32_t g_tiles = n_tiles - t0 < TREE_G ? n_tiles - t0 : TREE_G;
  for (uint32_t t = threadIdx.x; t < g_tiles; t += TREE_BS) {
    const Tile tile = tiles[t0 + t];
    tt[t] = TreeTile{tile.first, tile.count, masks[t0 + t]};
  }
  __syncthreads();
  G1J* const pn = pnodes + (size_t)t0 * TREE_P_SLOTS;
  G1J* const out = reinterpret_cast<G1J*>(sums + t0);
#pragma unroll 1
  for (uint32_t level = 1; level <= TREE_LEVELS; ++level) {
    const uint32_t n = tree_level_merges(TREE_G, level);
#pragma unroll 1
    for (uint32_t u = threadIdx.x; u < n; u += TREE_BS) tree_merge(level, u, g_tiles, tt, t1s, pn, rpk, idx, out);
    __syncthreads();  // the next level reads these nodes (global memory, workgroup scope)
  }
}
hipError_t launch_rlc_tree(hipStream_t s, uint32_t n_tiles, const Tile* tiles, const uint32_t* idx,
                           const uint64_t* masks, G1J* t1s, G1J* pnodes, const G1J* rpk, TileSums* sums) {
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rlc_tree, dim3((n_tiles + TREE_G - 1) / TREE_G), dim3(TREE_BS), 0, s, n_tiles, tiles,
                     idx, masks, t1s, pnodes, rpk, sums);
  return hipGetLastError();
}
#endif  // part 7

// ------------------------------------------------------------------------------ launchers
static inline uint32_t rlc_blocks(uint64_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }

#if HBTC_IN_PART(6)
bool rlc_items_split() { return HBTC_RLC_SPLIT != 0; }
bool rlc_items_tree() { return HBTC_RLC_TREE != 0; }
hipError_t launch_rlc_items(hipStream_t s, uint32_t n_tiles, const Tile* tiles, const uint32_t* idx,
                            const uint8_t* shares, const G1A* pk, const int32_t* pk_status,
                            const PtXY* pk_tab, uint32_t n_pk, RlcKey key, Suspects sus,
                            TileSums* sums, G1A* dec, int32_t* status, G1J* t1s, G1J* rpk,
                            uint64_t* masks, G1J* pnodes, hipEvent_t after_decode) {
  if (n_tiles == 0) return hipSuccess;
  hipError_t e;
  // the sender table: not in the exact mode, where no share enters the sums
  if (!sus.all && n_pk) {
    hipLaunchKernelGGL(k_rlc_rpk, dim3(rlc_blocks(n_pk, 64)), dim3(64), 0, s, pk, pk_status, pk_tab,
                       n_pk, key, rpk);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
#if HBTC_RLC_SPLIT
  hipLaunchKernelGGL(k_rlc_decode, dim3(n_tiles), dim3(64), 0, s, tiles, idx, shares, pk_status, n_pk,
                     dec, t1s, status);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (after_decode && (e = hipEventRecord(after_decode, s)) != hipSuccess) return e;
#endif
  hipLaunchKernelGGL(k_rlc_items, dim3(n_tiles), dim3(64), 0, s, tiles, idx, shares, pk_status, n_pk,
                     key, sus, sums, dec, status, t1s, rpk, masks);
#if HBTC_RLC_TREE
  // the tile sums: not in the exact mode, where no share enters them and no check reads them
  if (!sus.all) {
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_rlc_tree(s, n_tiles, tiles, idx, masks, t1s, pnodes, rpk, sums);
  }
#endif
  return hipGetLastError();
}
hipError_t launch_rlc_finalize(hipStream_t s, uint32_t n_tiles, const Tile* tiles,
                               const int32_t* h_status, const int32_t* w_status, int32_t* status,
                               const uint32_t* idx, uint32_t n_pk, uint32_t* rejects,
                               uint32_t* last_bad, uint32_t now, uint32_t thresh) {
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rlc_finalize, dim3(n_tiles), dim3(64), 0, s, tiles, h_status, w_status,
                     status, idx, n_pk, last_bad ? rejects : nullptr);
  if (last_bad)
    hipLaunchKernelGGL(k_track_update, dim3(rlc_blocks(n_pk, 256)), dim3(256), 0, s, n_pk, rejects,
                       last_bad, now, thresh);
  return hipGetLastError();
}
hipError_t launch_status_remap(hipStream_t s, uint32_t n, int32_t* status, int32_t from, int32_t to) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_status_remap, dim3(rlc_blocks(n, 256)), dim3(256), 0, s, n, status, from, to);
  return hipGetLastError();
}
#endif  // part 6

}  // namespace hbtc
