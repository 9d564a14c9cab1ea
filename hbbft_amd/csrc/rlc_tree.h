// The tile sums of a DecryptionShare call as a lane-dense tree (kernel: hbtc_rlc.hip k_rlc_tree;
// the same function runs on the CPU in tests/native/hbtc_tree_hosttest.cpp).
//
// rlc_common.h rlc_reduce_sp forms a tile's sums on the tile's own wave: past the first level
// 2 of every 2s lanes merge and the wave still issues every instruction.  Here one workgroup
// takes TREE_G consecutive tiles and, level by level, lists the merges of all of them (both
// sides: S = sum r_i d_i and P = sum r_i pk_i) densely over its threads, so a wave holds 64
// merges until a level has fewer than that, and a wave without merges skips the level.
//
// The merges, their operands, the order of the jac_add / jac_dbl calls and so the TileSums bytes
// are those of rlc_reduce_sp:
//     level 1   (positions 2m, 2m+1)       A = l + r,  B = r
//     level L   (groups of s = 2^(L-1))    B = 2 (B_l + B_r) + A_r,  then  A = A_l + A_r
//
// Nodes travel through global memory, levels are separated by a workgroup barrier.
//   S  in place in the shares' slots (k_rlc_items left S_i = [r_id] d_i, or the identity, in slot
//      i): the group rooted at position g keeps A in slot g and B in slot g + 1 (the level-1 right
//      child, which IS B after level 1 and is dead after it).
//   P  level-1 inputs are rpk[idx[i]] for the lanes of the tile's mask and the identity for the
//      others; A nodes go to TREE_P_SLOTS slots per tile (pair m = positions 2m, 2m + 1 -> slot
//      m): the group rooted at g keeps A in slot g / 2 and, from groups of 4 on, B in slot
//      g / 2 + 1 (a group of 2 has B = its right input, read again from rpk).
// A merge reads and writes only [g, g + 2s) of its own tile and side, so merges of one level
// never touch each other's nodes.
//
// Ragged tiles: a position >= count is the identity and its slot belongs to the next tile: it is
// never read or written.  A group rooted at g >= count is the identity on both sums (jac_add of
// two identities returns the second, so rlc_reduce_sp writes the canonical identity there too);
// the group rooted at g = count - 1 has one share, of weight 0, so its B is the identity as well
// and is not stored.
#pragma once
#include "curve.h"

namespace hbtc {

#ifndef HBTC_TREE_G
#define HBTC_TREE_G 8  // tiles per workgroup (measured at 4, 8 and 16: DESIGN.md §5)
#endif
#ifndef HBTC_TREE_BS
// threads per workgroup: both waves are full through level 3, one through level 4.  Small on
// purpose: a wave without merges waits at the level's barrier with its registers held.
#define HBTC_TREE_BS 128
#endif
constexpr uint32_t TREE_G = HBTC_TREE_G;
constexpr uint32_t TREE_BS = HBTC_TREE_BS;
constexpr uint32_t TREE_P_SLOTS = 32;  // G1J of P-node workspace per tile
constexpr uint32_t TREE_LEVELS = 6;

// TileSums (hbtc_kernels.h) as an array of G1J: the first entry of every member
constexpr uint32_t TS_S = 0, TS_P = 9, TS_SW = 18, TS_PW = 27, TS_SH = 36, TS_SHW = 38, TS_PH = 40,
                   TS_PHW = 42, TS_SQ = 44, TS_SQW = 46, TS_PQ = 48, TS_PQW = 50, TS_G1J = 52;

struct TreeTile {
  uint32_t first, count;  // the tile's items [first, first + count), count <= 64
  uint64_t mask;          // positions that enter the sums (the ballot of k_rlc_items)
};

// merges (both sides) of `g_tiles` tiles at level 1..6
HD uint32_t tree_level_merges(uint32_t g_tiles, uint32_t level) { return (2u * g_tiles * 64u) >> level; }

HD void tree_ld(G1J& r, const G1J* p, bool valid) {
  jac_set_inf(r);
  if (valid) r = *p;
}

// Where the finished group of 2^level positions rooted at g goes in the tile's sums (plain sum;
// the weighted sum goes to the member after next for [0..8], to the next member for the halves
// and quarters), or -1
HD int tree_out_slot(uint32_t level, uint32_t g, bool p_side) {
  if (level == 3) return (int)((p_side ? TS_P : TS_S) + (g >> 3));
  if (level == 4 && (g & 31u) == 0) return (int)((p_side ? TS_PQ : TS_SQ) + (g >> 5));
  if (level == 5) return (int)((p_side ? TS_PH : TS_SH) + (g >> 5));
  if (level == 6) return (int)((p_side ? TS_P : TS_S) + 8);
  return -1;
}

// Merge u of `level` for a group of g_tiles <= TREE_G tiles (u < tree_level_merges(TREE_G, level);
// the S merges first, then the P merges, each tile's in order).  tt: the group's tiles; pnodes:
// the group's P workspace (TREE_P_SLOTS per tile); sums: the group's TileSums as G1J (TS_G1J per
// tile).  t1s, rpk and idx are the call's arrays.
HD void tree_merge(uint32_t level, uint32_t u, uint32_t g_tiles, const TreeTile* tt, G1J* t1s,
                   G1J* pnodes, const G1J* rpk, const uint32_t* idx, G1J* sums) {
  const uint32_t per_log = TREE_LEVELS - level;  // merges per tile and side: 2^per_log
  const uint32_t side_merges = TREE_G << per_log;
  const bool p_side = u >= side_merges;
  if (p_side) u -= side_merges;
  const uint32_t t = u >> per_log;
  if (t >= g_tiles) return;
  const uint32_t g = (u & ((1u << per_log) - 1u)) << level;
  const uint32_t s = 1u << (level - 1);
  const uint32_t first = tt[t].first, count = tt[t].count;
  const uint64_t mask = tt[t].mask;
  G1J* const slots = t1s + first;                  // S nodes
  G1J* const pn = pnodes + t * TREE_P_SLOTS;       // P nodes
  G1J* const out = sums + (size_t)t * TS_G1J;
  const int oslot = tree_out_slot(level, g, p_side);
  const int wslot = oslot < 0 ? -1 : oslot + (level == 3 || level == 6 ? 18 : 2);
  if (g >= count) {  // the identity on both sums; nothing stored
    if (oslot >= 0) {
      G1J z;
      jac_set_inf(z);
      out[oslot] = z;
      out[wslot] = z;
    }
    return;
  }
  if (level == 1) {
    const G1J *pl, *pr;
    bool vl, vr;
    if (p_side) {
      vl = (mask >> g) & 1u;
      vr = (mask >> (g + 1)) & 1u;
      pl = rpk + (vl ? idx[first + g] : 0u);
      pr = rpk + (vr ? idx[first + g + 1] : 0u);
    } else {
      vl = true;
      vr = g + 1 < count;
      pl = slots + g;
      pr = slots + g + 1;
    }
    G1J a, l, r;
    tree_ld(l, pl, vl);
    tree_ld(r, pr, vr);
    jac_add(a, l, r);
    if (p_side) {
      pn[g >> 1] = a;
    } else {
      slots[g] = a;
    }
    return;
  }
  // the operands: A and B of the left group (rooted at g) and of the right one (at g + s)
  const uint32_t gr = g + s;
  const G1J *pal, *pbl, *par, *pbr;
  G1J *wa, *wb;
  bool vbl, var, vbr, vwb;
  if (p_side) {
    pal = pn + (g >> 1);
    par = pn + (gr >> 1);
    var = gr < count;
    if (level == 2) {  // groups of 2: B is the right input
      vbl = (mask >> (g + 1)) & 1u;
      vbr = (mask >> (gr + 1)) & 1u;
      pbl = rpk + (vbl ? idx[first + g + 1] : 0u);
      pbr = rpk + (vbr ? idx[first + gr + 1] : 0u);
    } else {
      vbl = true;
      vbr = var;
      pbl = pal + 1;
      pbr = par + 1;
    }
    wa = pn + (g >> 1);
    wb = wa + 1;
    vwb = true;
  } else {
    pal = slots + g;
    pbl = pal + 1;
    par = slots + gr;
    pbr = par + 1;
    vbl = g + 1 < count;
    var = gr < count;
    vbr = gr + 1 < count;
    wa = slots + g;
    wb = wa + 1;
    vwb = vbl;
  }
  // one merge at a time, so at most three points are live (as rlc_reduce_sp)
  G1J bl;
  tree_ld(bl, pbl, vbl);
  {
    G1J br;
    tree_ld(br, pbr, vbr);
    jac_add(bl, bl, br);
  }
  G1J ar;
  tree_ld(ar, par, var);
  jac_dbl(bl, bl);
  jac_add(bl, bl, ar);
  if (vwb) *wb = bl;
  if (oslot >= 0) out[wslot] = bl;
  G1J al = *pal;
  jac_add(al, al, ar);
  *wa = al;
  if (oslot >= 0) out[oslot] = al;
}

}  // namespace hbtc
