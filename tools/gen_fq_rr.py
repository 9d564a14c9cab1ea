#!/usr/bin/env python3
"""Generate hbbft_amd/csrc/fq_rr.h: the Fq Montgomery product and squaring on 13 limbs of 30 bits
(R' = 2^390), each ONE inline-asm block for gfx950 plus the same schedule as plain 64-bit C++ for
the host build.

Why 30-bit limbs: a column of the 12 x 32 product (fq_fips_asm.h) needs a carry word, one
v_addc_co_u32 per v_mad_u64_u32, and both are 4-cycle instructions.  With limbs below 2^30 a
product is below 2^60 and up to 16 of them add into the MAD's 64-bit addend with no carry-out, so
the v_addc goes; a column ends in one 30-bit split (v_and, v_alignbit, v_lshrrev: full rate).

Form: product scanning, column k = sum a_i b_(k-i) + sum q_i p_(k-i) + carry, for k < 13 the
Montgomery digit q_k = (low 30 bits * n') mod 2^30 and its term q_k p_0 (the low 30 bits are then
0), for k >= 13 the result limb r_(k-13) = low 30 bits; carry = column >> 30 (up to 35 bits: it is
the next column's first 64-bit addend).  The accumulator alternates between two register pairs
(HBTC_FIPS_ACC*, the pins of fq_fips_asm.h), so the split writes the next column's pair directly.

Column overflow: a middle column holds 13 a b + 13 q p terms, more than 2^64.  schedule()
adds every term's exact maximum (operand limbs <= 2^30 - 1, q <= 2^30 - 1, p's actual limbs, the
carry-in bound) and, only where the next term would pass 2^64 - 1, emits a split at bit 32: the
accumulator's high word moves to h and is zeroed (two v_mov), and the next column adds 4 h (weight
2^32 = 4 * 2^30) as one more MAD.  The simulator (run) raises on any MAD carry-out.

Bounds: for inputs a, b < 16p the result is (a b + q p) / 2^390 < p (256 p / 2^390 + 1) < 1.5p
(p < 2^381), every limb below 2^30: a chain of products and squarings needs no subtraction.  For
any limbs <= 2^30 - 1 (values up to 2^390 - 1) the result is still congruent and below 2^390 + p;
its top limb may then pass 2^30.

Squaring: sum_i a_i^2 + sum_(i<j) a_i (2 a_j), the doubled limbs d_j = 2 a_j < 2^31 formed outside
the block: 91 + 169 MADs against the product's 169 + 169.

Operand bounds are a parameter, per limb (schedule(square, la, lb)): the default, every limb
<= 2^30 - 1, gives mont_mul / mont_sqr; the weakly normalised operands of the redundant form (W_LIMBS
below: limbs 0..11 <= 2^30 + 2, the top limb bounded by the value) give mont_mul_w / mont_sqr_w, whose
splits stand elsewhere.  The subtraction constants of that form (sub_const) are emitted here too.

Usage: tools/gen_fq_rr.py > hbbft_amd/csrc/fq_rr.h ; tools/gen_fq_rr.py --selftest-rr ;
tools/gen_fq_rr.py --selftest-w
"""
import random
import sys

P_MOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
N, W = 13, 30
M = (1 << W) - 1
RBITS = N * W                                   # R' = 2^390
NP = (-pow(P_MOD, -1, 1 << W)) % (1 << W)       # -p^-1 mod 2^30
P_L = [(P_MOD >> (W * i)) & M for i in range(N)]
K_IN = (1 << (2 * RBITS)) * pow(1 << 384, -1, P_MOD) % P_MOD   # R'^2 / R: 12x32 Montgomery -> 13x30
K_OUT = (1 << 384) % P_MOD                                     # R: 13x30 -> 12x32 Montgomery
U64 = (1 << 64) - 1


def limbs(v):
    return [(v >> (W * i)) & M for i in range(N)]


# ---- the redundant form (field.h FqW): sums and differences are taken limb by limb with no carry,
# so limbs pass 2^30 - 1 and the value passes p by a tracked multiple.  One weak normalisation
# l_i = (l_i & M) + (l_(i-1) >> 30) of limbs below 2^32 leaves limbs <= M + W_SLACK (the top limb
# keeps its high bits and is bounded by the value alone).  The relaxed blocks (mont_mul_w,
# mont_sqr_w) take such operands with values up to W_VMAX p; their result has limbs <= M again and
# is below (A B / 630 + 1) p for operands <= A p, B p (2^390 / p = 630.07).
W_SLACK = 3
W_VMAX = 64
W_LIMBS = [M + W_SLACK] * (N - 1) + [(W_VMAX * P_MOD) >> (W * (N - 1))]
ONE = (1 << RBITS) % P_MOD                                     # the Montgomery one, R' mod p
# beta of the G1 endomorphism phi(x, y) = (beta x, y) (tools/gen_constants.py G1_BETA), for the table
# of the x-adic multiplication on this form (curve.h xadic_mul_sac8_w)
BETA = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe
assert pow(BETA, 3, P_MOD) == 1 and BETA != 1


def sub_const(b, k):
    """k p spelled with b units of 2^30 borrowed from every limb above into the limb below: every
    limb but the top is at least b (2^30 - 1), so a + sub_const - s has no borrow for a subtrahend
    whose limbs the constant dominates (tools/rr_bounds.py checks each use limb by limb)."""
    assert k * P_MOD < 1 << RBITS
    l = limbs(k * P_MOD)
    c = [l[0] + (b << W)] + [l[i] + (b << W) - b for i in range(1, N - 1)] + [l[N - 1] - b]
    assert all(0 <= x < 1 << 32 for x in c) and sum(x << (W * i) for i, x in enumerate(c)) == k * P_MOD
    return c


# the constants the point formulas of curve.h use: (units borrowed, multiple of p), one per bound
# class of subtrahend (strict limbs and a small value; twice a strict or normalised value, ...)
SUB_CONSTS = [(1, 4), (2, 4), (2, 8), (2, 10), (2, 14)]


def schedule(square, la=None, lb=None):
    """The instruction list in symbolic form, with the overflow splits the bounds require.
    la, lb: the operands' per-limb maxima (13 each; default every limb 2^30 - 1; a squaring takes la).
    Ops: ("mad", x, y) acc += x y; ("mad0", x, y) acc = x y; ("madh",) acc += 4 h;
    ("split32",) h = acc.hi, acc.hi = 0; ("q", k) q_k = (acc.lo n') & M; ("out", j) r_j = acc.lo & M;
    ("carry",) the other pair = acc >> 30 and becomes acc; ("top",) r_12 = acc >> 30."""
    la = la or [M] * N
    lb = la if square else (lb or [M] * N)
    lim = {}
    for i in range(N):
        lim["a%d" % i], lim["b%d" % i], lim["q%d" % i] = la[i], lb[i], M
        lim["d%d" % i] = 2 * la[i]
        assert lim["d%d" % i] < 1 << 32, "a doubled limb of the squaring passes 32 bits"
        lim["p%d" % i] = P_L[i]
    ops, info = [], {"splits": [], "max": 0}
    bound, hb, h_live = 0, 0, False   # accumulator bound, bound of h, h pending for this column
    for k in range(2 * N - 1):
        lo_i, hi_i = (0, k) if k < N else (k - N + 1, N - 1)
        terms = []
        if square:
            for i in range(lo_i, hi_i + 1):
                j = k - i
                if i < j:
                    terms.append(("a%d" % i, "d%d" % j))
                elif i == j:
                    terms.append(("a%d" % i, "a%d" % i))
        else:
            terms += [("a%d" % i, "b%d" % (k - i)) for i in range(lo_i, hi_i + 1)]
        terms += [("q%d" % i, "p%d" % (k - i)) for i in range(lo_i, (k - 1 if k < N else N - 1) + 1)]
        split_here = False

        def add(op, tb):
            nonlocal bound, hb, split_here
            if bound + tb > U64:
                assert not split_here, "two splits in column %d" % k
                assert not h_live, "h still pending in column %d" % k
                ops.append(("split32",))
                info["splits"].append(k)
                hb, bound, split_here = bound >> 32, (1 << 32) - 1, True
            assert bound + tb <= U64
            bound += tb
            info["max"] = max(info["max"], bound)
            ops.append(op)

        if h_live:          # the previous column's split: its high word at weight 2^32 = 4 * 2^30
            add(("madh",), 4 * hb)
            h_live = False
        for n, (x, y) in enumerate(terms):
            first = k == 0 and n == 0
            add(("mad0" if first else "mad", x, y), lim[x] * lim[y])
        if k < N:
            ops.append(("q", k))
            add(("mad", "q%d" % k, "p0"), M * P_L[0])
        else:
            ops.append(("out", k - N))
        h_live = split_here
        if k < 2 * N - 2:
            ops.append(("carry",))
            bound >>= W
        else:
            assert not h_live
            ops.append(("top",))
            assert bound >> W < 1 << 32
    return ops, info


def run(ops, a, b=None):
    """Execute a schedule on Python integers: the register semantics of the asm rendering (64-bit
    accumulator pair, 32-bit h / q / r).  A MAD whose sum passes 2^64 - 1 is an error."""
    square = b is None
    reg = {}
    for i in range(N):
        reg["a%d" % i] = a[i]
        reg["p%d" % i] = P_L[i]
        if square:
            reg["d%d" % i] = (a[i] << 1) & 0xFFFFFFFF
            assert a[i] < 1 << 31
        else:
            reg["b%d" % i] = b[i]
    acc, h, r = 0, None, [0] * N

    def mad(x, y, z):
        s = x * y + z
        if s > U64:
            raise OverflowError("v_mad_u64_u32 carry-out")
        return s

    for op in ops:
        if op[0] == "mad":
            acc = mad(reg[op[1]], reg[op[2]], acc)
        elif op[0] == "mad0":
            acc = mad(reg[op[1]], reg[op[2]], 0)
        elif op[0] == "madh":
            acc = mad(h, 4, acc)
            h = None
        elif op[0] == "split32":
            assert h is None
            h, acc = acc >> 32, acc & 0xFFFFFFFF
        elif op[0] == "q":
            reg["q%d" % op[1]] = (((acc & 0xFFFFFFFF) * NP) & 0xFFFFFFFF) & M
        elif op[0] == "out":
            r[op[1]] = acc & M
        elif op[0] == "carry":
            acc = (((acc >> W) & 0xFFFFFFFF) | ((acc >> 62) << 32))   # v_alignbit, v_lshrrev
        elif op[0] == "top":
            r[N - 1] = (acc >> W) & 0xFFFFFFFF
            assert acc >> W < 1 << 32
        else:
            raise ValueError(op)
    return r


# ------------------------------------------------------------------------------------ rendering
def asm_lines(ops, square):
    """Operands: r0..r12 %0..%12, q0..q12 %13..%25, h %26, a0..a12 %27..%39, then b0..b12 (product)
    or d1..d12 (squaring), then p0..p12, n', the 30-bit mask (SGPRs)."""
    names = {}
    n = 0
    for pre, cnt, start in (("r", N, 0), ("q", N, 0), ("h", 1, 0), ("a", N, 0)):
        for i in range(start, cnt):
            names[pre + (str(i) if pre != "h" else "")] = "%%%d" % n
            n += 1
    if square:
        for i in range(1, N):
            names["d%d" % i] = "%%%d" % n
            n += 1
    else:
        for i in range(N):
            names["b%d" % i] = "%%%d" % n
            n += 1
    for i in range(N):
        names["p%d" % i] = "%%%d" % n
        n += 1
    names["np"] = "%%%d" % n
    names["mask"] = "%%%d" % (n + 1)
    reg = lambda i: 'v" HBTC_XS(HBTC_FIPS_ACC%d) "' % i
    pair = lambda p: 'v[" HBTC_XS(HBTC_FIPS_ACC%d) ":" HBTC_XS(HBTC_FIPS_ACC%d) "]' % (2 * p, 2 * p + 1)
    out, p = [], 0
    for op in ops:
        acc, lo, hi = pair(p), reg(2 * p), reg(2 * p + 1)
        if op[0] == "mad":
            out.append("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (acc, names[op[1]], names[op[2]], acc))
        elif op[0] == "mad0":
            out.append("v_mad_u64_u32 %s, vcc, %s, %s, 0" % (acc, names[op[1]], names[op[2]]))
        elif op[0] == "madh":
            out.append("v_mad_u64_u32 %s, vcc, %s, 4, %s" % (acc, names["h"], acc))
        elif op[0] == "split32":
            out.append("v_mov_b32 %s, %s" % (names["h"], hi))
            out.append("v_mov_b32 %s, 0" % hi)
        elif op[0] == "q":
            q = names["q%d" % op[1]]
            out.append("v_mul_lo_u32 %s, %s, %s" % (q, lo, names["np"]))
            out.append("v_and_b32 %s, %s, %s" % (q, names["mask"], q))
        elif op[0] == "out":
            out.append("v_and_b32 %s, %s, %s" % (names["r%d" % op[1]], names["mask"], lo))
        elif op[0] == "carry":
            out.append("v_alignbit_b32 %s, %s, %s, 30" % (reg(2 * (1 - p)), hi, lo))
            out.append("v_lshrrev_b32 %s, 30, %s" % (reg(2 * (1 - p) + 1), hi))
            p = 1 - p
        elif op[0] == "top":
            out.append("v_alignbit_b32 %s, %s, %s, 30" % (names["r%d" % (N - 1)], hi, lo))
    return out


def asm_block(name, square, la=None, lb=None):
    ops, _ = schedule(square, la, lb)
    text = "\n".join('      "%s\\n\\t"' % l for l in asm_lines(ops, square))
    outs = ", ".join('"=&v"(r[%d])' % i for i in range(N)) + ",\n        " + \
        ", ".join('"=&v"(q[%d])' % i for i in range(N)) + ', "=&v"(h)'
    ins = ", ".join('"v"(a[%d])' % i for i in range(N)) + ",\n        "
    if square:
        ins += ", ".join('"v"(d[%d])' % i for i in range(1, N))
    else:
        ins += ", ".join('"v"(b[%d])' % i for i in range(N))
    ins += ",\n        " + ", ".join('"s"(RR_P[%d])' % i for i in range(N)) + ', "s"(RR_NP), "s"(RR_MASK)'
    clob = ", ".join('"v" HBTC_XS(HBTC_FIPS_ACC%d)' % n for n in range(4)) + ', "vcc"'
    args = "uint32_t* r, const uint32_t* a" + ("" if square else ", const uint32_t* b")
    prep = ""
    if square:
        prep = """  uint32_t d[13];
#pragma unroll
  for (int j = 1; j < 13; ++j) d[j] = a[j] << 1;
"""
    return """__device__ __forceinline__ void %s(%s) {
  uint32_t q[13], h;
%s  asm volatile(
%s
      : %s
      : %s
      : %s);
}
""" % (name, args, prep, text, outs, ins, clob)


def cxx_block(name, square, la=None, lb=None):
    """The same schedule as straight-line C++ on one 64-bit accumulator.  HBTC_RR_MAD checks the
    no-carry-out claim when HBTC_RR_ASSERT is defined (host tests)."""
    ops, _ = schedule(square, la, lb)
    v = lambda s: "%s[%s]" % (s[0], s[1:])
    body = []
    for op in ops:
        if op[0] == "mad":
            body.append("HBTC_RR_MAD(acc, %s, %s);" % (v(op[1]), v(op[2])))
        elif op[0] == "mad0":
            body.append("acc = (uint64_t)%s * %s;" % (v(op[1]), v(op[2])))
        elif op[0] == "madh":
            body.append("HBTC_RR_MAD(acc, h, 4u);")
        elif op[0] == "split32":
            body.append("h = (uint32_t)(acc >> 32); acc &= 0xffffffffull;")
        elif op[0] == "q":
            body.append("q[%d] = ((uint32_t)acc * RR_NP) & RR_MASK;" % op[1])
        elif op[0] == "out":
            body.append("t[%d] = (uint32_t)acc & RR_MASK;" % op[1])
        elif op[0] == "carry":
            body.append("acc >>= 30;")
        elif op[0] == "top":
            body.append("t[12] = (uint32_t)(acc >> 30);")
    args = "uint32_t* r, const uint32_t* a" + ("" if square else ", const uint32_t* b")
    prep = "  const uint32_t* p = RR_P;\n  uint32_t q[13], t[13], h = 0;\n  uint64_t acc;\n"
    if square:
        prep += "  uint32_t d[13];\n  for (int j = 0; j < 13; ++j) d[j] = a[j] << 1;\n"
    return "HBTC_RR_HD void %s(%s) {\n%s  %s\n  for (int j = 0; j < 13; ++j) r[j] = t[j];\n  (void)h;\n}\n" % (
        name, args, prep, "\n  ".join(body))


def arr(name, vals):
    return "HBTC_RR_CONST uint32_t %s[13] = {%s};" % (name, ", ".join("0x%08xu" % x for x in vals))


def main():
    _, im = schedule(False)
    _, isq = schedule(True)
    print("""// GENERATED by tools/gen_fq_rr.py -- do not edit.
// The Fq Montgomery product and squaring on 13 limbs of 30 bits, R' = 2^390 (see the generator's
// docstring): product scanning with NO carry word -- the terms of a column add into the 64-bit
// addend of v_mad_u64_u32 -- and one 30-bit split per column.  Inputs: limbs <= 2^30 - 1; for
// values < 16p the result is < 1.5p with limbs < 2^30.  Overflow splits (bit 32, carried as 4 h
// into the next column) in columns %s (product) and %s (squaring).
// rr::mont_mul_cxx / mont_sqr_cxx are the same schedule in plain 64-bit C++ (host build, and the
// reference of the device tests); rr::mont_mul_asm / mont_sqr_asm are one inline-asm block each,
// the accumulator pairs on the HBTC_FIPS_ACC* registers of fq_fips_asm.h.
#pragma once
#include <cstdint>
#if defined(__HIPCC__) || defined(__HIP__)
#define HBTC_RR_HD __host__ __device__ __forceinline__
#else
#define HBTC_RR_HD static inline
#endif
#define HBTC_RR_CONST static constexpr
#if defined(HBTC_RR_ASSERT) && !defined(__HIP_DEVICE_COMPILE__)
#include <cstdio>
#include <cstdlib>
#define HBTC_RR_MAD(acc, x, y)                                                          \\
  do {                                                                                  \\
    if (__builtin_add_overflow((acc), (uint64_t)(x) * (y), &(acc))) {                   \\
      std::fprintf(stderr, "fq_rr: MAD carry-out at %%s:%%d\\n", __FILE__, __LINE__);       \\
      std::abort();                                                                     \\
    }                                                                                   \\
  } while (0)
#else
#define HBTC_RR_MAD(acc, x, y) ((acc) += (uint64_t)(x) * (y))
#endif
namespace hbtc {
namespace rr {
""" % (im["splits"], isq["splits"]))
    print(arr("RR_P", P_L) + "  // p")
    print("HBTC_RR_CONST uint32_t RR_NP = 0x%08xu;  // -p^-1 mod 2^30" % NP)
    print("HBTC_RR_CONST uint32_t RR_MASK = 0x%08xu;" % M)
    print(arr("RR_K_IN", limbs(K_IN)) + "   // 2^780 / 2^384 mod p: a R -> a R'")
    print(arr("RR_K_OUT", limbs(K_OUT)) + "  // 2^384 mod p: a R' -> a R")
    print()
    print(cxx_block("mont_mul_cxx", False))
    print(cxx_block("mont_sqr_cxx", True))
    print("""#if defined(__HIP_DEVICE_COMPILE__)
#ifndef HBTC_FIPS_ACC0
#define HBTC_FIPS_ACC0 2
#define HBTC_FIPS_ACC1 3
#define HBTC_FIPS_ACC2 4
#define HBTC_FIPS_ACC3 5
#endif
#ifndef HBTC_XS
#define HBTC_S(x) #x
#define HBTC_XS(x) HBTC_S(x)
#endif
""")
    print(asm_block("mont_mul_asm", False))
    print(asm_block("mont_sqr_asm", True))
    _, wm = schedule(False, W_LIMBS, W_LIMBS)
    _, wsq = schedule(True, W_LIMBS)
    print("""#endif

// ---- the relaxed-bound blocks of the redundant form (field.h FqW): operands weakly normalised,
// limbs 0..11 <= 2^30 - 1 + %d and the top limb <= 0x%x (values up to %d p); the result has limbs
// <= 2^30 - 1 and is below (A B / 630 + 1) p for operands <= A p and B p.  Overflow splits in
// columns %s (product) and %s (squaring).
HBTC_RR_CONST uint32_t RR_W_SLACK = %du;
HBTC_RR_CONST uint32_t RR_W_TOP = 0x%08xu;""" % (W_SLACK, W_LIMBS[N - 1], W_VMAX, wm["splits"], wsq["splits"],
                                                   W_SLACK, W_LIMBS[N - 1]))
    print(arr("RR_ONE", limbs(ONE)) + "  // 2^390 mod p: the Montgomery one")
    print(arr("RR_BETA", limbs(BETA * ONE % P_MOD)) + "  // beta 2^390 mod p (bls_constants.h G1_BETA on this form)")
    for b, k in SUB_CONSTS:
        print(arr("RR_SUB_%d_%d" % (b, k), sub_const(b, k)) +
              "  // %d p with %d borrowed per limb: a + this - s for limbs of s <= these" % (k, b))
    print()
    print(cxx_block("mont_mul_w_cxx", False, W_LIMBS, W_LIMBS))
    print(cxx_block("mont_sqr_w_cxx", True, W_LIMBS))
    print("#if defined(__HIP_DEVICE_COMPILE__)")
    print(asm_block("mont_mul_w_asm", False, W_LIMBS, W_LIMBS))
    print(asm_block("mont_sqr_w_asm", True, W_LIMBS))
    print("""#endif
}  // namespace rr
}  // namespace hbtc""")


# ------------------------------------------------------------------------------------- selftest
def selftest_rr(trials=300):
    """Product and squaring on the simulator against Python integers: no MAD carry-out, the
    result congruent to a b / 2^390; for operands < 16p also < 1.5p with every limb < 2^30."""
    rng = random.Random(13)
    Ri = pow(1 << RBITS, -1, P_MOD)
    edge = [0, 1, P_MOD - 1, P_MOD, 2 * P_MOD - 1, 16 * P_MOD - 1, (1 << RBITS) - 1]
    pairs = [(x, y) for x in edge for y in edge]
    pairs += [(rng.randrange(16 * P_MOD), rng.randrange(16 * P_MOD)) for _ in range(trials)]
    for square in (False, True):
        ops, info = schedule(square)
        assert info["max"] <= U64
        for a, b in pairs:
            if square:
                b = a
            r = run(ops, limbs(a), None if square else limbs(b))
            val = sum(x << (W * i) for i, x in enumerate(r))
            assert val % P_MOD == a * b * Ri % P_MOD, (square, hex(a), hex(b))
            assert val < (1 << RBITS) + P_MOD
            if a < 16 * P_MOD and b < 16 * P_MOD:
                assert 2 * val < 3 * P_MOD and all(x <= M for x in r), (square, hex(a), hex(b))
        # the asm rendering is the schedule op for op (one line each; split and q two, carry two)
        n_asm = len(asm_lines(ops, square))
        want = sum({"split32": 2, "q": 2, "carry": 2}.get(op[0], 1) for op in ops)
        assert n_asm == want
        mads = sum(op[0] in ("mad", "mad0", "madh") for op in ops)
        print("selftest_rr %s ok: %d MADs (%d for overflow splits in columns %s), %d instructions, "
              "largest column bound 2^64 - %d" % ("squaring" if square else "product", mads,
                                                  len(info["splits"]), info["splits"], n_asm,
                                                  U64 + 1 - info["max"]))
    # conversions: a R -> a R' -> a R
    for _ in range(50):
        x = rng.randrange(P_MOD)
        xr = x * (1 << 384) % P_MOD + P_MOD * rng.randrange(2)
        ops, _ = schedule(False)
        y = sum(v << (W * i) for i, v in enumerate(run(ops, limbs(xr), limbs(K_IN))))
        assert y % P_MOD == x * (1 << RBITS) % P_MOD and 2 * y < 3 * P_MOD
        z = sum(v << (W * i) for i, v in enumerate(run(ops, limbs(y), limbs(K_OUT))))
        assert z % P_MOD == x * (1 << 384) % P_MOD and z < 2 * P_MOD
    print("selftest_rr conversions ok")


def selftest_w(trials=300):
    """The relaxed-bound blocks on the simulator: operands spelled with limbs up to W_LIMBS (not
    canonical: the value is what the limbs spell), no MAD carry-out, the result congruent to
    a b / 2^390, its limbs 0..11 <= 2^30 - 1 and its value below a b / 2^390 + p."""
    rng = random.Random(14)
    Ri = pow(1 << RBITS, -1, P_MOD)
    top = sum(x << (W * i) for i, x in enumerate(W_LIMBS))
    edge = [limbs(v) for v in [0, 1, P_MOD - 1, P_MOD] + [k * P_MOD - 1 for k in range(2, W_VMAX + 1)]]
    edge.append(list(W_LIMBS))                                  # every limb at its declared maximum
    edge.append([M + W_SLACK] * (N - 1) + [0])
    rnd = lambda: [rng.randrange(W_LIMBS[i] + 1) for i in range(N)]
    pairs = [(x, y) for x in edge for y in edge] + [(rnd(), rnd()) for _ in range(trials)]
    for square in (False, True):
        ops, info = schedule(square, W_LIMBS, W_LIMBS)
        assert info["max"] <= U64
        for a, b in pairs:
            if square:
                b = a
            assert all(x <= w for x, w in zip(a, W_LIMBS)) and all(x <= w for x, w in zip(b, W_LIMBS))
            va = sum(x << (W * i) for i, x in enumerate(a))
            vb = sum(x << (W * i) for i, x in enumerate(b))
            assert va <= top and vb <= top
            r = run(ops, a, None if square else b)
            val = sum(x << (W * i) for i, x in enumerate(r))
            assert val % P_MOD == va * vb * Ri % P_MOD, (square, a, b)
            assert all(x <= M for x in r[:N - 1]) and val < (va * vb >> RBITS) + P_MOD + 1
        mads = sum(op[0] in ("mad", "mad0", "madh") for op in ops)
        print("selftest_w %s ok: %d MADs, splits in columns %s, %d instructions, largest column bound "
              "2^64 - %d" % ("squaring" if square else "product", mads, info["splits"],
                             len(asm_lines(ops, square)), U64 + 1 - info["max"]))
    for b, k in SUB_CONSTS:
        c = sub_const(b, k)
        assert min(c[:N - 1]) >= b * M and c[N - 1] > 0
    print("selftest_w constants ok")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--selftest-rr":
        selftest_rr()
    elif len(sys.argv) > 1 and sys.argv[1] == "--selftest-w":
        selftest_w()
    elif len(sys.argv) == 1:
        main()
    else:
        sys.exit("usage: gen_fq_rr.py [--selftest-rr | --selftest-w]")
