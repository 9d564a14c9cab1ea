"""Shared case tables and the Python-integer reference for the device-arithmetic tests
(tests/test_devarith_host.py on the host fallback, tests/test_gpu_devarith.py on gfx950).

Everything here works on RAW limbs: a value is the integer its twelve 32-bit limbs spell, i.e.
the Montgomery representative itself (R = 2^384), anywhere in the lazy range [0, 2p).  The
reference restates field.h on Python integers:
    mont(T)  = (T + ((-T p^-1) mod 2^384) p) / 2^384          (exact, no final subtraction)
    redc(T)  = mont(T), then minus 4p, then minus 2p, where they fit
    add / sub / neg / canon as field.h defines them on [0, 2p)
so the Fq and accumulator outputs are compared as exact integers.  Fq2, curve and GT results are
compared as canonical residues against oracle/bls12_381.py.

The harness entry points (tests/native) share one calling shape per family, so the same runner
serves the host library and every device variant."""
import ctypes
import functools
import random

from oracle import bls12_381 as B

P = B.P
R = 1 << 384
MASK = R - 1
NP = (-pow(P, -1, R)) % R
RINV = pow(R, -1, P)
TWO_P = 2 * P
M = R % P                    # Montgomery one
R3 = pow(2, 3 * 384, P)      # bls_constants.h FQ_R3
K24 = 24 * P * P             # field.h FQ_ACC_K24


# ----------------------------------------------------------------------------- reference
def mont(t):
    return (t + ((t * NP) & MASK) * P) >> 384


def mmul(a, b):
    return mont(a * b)


def add(a, b):
    s = a + b
    return s - TWO_P if s >= TWO_P else s


def sub(a, b):
    d = a - b
    return d if d >= 0 else d + TWO_P


def neg(a):
    return sub(0, a)


def canon(a):
    return a - P if a >= P else a


def redc(t):
    x = mont(t)
    for m in (4 * P, TWO_P):
        if x >= m:
            x -= m
    return x


def to_m(v, lazy=False):
    """canonical integer -> raw Montgomery limbs value (plus p when lazy)"""
    return v * R % P + (P if lazy else 0)


def from_m(raw):
    return raw * RINV % P


def _pow_plan(e, w=4):
    """field.h pow_plan: the sliding-window schedule (first table index, [(nsq, idx or None)])."""
    def bit(i):
        return (e >> i) & 1

    def window(top):
        low = max(0, top - (w - 1))
        while not bit(low):
            low += 1
        v = 0
        for b in range(top, low - 1, -1):
            v = 2 * v + bit(b)
        return v, low

    i = e.bit_length() - 1
    v, low = window(i)
    first = (v - 1) // 2
    i = low - 1
    steps, nsq = [], 0
    while i >= 0:
        if not bit(i):
            nsq += 1
            i -= 1
            continue
        v, low = window(i)
        nsq += i - low + 1
        steps.append((nsq, (v - 1) // 2))
        nsq = 0
        i = low - 1
    if nsq:
        steps.append((nsq, None))
    return first, steps


_SQRT_PLAN = _pow_plan((P - 3) // 4)


def pow_window(a):
    """field.h fq_pow_window(a, POW_SQRT_PLAN) as the same chain of Montgomery products."""
    first, steps = _SQRT_PLAN
    tab = [a]
    a2 = mmul(a, a)
    for _ in range(7):
        tab.append(mmul(tab[-1], a2))
    acc = tab[first]
    for nsq, idx in steps:
        for _ in range(nsq):
            acc = mmul(acc, acc)
        if idx is not None:
            acc = mmul(acc, tab[idx])
    return acc


def is_zero(a):
    return canon(a) == 0


def fq_eq(a, b):
    return is_zero(sub(a, b))


def from_mont_op(a):
    return canon(mmul(a, 1))


# ----------------------------------------------------------------------------- operand set E
def _limbs(ws):
    return sum(w << (32 * i) for i, w in enumerate(ws))


def operand_set():
    e = [0, 1, 2, 3, P - 2, P - 1, P, P + 1, TWO_P - 2, TWO_P - 1, (P - 1) // 2, (P + 1) // 2,
         M, M + P, P - M, TWO_P - M]
    for k in range(1, 12):
        e += [1 << (32 * k), (1 << (32 * k)) - 1]
    e.append(1 << 381)
    top = (TWO_P - 1) >> 352
    low = (1 << 352) - 1
    v = (top << 352) | low
    e.append(v if v < TWO_P else ((top - 1) << 352) | low)   # limbs 0..10 all ones
    even = _limbs([0xffffffff if i % 2 == 0 else 0 for i in range(12)])
    odd = _limbs([0xffffffff if i % 2 == 1 else 0 for i in range(11)] + [0x0fffffff])
    e += [even, odd]
    rng = random.Random(0xE)
    e += [rng.randrange(P) for _ in range(5)] + [rng.randrange(P, TWO_P) for _ in range(3)]
    assert all(0 <= x < TWO_P for x in e) and len(set(e)) == len(e)
    return e


E = operand_set()
E_RANDOM = E[-8:]            # the seeded random members (mutation evidence: "random cases alone")
# a 12-value subset for the quadratic tables
E12 = [0, 1, P - 1, P, TWO_P - 1, M, M + P, P - M, (1 << 352) - 1, E[-9], E[-1], E[-8]]
assert all(x in E for x in E12)

# ----------------------------------------------------------------------------- Fq table
(OP_MUL, OP_SQR, OP_MUL_OL, OP_ADD, OP_SUB, OP_DBL, OP_NEG, OP_CANON, OP_IS_ZERO, OP_EQ,
 OP_FROM_MONT, OP_LEX, OP_INV, OP_SQRT, OP_MUL2) = range(15)
FQ_OP_NAMES = ["mul", "sqr", "mul_ol", "add", "sub", "dbl", "neg", "canon", "is_zero", "eq",
               "from_mont", "is_lex_largest", "inv_binary", "sqrt", "mul2"]


def fq_ref(op, a, b, c, d):
    """(out, flag) of one item: the exact integers field.h defines."""
    if op in (OP_MUL, OP_MUL_OL):
        return mmul(a, b), 0
    if op == OP_SQR:
        return mmul(a, a), 0
    if op == OP_ADD:
        return add(a, b), 0
    if op == OP_SUB:
        return sub(a, b), 0
    if op == OP_DBL:
        return add(a, a), 0
    if op == OP_NEG:
        return neg(a), 0
    if op == OP_CANON:
        return canon(a), 0
    if op == OP_IS_ZERO:
        return 0, int(is_zero(a))
    if op == OP_EQ:
        return 0, int(fq_eq(a, b))
    if op == OP_FROM_MONT:
        return from_mont_op(a), 0
    if op == OP_LEX:
        return 0, int(from_mont_op(a) > (P - 1) // 2)
    if op == OP_INV:
        u = canon(a)
        x = pow(u, -1, P) if u else 0
        return mmul(x, R3), 0
    if op == OP_SQRT:
        t = pow_window(a)
        y = mmul(t, a)
        return y, int(fq_eq(mmul(y, y), a))
    if op == OP_MUL2:
        return mont(a * b + c * d), 0
    raise ValueError(op)


def fq_table():
    """[(op, a, b, c, d)], grouped by op (a wave then runs one operation on most lanes, and the
    inversions share waves, so their wave-uniform loop ends at different iterations per lane)."""
    t = []
    for op in (OP_MUL, OP_MUL_OL, OP_ADD, OP_SUB, OP_EQ):
        t += [(op, a, b, 0, 0) for a in E for b in E]
    for op in (OP_SQR, OP_DBL, OP_NEG, OP_CANON, OP_IS_ZERO, OP_FROM_MONT, OP_LEX, OP_SQRT):
        t += [(op, a, 0, 0, 0) for a in E]
    inv = list(E) + [(M << k) % P for k in (1, 5, 31, 32, 33, 63, 200, 380)]
    inv += [1 << k for k in (31, 33, 63, 95, 380)] + [(1 << 380) + 1, 3 << 377]
    t += [(OP_INV, a, 0, 0, 0) for a in inv]
    rng = random.Random(0x2E)
    top = TWO_P - 1
    m2 = [(top, top, top, top), (top, top, 0, 0), (0, 0, top, top), (0, top, top, 0),
          (P, P, P, P), (1 << 192, 1 << 192, 0, 0), (1 << 192, 1 << 192, 1 << 192, 1 << 192)]
    for i, a in enumerate(E12):
        for j, b in enumerate(E12):
            m2.append((a, b, E12[(j + 5) % 12], E12[(i + 7) % 12]))
    m2 += [tuple(rng.randrange(TWO_P) for _ in range(4)) for _ in range(16)]
    t += [(OP_MUL2,) + q for q in m2]
    return t


# ----------------------------------------------------------------------------- accumulator table
ACC_MAC, ACC_MAC2, ACC_MACSUB, ACC_SUBSUB, ACC_KARA = range(5)
ACC_MODE_NAMES = ["mac/redc", "mac2/redc2", "macsub", "subsub", "kara"]


def acc_ref(mode, terms):
    """(out0, out1): terms are (a, b) pairs, for ACC_KARA (a0, a1, b0, b1).  Asserts the documented
    preconditions: every accumulator ends in [0, 48 p^2)."""
    if mode == ACC_KARA:
        x = K24 + sum(a0 * b0 - a1 * b1 for a0, a1, b0, b1 in terms)
        y = sum(a0 * b1 + a1 * b0 for a0, a1, b0, b1 in terms)
    else:
        s = sum(a * b for a, b in terms)
        x, y = {ACC_MAC: (s, 0), ACC_MAC2: (0, s), ACC_MACSUB: (s, K24 - s),
                ACC_SUBSUB: (K24 - s, K24 - s)}[mode]
    assert 0 <= x < 2 * K24 and 0 <= y < 2 * K24, "accumulator precondition"
    return redc(x), redc(y)


def acc_table():
    """[(mode, terms, tag)]"""
    top = TWO_P - 1
    rng = random.Random(0xACC)
    t = []
    pairs = [(a, b) for a in E for b in E]
    for mode, nts in ((ACC_MAC, (1, 2, 6, 12)), (ACC_MAC2, (1, 2, 6, 12)), (ACC_MACSUB, (1, 2, 6)),
                      (ACC_SUBSUB, (1, 2, 6))):
        nmax = nts[-1]
        for nt in nts:
            t.append((mode, [(top, top)] * nt, "max x%d" % nt))
        t.append((mode, [(0, 0)] * nmax, "zero"))
        t.append((mode, [(1 << 192, 1 << 192)], "2^192 squared"))
        t.append((mode, [(P, P)] * nmax, "p p"))
        for s in range(0, len(pairs), len(pairs) // 16):
            t.append((mode, [pairs[(s + 53 * i) % len(pairs)] for i in range(nmax)], "E %d" % s))
        for i in range(8):
            t.append((mode, [(rng.randrange(TWO_P), rng.randrange(TWO_P))
                             for _ in range(rng.randint(1, nmax))], "random %d" % i))
    t.append((ACC_KARA, [(top, 0, top, 0)] * 6, "kara X top"))
    t.append((ACC_KARA, [(0, top, 0, top)] * 6, "kara X bottom"))
    t.append((ACC_KARA, [(top, top, top, top)] * 6, "kara Y top"))
    t.append((ACC_KARA, [(0, 0, 0, 0)] * 6, "kara zero"))
    for s in range(8):
        t.append((ACC_KARA, [tuple(E[(s + 7 * i + 13 * j) % len(E)] for j in range(4))
                             for i in range(6)], "kara E %d" % s))
    for i in range(8):
        t.append((ACC_KARA, [tuple(rng.randrange(TWO_P) for _ in range(4))
                             for _ in range(rng.randint(1, 6))], "kara random %d" % i))
    return t


# ----------------------------------------------------------------------------- Fq2 (lane pairs)
(F2_MUL, F2_SQR, F2_INV, F2_CONJ, F2_NEG, F2_IS_ZERO, F2_EQ, F2_MUL_FQ, F2_ONE) = range(9)
F2_OP_NAMES = ["fmul", "fsqr", "finv_fast", "fconj", "fneg", "fis_zero", "feq", "fmul_by_fq", "fone"]


def fq2_elements():
    """24 raw Fq2 elements (pairs of raw limbs values) from the 12-value subset."""
    x = E12[9]
    els = [(0, 0), (M, 0), (0, M), (P, P), (x, x), (x, P - x), (x, TWO_P - x), (P - x, x),
           (TWO_P - 1, TWO_P - 1), (TWO_P - 1, 0), (0, TWO_P - 1), (P, 0), (M + P, P), (1, P - 1)]
    rng = random.Random(0xF2)
    while len(els) < 24:
        c = (rng.choice(E12), rng.choice(E12))
        if c not in els:
            els.append(c)
    return els


def f2v(a):
    return (from_m(a[0]), from_m(a[1]))


def fq2_ref(op, a, b, c):
    """(value as canonical (c0, c1), flag)"""
    va, vb = f2v(a), f2v(b)
    if op == F2_MUL:
        return B.f2_mul(va, vb), 0
    if op == F2_SQR:
        return B.f2_sqr(va), 0
    if op == F2_INV:
        return (B.f2_inv(va) if va != (0, 0) else (0, 0)), 0
    if op == F2_CONJ:
        return B.f2_conj(va), 0
    if op == F2_NEG:
        return B.f2_neg(va), 0
    if op == F2_IS_ZERO:
        return (0, 0), int(va == (0, 0))
    if op == F2_EQ:
        return (0, 0), int(va == vb)
    if op == F2_MUL_FQ:
        return B.f2_scale(va, from_m(c)), 0
    if op == F2_ONE:
        return (1, 0), 0
    raise ValueError(op)


def fq2_table():
    """[(op, a, b, c)]"""
    els = fq2_elements()
    t = [(F2_MUL, a, b, 0) for a in els for b in els]
    t += [(F2_EQ, a, b, 0) for a in els for b in els]
    for op in (F2_SQR, F2_INV, F2_CONJ, F2_NEG, F2_IS_ZERO):
        t += [(op, a, (0, 0), 0) for a in els]
    t += [(F2_MUL_FQ, a, (0, 0), c) for a in els for c in (0, M, TWO_P - 1, P, E12[10])]
    t += [(F2_ONE, (0, 0), (0, 0), 0)] * 3
    return t


# ----------------------------------------------------------------------------- G2 (lane pairs)
(G2_DBL, G2_ADD_AFF, G2_ADD, G2_PSI, G2_PSI_JAC, G2_WALK, G2_CLEAR) = range(7)
G2_OP_NAMES = ["jac_dbl", "jac_add_aff", "jac_add", "g2p_psi", "g2p_psi_jac",
               "g2p_walk_lines+psi_test", "g2p_clear_cofactor"]


def g2_points():
    """[(name, point or None, order is large)]"""
    from test_native_arith import _rand_curve, _small_component
    rng = random.Random(0x62)
    pts = [("generator", B.G2_GEN, True)]
    for i in range(2):
        pts.append(("subgroup %d" % i, B.g2_mul(B.G2_GEN, rng.randrange(1, B.R)), True))
    pts.append(("infinity", None, False))
    for i in range(2):
        while True:
            p = _rand_curve(rng, 2)
            if not B.g2_in_subgroup(p):
                break
        pts.append(("off subgroup %d" % i, p, True))
    for prime in (13, 23):
        pts.append(("order %d" % prime, _small_component(rng, 2, prime, B.H2), False))
    return pts


def _raw2(v, rng):
    return (to_m(v[0], rng.random() < 0.4), to_m(v[1], rng.random() < 0.4))


def raw_aff(pt, rng):
    """(x, y, inf) raw"""
    if pt is None:
        return ((0, 0), (0, 0), 1)
    return (_raw2(pt[0], rng), _raw2(pt[1], rng), 0)


def raw_jac(pt, rng, z=None):
    """(X, Y, Z) raw with a random (or given) Z; infinity is Z = 0 with arbitrary X, Y."""
    if pt is None:
        return (_raw2((rng.randrange(P), rng.randrange(P)), rng), _raw2((1, 0), rng),
                (rng.choice((0, P)), rng.choice((0, P))))
    if z is None:
        z = (rng.randrange(1, P), rng.randrange(P))
    z2 = B.f2_sqr(z)
    z3 = B.f2_mul(z2, z)
    return (_raw2(B.f2_mul(pt[0], z2), rng), _raw2(B.f2_mul(pt[1], z3), rng), _raw2(z, rng))


def jac_value(j):
    """raw (X, Y, Z) -> affine canonical point or None"""
    x, y, z = f2v(j[0]), f2v(j[1]), f2v(j[2])
    if z == (0, 0):
        return None
    zi = B.f2_inv(z)
    zi2 = B.f2_sqr(zi)
    return (B.f2_mul(x, zi2), B.f2_mul(y, B.f2_mul(zi2, zi)))


def g2_table():
    """[(op, aff, jac1, jac2, expect, tag)]: expect is ("jac", point-or-None), ("aff", (x, y)),
    ("walk", point-or-SKIP, flag)."""
    from test_cofactor import clear_cofactor_psi, mul as cmul, psi
    rng = random.Random(0x6262)
    pts = g2_points()
    inf_a = raw_aff(None, rng)
    t = []

    def J(pt):
        return raw_jac(pt, rng)

    def A(pt):
        return raw_aff(pt, rng)

    for name, pt, _big in pts:
        t.append((G2_DBL, inf_a, J(pt), J(None), ("jac", B.g2_add(pt, pt)), name))
        t.append((G2_DBL, inf_a, raw_jac(pt, rng, (1, 0)), J(None), ("jac", B.g2_add(pt, pt)),
                  name + " z=1"))
        t.append((G2_PSI_JAC, inf_a, J(pt), J(None), ("jac", psi(pt) if pt else None), name))
        t.append((G2_CLEAR, A(pt), J(None), J(None),
                  ("jac", clear_cofactor_psi(pt) if pt else None), name))
        if pt is None:
            continue
        t.append((G2_PSI, A(pt), J(None), J(None), ("aff", psi(pt)), name))
        in_g2 = B.g2_in_subgroup(pt)
        t.append((G2_WALK, A(pt), J(None), J(None),
                  ("walk", cmul(pt, abs(B.X)) if _big else "skip", int(in_g2)), name))
    named = [(n, p) for n, p, _ in pts]
    combos = []
    for i, (n1, p1) in enumerate(named):
        n2, p2 = named[(i + 1) % len(named)]
        combos += [(n1 + " + " + n2, p1, p2), (n1 + " + same", p1, p1),
                   (n1 + " - same", p1, B.g2_neg(p1) if p1 else None),
                   (n1 + " + inf", p1, None), ("inf + " + n1, None, p1)]
    for tag, p1, p2 in combos:
        want = ("jac", B.g2_add(p1, p2))
        t.append((G2_ADD_AFF, A(p2), J(p1), J(None), want, tag))
        t.append((G2_ADD, inf_a, J(p1), J(p2), want, tag))
    if len(t) % 2 == 0:  # an odd item count: the last wave of lane pairs is partial
        t.append((G2_DBL, inf_a, J(B.G2_GEN), J(None), ("jac", B.g2_add(B.G2_GEN, B.G2_GEN)), "pad"))
    return t


# ----------------------------------------------------------------------------- GT (6 lanes)
(GT_MUL, GT_SQR, GT_CYC_SQR, GT_FROB1, GT_FROB2, GT_FROB3, GT_CONJ, GT_FINAL_EXP, GT_EASY,
 GT_EXP_X) = range(10)
GT_OP_NAMES = ["mul", "sqr", "cyc_sqr", "frob1", "frob2", "frob3", "conj", "final_exp",
               "easy_part", "exp_by_x"]


def gt_to_flat(raw6):
    """six raw Fq2 coefficients f_k (gt6.h basis) -> the oracle's 12 coefficients over w"""
    e = [0] * 12
    for k, c in enumerate(raw6):
        a0, a1 = f2v(c)
        e[k] = (a0 - a1) % P
        e[k + 6] = a1
    return e


def flat_to_gt(e):
    """oracle element -> six canonical (c0, c1)"""
    return [((e[k] + e[k + 6]) % P, e[k + 6]) for k in range(6)]


def _f12_pow(a, n):
    r = B.f12_one()
    for bit in bin(n)[2:]:
        r = B.f12_sqr(r)
        if bit == "1":
            r = B.f12_mul(r, a)
    return r


def _easy(f):
    """gt6.h easy_part: f^(p^6 - 1)"""
    return B.f12_mul(B.f12_conj(f), B.f12_inv(f))


def _cyclotomic(f):
    t = _easy(f)
    return B.f12_mul(B.f12_frob(B.f12_frob(t)), t)      # ^(p^2 + 1)


def gt_ref(op, a, b):
    """six canonical (c0, c1) of the result"""
    fa, fb = gt_to_flat(a), gt_to_flat(b)
    if op == GT_MUL:
        r = B.f12_mul(fa, fb)
    elif op in (GT_SQR, GT_CYC_SQR):
        r = B.f12_sqr(fa)
    elif op in (GT_FROB1, GT_FROB2, GT_FROB3):
        r = fa
        for _ in range(op - GT_FROB1 + 1):
            r = B.f12_frob(r)
    elif op == GT_CONJ:
        r = B.f12_conj(fa)
    elif op == GT_FINAL_EXP:
        e = B.final_exponentiation(fa)
        r = B.f12_mul(B.f12_mul(e, e), e)      # the HHT chain gives the cube
    elif op == GT_EASY:
        r = _easy(fa)
    elif op == GT_EXP_X:
        r = B.f12_conj(_f12_pow(fa, abs(B.X)))
    else:
        raise ValueError(op)
    return flat_to_gt(r)


def gt_table():
    """[(op, a, b, tag)]: a, b lists of six raw (c0, c1)."""
    rng = random.Random(0x67)

    def rnd(lazy=True):
        return [(to_m(rng.randrange(P), lazy and rng.random() < 0.3),
                 to_m(rng.randrange(P), lazy and rng.random() < 0.3)) for _ in range(6)]

    def only(k):
        return [(to_m(rng.randrange(1, P)), to_m(rng.randrange(1, P))) if i == k else (0, 0)
                for i in range(6)]

    top = [(TWO_P - 1, TWO_P - 1)] * 6
    one = [(M, 0)] + [(0, 0)] * 5
    zero = [(0, 0)] * 6
    r0, r1, r2 = rnd(), rnd(), rnd(False)
    cyc = [(to_m(c0), to_m(c1)) for c0, c1 in flat_to_gt(_cyclotomic(gt_to_flat(r0)))]
    cyc_lazy = [(c0 + P, c1) for c0, c1 in cyc]
    t = []
    for op in (GT_MUL, GT_SQR):
        t += [(op, r0, r1, "random"), (op, r2, r0, "random canonical"), (op, top, top, "all 2p-1"),
              (op, top, r1, "2p-1 x random"), (op, one, r1, "one"), (op, r0, one, "x one"),
              (op, zero, r1, "zero"), (op, only(0), r1, "f0 only"), (op, only(5), r1, "f5 only"),
              (op, only(5), only(5), "f5 x f5"), (op, r1, only(5), "x f5 only")]
    for op in (GT_FROB1, GT_FROB2, GT_FROB3, GT_CONJ):
        t += [(op, r0, zero, "random"), (op, r2, zero, "random canonical"), (op, one, zero, "one"),
              (op, zero, zero, "zero"), (op, only(0), zero, "f0 only"), (op, only(5), zero, "f5 only")]
    for op in (GT_CYC_SQR, GT_EXP_X):
        t += [(op, cyc, zero, "cyclotomic"), (op, cyc_lazy, zero, "cyclotomic lazy"),
              (op, one, zero, "one")]
    for op in (GT_EASY, GT_FINAL_EXP):
        t += [(op, r0, zero, "random"), (op, one, zero, "one"), (op, only(5), zero, "f5 only")]
    return t


# ----------------------------------------------------------------------------- marshalling
def words(vals, nlimbs=12):
    """integers -> a ctypes uint32 array of little-endian limbs"""
    buf = b"".join(v.to_bytes(4 * nlimbs, "little") for v in vals)
    return (ctypes.c_uint32 * (len(buf) // 4)).from_buffer_copy(buf)


def u32(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


def out_words(n):
    return (ctypes.c_uint32 * n)()


def ints(arr, nlimbs=12):
    raw = bytes(arr)
    step = 4 * nlimbs
    return [int.from_bytes(raw[i:i + step], "little") for i in range(0, len(raw), step)]


# ----------------------------------------------------------------------------- runners + checks
# The tables and their references are built once per process and shared by every test that
# runs them (host fallback, each device variant); nothing mutates them.
@functools.lru_cache(maxsize=None)
def fq_cases():
    table = fq_table()
    return table, [fq_ref(*item) for item in table]


@functools.lru_cache(maxsize=None)
def acc_cases():
    table = acc_table()
    return table, [acc_ref(mode, terms) for mode, terms, _tag in table]


@functools.lru_cache(maxsize=None)
def fq2_cases():
    table = fq2_table()
    return table, [fq2_ref(*item) for item in table]


@functools.lru_cache(maxsize=None)
def g2_cases():
    return g2_table()


@functools.lru_cache(maxsize=None)
def gt_cases():
    table = gt_table()
    return table, [gt_ref(op, a, b) for op, a, b, _tag in table]


def run_fq(fn, table):
    """fn(n, ops, a, b, c, d, out, flag) -> [(out, flag)]"""
    n = len(table)
    out, flag = out_words(12 * n), out_words(n)
    rc = fn(n, u32([t[0] for t in table]), *(words([t[i] for t in table]) for i in (1, 2, 3, 4)),
            out, flag)
    assert rc == 0, "harness status %d" % rc
    return list(zip(ints(out), list(flag)))


def check_fq(table, want, got, mul2_exact=True):
    """Exact integers and < 2p (mul2 outside the subroutine build: congruence and < 2p).
    Returns the failing items (op name, operands, got, want)."""
    bad = []
    for item, (wo, wf), (o, f) in zip(table, want, got):
        op = item[0]
        if op == OP_MUL2 and not mul2_exact:
            ok = o < TWO_P and o % P == wo % P
        else:
            ok = o == wo and o < TWO_P
        if not ok or f != wf:
            bad.append((FQ_OP_NAMES[op],) + tuple(hex(x) for x in item[1:]) + ((hex(o), f), (hex(wo), wf)))
    return bad


def acc_arrays(table):
    n = len(table)
    a, b = [0] * (12 * n), [0] * (12 * n)
    for i, (mode, terms, _tag) in enumerate(table):
        for t, term in enumerate(terms):
            if mode == ACC_KARA:
                a[12 * i + 2 * t], a[12 * i + 2 * t + 1] = term[0], term[1]
                b[12 * i + 2 * t], b[12 * i + 2 * t + 1] = term[2], term[3]
            else:
                a[12 * i + t], b[12 * i + t] = term
    return u32([t[0] for t in table]), u32([len(t[1]) for t in table]), words(a), words(b)


def run_acc(fn, table):
    """fn(n, mode, nt, a, b, out0, out1): 12 operand slots per item in a and b (kara: term t in
    slots 2t, 2t + 1 = (a0, a1) / (b0, b1)) -> [(out0, out1)]"""
    n = len(table)
    o0, o1 = out_words(12 * n), out_words(12 * n)
    rc = fn(n, *acc_arrays(table), o0, o1)
    assert rc == 0, "harness status %d" % rc
    return list(zip(ints(o0), ints(o1)))


def check_acc(table, want, got):
    """Exact integers and < 2p; an accumulator a mode leaves untouched must reduce to redc of its
    start value too (mac: out1 = redc(0) = 0, mac2: out0 = 0)."""
    bad = []
    for (mode, _terms, tag), w, g in zip(table, want, got):
        if tuple(g) != tuple(w) or any(x >= TWO_P for x in g):
            bad.append((ACC_MODE_NAMES[mode], tag, [hex(x) for x in g], [hex(x) for x in w]))
    return bad


def run_fq2(fn, table):
    """fn(n, ops, a, b, c, out, flag) -> [((c0, c1) raw, flag)]"""
    n = len(table)
    out, flag = out_words(24 * n), out_words(n)
    rc = fn(n, u32([t[0] for t in table]), words([c for t in table for c in t[1]]),
            words([c for t in table for c in t[2]]), words([t[3] for t in table]), out, flag)
    assert rc == 0, "harness status %d" % rc
    v = ints(out)
    return [((v[2 * i], v[2 * i + 1]), flag[i]) for i in range(n)]


def check_fq2(table, want, got):
    """Canonical residues against the oracle, every component < 2p."""
    bad = []
    for item, (wv, wf), (g, f) in zip(table, want, got):
        if f2v(g) != wv or f != wf or any(x >= TWO_P for x in g):
            bad.append((F2_OP_NAMES[item[0]], [hex(x) for x in item[1] + item[2]], hex(item[3]),
                        ([hex(x) for x in g], f), (wv, wf)))
    return bad


LINE_WORDS = 68 * 3 * 24     # the projective line triples of one point (pairing.h MILLER_STEPS)


def aff_words(aff):
    x, y, inf = aff
    raw = b"".join(c.to_bytes(48, "little") for c in x + y) + inf.to_bytes(4, "little")
    return (ctypes.c_uint32 * 49).from_buffer_copy(raw)


def run_g2(fn, table):
    """fn(n, ops, aff, j1, j2, out, flag, lines) -> [((X, Y, Z) raw, flag, line values raw)]"""
    n = len(table)
    aff = (ctypes.c_uint32 * (49 * n)).from_buffer_copy(b"".join(bytes(aff_words(t[1])) for t in table))
    j1 = words([c for t in table for f in t[2] for c in f])
    j2 = words([c for t in table for f in t[3] for c in f])
    out, flag, lines = out_words(72 * n), out_words(n), out_words(LINE_WORDS * n)
    rc = fn(n, u32([t[0] for t in table]), aff, j1, j2, out, flag, lines)
    assert rc == 0, "harness status %d" % rc
    v = ints(out)
    raw = bytes(lines)
    return [(tuple((v[6 * i + 2 * k], v[6 * i + 2 * k + 1]) for k in range(3)), flag[i],
             ints(raw[4 * LINE_WORDS * i:4 * LINE_WORDS * (i + 1)]) if table[i][0] == G2_WALK else None)
            for i in range(n)]


def host_lines(ht, aff):
    """The one-lane line table of the same raw point from the host library (ht_g2_proj_lines_raw)."""
    out = out_words(LINE_WORDS)
    assert ht.ht_g2_proj_lines_raw(aff_words(aff), out) == 0
    return ints(out)


def check_g2(table, got, ht=None):
    """The point (Jacobian -> affine canonical residues) against the oracle, every limb value
    < 2p, the subgroup flag of the walk and, given the host library, the walk's 68 line triples
    as canonical residues against the one-lane g2_proj_lines (points of large order: the walk of
    a point of order 13 or 23 passes through degenerate steps, only its verdict is defined)."""
    bad = []
    for (op, aff, _j1, _j2, want, tag), (j, f, lines) in zip(table, got):
        ok = all(x < TWO_P for c in j for x in c)
        if want[0] == "walk":
            ok = ok and f == want[2] and (want[1] == "skip" or jac_value(j) == want[1])
            if ht is not None and want[1] != "skip":
                ok = ok and all(x < TWO_P for x in lines)
                ok = ok and [from_m(x) for x in lines] == [from_m(x) for x in host_lines(ht, aff)]
        else:
            ok = ok and jac_value(j) == want[1]
        if not ok:
            bad.append((G2_OP_NAMES[op], tag))
    return bad


def gt_arrays(items):
    a = words([c for it in items for pair in it[1] for c in pair])
    b = words([c for it in items for pair in it[2] for c in pair])
    return a, b


def gt_blocks(table, rep):
    """One operation per wave: the items of each op in chunks of the wave's whole groups (10 or
    3); the last chunk of an op is usually short, so its wave has idle groups.  Returns the item
    order and the per-block (op, first, count)."""
    full = 64 // (6 * rep)
    order = sorted(range(len(table)), key=lambda i: table[i][0])
    blocks = []
    s = 0
    while s < len(order):
        op = table[order[s]][0]
        e = s
        while e < len(order) and e - s < full and table[order[e]][0] == op:
            e += 1
        blocks.append((op, s, e - s))
        s = e
    return order, blocks


def run_gt_device(fn, table, rep):
    """fn(nblk, nitems, rep, blk_op, blk_first, blk_cnt, a, b, out) -> per item six raw (c0, c1);
    asserts that the rep sub-lane copies of every coefficient agree."""
    order, blocks = gt_blocks(table, rep)
    items = [table[i] for i in order]
    a, b = gt_arrays(items)
    out = out_words(144 * rep * len(items))
    rc = fn(len(blocks), len(items), rep, u32([x[0] for x in blocks]), u32([x[1] for x in blocks]),
            u32([x[2] for x in blocks]), a, b, out)
    assert rc == 0, "harness status %d" % rc
    v = ints(out)
    got = [None] * len(table)
    for pos, i in enumerate(order):
        copies = [[(v[12 * (rep * pos + s) + 2 * k], v[12 * (rep * pos + s) + 2 * k + 1])
                   for k in range(6)] for s in range(rep)]
        assert all(c == copies[0] for c in copies), ("sub-lanes disagree", table[i][3])
        got[i] = copies[0]
    return got


def check_gt(table, want, got):
    """got: per item six raw (c0, c1); canonical residues against the oracle, every limb value < 2p"""
    bad = []
    for (op, _a, _b, tag), w, g in zip(table, want, got):
        if [f2v(c) for c in g] != w or any(x >= TWO_P for c in g for x in c):
            bad.append((GT_OP_NAMES[op], tag))
    return bad
