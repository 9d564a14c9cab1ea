#!/usr/bin/env python3
"""Bounds interpreter of the point formulas on the redundant 13 x 30 form (field.h FqW, curve.h
jacw_dbl / jacw_add_aff / jacw_add / jacw_eq_aff, and xadic_mul_sac8_w with its table chain).

The formulas are written once, over an abstract set of field operations, in the order and with the
normalisations and subtraction constants of curve.h.  Two implementations of the operations run them:

  Bounds   pushes (per-limb maximum, value maximum in units of p) through every operation and
           refuses: a limb sum that could pass 2^32 - 1; a product operand outside the bound the
           relaxed blocks were generated for (gen_fq_rr.W_LIMBS); a subtraction constant with a limb
           below its subtrahend's bound; a zero test on anything but a product result below 2p.
  Limbs    runs them on actual limbs (the generator's simulator for the products), for the tests.

check_closure() shows that from the declared loop-entry bound ENTRY every output of jacw_dbl and of
both additions, with and without the special-case exits, is inside ENTRY again.
check_items_closure() does the same for the item pass's x-adic multiplication (curve.h
xadic_mul_sac8_w): the packed table chain, the column, the even-d0 correction and the exit.
check_walk_closure() runs the calls of the G1 bucket walk (hbtc_msm.hip k_msm_buckets<Fq> over JacW) in
the walk's order: the step, the flush, walk_finish and the exit.

Usage: tools/rr_bounds.py            (prints the bound of every output and "closure ok")
"""
import os
import sys
from fractions import Fraction

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_fq_rr as G  # noqa: E402

N, W, M, P = G.N, G.W, G.M, G.P_MOD
U32 = (1 << 32) - 1
X_ABS = 0xd201000000010000      # |x| of BLS12-381
PACK_V = Fraction(3, 2)          # everything that is packed (field.h fw_pack) is a product result below 1.5p
ENTRY_V = 12                     # the loop invariant: every coordinate of the accumulator <= 12 p,
BASE_V = 12                      # of a Jacobian base likewise; an affine base is a product result


class BoundsError(Exception):
    pass


def top_of(v):
    """the largest top limb of a value <= v p (every limb is non-negative)"""
    return int(v * P) >> (W * (N - 1))


class Bd:
    """per-limb maxima and the value maximum in units of p"""

    def __init__(self, limbs, v):
        self.l = list(limbs)
        self.v = Fraction(v)
        self.l[N - 1] = min(self.l[N - 1], top_of(self.v))

    def within(self, other):
        return all(a <= b for a, b in zip(self.l, other.l)) and self.v <= other.v

    def __repr__(self):
        return "limbs <= 2^30 + %d, top <= %d, value <= %.3f p" % (max(self.l[:N - 1]) - (1 << W), self.l[N - 1],
                                                                  float(self.v))


def strict(v):
    return Bd([M] * N, v)


def entry(v=ENTRY_V):
    return Bd([M + G.W_SLACK] * (N - 1) + [U32], v)


class Bounds:
    """the bounds-only interpreter"""
    consts = dict(((b, k), G.sub_const(b, k)) for b, k in G.SUB_CONSTS)

    def __init__(self, forced=None):
        self.forced = forced or {}

    def _chk(self, limbs, what):
        if max(limbs) > U32:
            raise BoundsError("%s: a limb could reach %d > 2^32 - 1" % (what, max(limbs)))
        return limbs

    def add(self, a, b):
        return Bd(self._chk([x + y for x, y in zip(a.l, b.l)], "add"), a.v + b.v)

    def dbl(self, a):
        return self.add(a, a)

    def sub(self, a, s, c):
        cl = self.consts[c]
        for i in range(N):
            if cl[i] < s.l[i]:
                raise BoundsError("sub: limb %d of constant %s is %d, the subtrahend may reach %d" % (i, c, cl[i], s.l[i]))
        return Bd(self._chk([x + y for x, y in zip(a.l, cl)], "sub"), a.v + c[1])

    def norm(self, a):
        self._chk(a.l, "norm")
        return Bd([M] + [M + (a.l[i - 1] >> W) for i in range(1, N - 1)] + [a.l[N - 1] + (a.l[N - 2] >> W)], a.v)

    def _operand(self, a, what):
        for i in range(N):
            if a.l[i] > G.W_LIMBS[i]:
                raise BoundsError("%s: operand limb %d may reach %d, the block takes %d" % (what, i, a.l[i], G.W_LIMBS[i]))

    def mul(self, a, b):
        self._operand(a, "mul")
        self._operand(b, "mul")
        return strict(a.v * b.v * P / (1 << G.RBITS) + 1)

    def sqr(self, a):
        self._operand(a, "sqr")
        return strict(a.v * a.v * P / (1 << G.RBITS) + 1)

    def is_zero(self, a, tag):
        """a == 0 or a == p: sees every representative of 0 only for strict limbs and a value < 2p"""
        if max(a.l[:N - 1]) > M or a.v >= 2:
            raise BoundsError("zero test %s on %r" % (tag, a))
        return self.forced.get(tag, False)

    def one(self):
        return strict(1)

    def zero(self):
        return Bd([0] * N, 0)

    def canon_eq(self, a, b):
        if max(a.l[:N - 1] + b.l[:N - 1]) > M or a.v >= 2 or b.v >= 2:
            raise BoundsError("comparison of %r and %r" % (a, b))
        return True

    def sel(self, c, a, b):
        """either of the two: the larger bound, limb by limb"""
        return Bd([max(x, y) for x, y in zip(a.l, b.l)], max(a.v, b.v))

    def const(self, v):
        """a constant below p on limbs < 2^30 (fq_rr.h RR_BETA, RR_K_OUT)"""
        return strict(1)

    def pack(self, a):
        """field.h fw_pack: only a product result below 1.5p goes onto 12 words"""
        if max(a.l) > M or a.v > PACK_V:
            raise BoundsError("packing %r" % (a,))
        return a

    def unpack(self, a):
        return strict(PACK_V)


def val(l):
    return sum(x << (W * i) for i, x in enumerate(l))


class Limbs:
    """the same operations on actual limbs"""
    MUL, _ = G.schedule(False, G.W_LIMBS, G.W_LIMBS)
    SQR, _ = G.schedule(True, G.W_LIMBS)

    def _chk(self, l):
        assert all(0 <= x <= U32 for x in l)
        return l

    def add(self, a, b):
        return self._chk([x + y for x, y in zip(a, b)])

    def dbl(self, a):
        return self.add(a, a)

    def sub(self, a, s, c):
        return self._chk([x + y - z for x, y, z in zip(a, G.sub_const(*c), s)])

    def norm(self, a):
        return [a[0] & M] + [(a[i] & M) + (a[i - 1] >> W) for i in range(1, N - 1)] + [a[N - 1] + (a[N - 2] >> W)]

    def mul(self, a, b):
        return G.run(self.MUL, a, b)

    def sqr(self, a):
        return G.run(self.SQR, a)

    def is_zero(self, a, tag):
        return val(a) in (0, P)

    def one(self):
        return G.limbs(G.ONE)

    def zero(self):
        return [0] * N

    def canon_eq(self, a, b):
        assert val(a) < 2 * P and val(b) < 2 * P
        return val(a) % P == val(b) % P

    def sel(self, c, a, b):
        return a if c else b

    def const(self, v):
        return G.limbs(v * G.ONE % P)

    def pack(self, a):
        """12 words of 32 bits and back: the same limbs when the integer is below 2^384"""
        assert max(a) <= M and val(a) < 1 << 384
        return G.limbs(val(a) & ((1 << 384) - 1))

    def unpack(self, a):
        return a


# ------------------------------------------------------------------------------ the formulas
S1, S2, S2B, S2C, S2D = (1, 4), (2, 4), (2, 8), (2, 10), (2, 14)


def jacw_set_inf(o):
    return (o.one(), o.one(), o.zero())


def jacw_dbl(o, p):
    """dbl-2009-l (a = 0) with D = 2((X + B)^2 - A - C) taken as the product X (4B): a product result,
    so X3, Y3 stay a few p and the invariant closes."""
    X, Y, Z = p
    A = o.sqr(X)
    B = o.sqr(Y)
    C = o.sqr(B)
    B4 = o.norm(o.dbl(o.dbl(B)))
    D = o.mul(X, B4)
    E = o.norm(o.add(o.dbl(A), A))
    F = o.sqr(E)
    X3 = o.norm(o.sub(F, o.dbl(D), S2))
    t = o.norm(o.sub(D, X3, S2B))
    C4 = o.norm(o.dbl(o.dbl(C)))
    Y3 = o.norm(o.sub(o.mul(E, t), o.dbl(C4), S2C))
    Z3 = o.norm(o.dbl(o.mul(Y, Z)))
    return (X3, Y3, Z3)


def _add_tail(o, p, X1, S1v, H, HH, rr, z3):
    """the common second half of madd-2007-bl and add-2007-bl: X1 = U1 (or X), S1v = S1 (or Y)"""
    I = o.norm(o.dbl(o.dbl(HH)))
    J = o.mul(H, I)
    r2 = o.norm(o.dbl(rr))
    V = o.mul(X1, I)
    x3 = o.norm(o.sub(o.sqr(r2), J, S1))
    x3 = o.norm(o.sub(x3, o.dbl(V), S2))
    t = o.norm(o.sub(V, x3, S2D))
    y3 = o.mul(r2, t)
    t = o.mul(S1v, J)
    y3 = o.norm(o.sub(y3, o.dbl(t), S2))
    return (x3, y3, z3)


def jacw_add_aff(o, p, q):
    """madd-2007-bl: q = (x, y) affine and not infinity"""
    X, Y, Z = p
    z1z1 = o.sqr(Z)
    if o.is_zero(z1z1, "p_inf"):
        return (q[0], q[1], o.one())
    u2 = o.mul(q[0], z1z1)
    s2 = o.mul(o.mul(q[1], Z), z1z1)
    H = o.norm(o.sub(u2, X, S2D))
    rr = o.norm(o.sub(s2, Y, S2D))
    HH = o.sqr(H)
    if o.is_zero(HH, "h_zero"):
        if o.is_zero(o.mul(rr, o.one()), "r_zero"):
            return jacw_dbl(o, p)
        return jacw_set_inf(o)
    z3 = o.sqr(o.norm(o.add(Z, H)))
    z3 = o.norm(o.sub(z3, o.add(z1z1, HH), S2))
    return _add_tail(o, p, X, Y, H, HH, rr, z3)


def jacw_add(o, p, q):
    """add-2007-bl: both Jacobian"""
    X, Y, Z = p
    z1z1 = o.sqr(Z)
    if o.is_zero(z1z1, "p_inf"):
        return q
    z2z2 = o.sqr(q[2])
    if o.is_zero(z2z2, "q_inf"):
        return p
    u1 = o.mul(X, z2z2)
    u2 = o.mul(q[0], z1z1)
    s1 = o.mul(o.mul(Y, q[2]), z2z2)
    s2 = o.mul(o.mul(q[1], Z), z1z1)
    H = o.norm(o.sub(u2, u1, S1))
    rr = o.norm(o.sub(s2, s1, S1))
    HH = o.sqr(H)
    if o.is_zero(HH, "h_zero"):
        if o.is_zero(o.mul(rr, o.one()), "r_zero"):
            return jacw_dbl(o, p)
        return jacw_set_inf(o)
    z3 = o.sqr(o.norm(o.add(Z, q[2])))
    z3 = o.norm(o.sub(z3, o.add(z1z1, z2z2), S2))
    z3 = o.mul(z3, H)
    return _add_tail(o, p, u1, s1, H, HH, rr, z3)


def jacw_eq_aff(o, p, ax, ay):
    """is p (not infinity) the affine point (ax, ay)?  Both sides as product results, then canonical."""
    X, Y, Z = p
    z2 = o.sqr(Z)
    z3 = o.mul(z2, Z)
    if not o.canon_eq(o.mul(ax, z2), o.mul(X, o.one())):
        return False
    return o.canon_eq(o.mul(ay, z3), o.mul(Y, o.one()))


def jacw_mul_x(o, q, affine, k=X_ABS):
    acc = jacw_set_inf(o)
    for b in range(63, -1, -1):
        acc = jacw_dbl(o, acc)
        if (k >> b) & 1:
            acc = jacw_add_aff(o, acc, q) if affine else jacw_add(o, acc, q)
    return acc


# --------------------------------------- the x-adic multiplication of the item pass (xadic_mul_sac8_w)
def neg(o, a):
    """fw_neg: a product result or constant (strict limbs, below 3p) -> weakly normalised, <= 4p"""
    return o.norm(o.sub(o.zero(), a, S1))


def jacw_madd_generic(o, p, qx, qy):
    """madd-2007-bl without the exceptional cases (jac_madd_generic's schedule): Z3 = 2 Z1 H as a product"""
    X, Y, Z = p
    z1z1 = o.sqr(Z)
    u2 = o.mul(qx, z1z1)
    s2 = o.mul(o.mul(qy, Z), z1z1)
    H = o.norm(o.sub(u2, X, S2D))
    rr = o.norm(o.sub(s2, Y, S2D))
    HH = o.sqr(H)
    z3 = o.norm(o.dbl(o.mul(Z, H)))
    return _add_tail(o, p, X, Y, H, HH, rr, z3)


def coz_add_w(o, a, b):
    """co-Z sum of product results a and b: (the sum, a at the sum's Z, h); all product results but h"""
    ax, ay = a
    h = o.norm(o.sub(b[0], ax, S1))
    r = o.norm(o.sub(b[1], ay, S1))
    hh = o.sqr(h)
    hhh = o.mul(hh, h)
    v = o.mul(ax, hh)
    ay = o.mul(ay, hhh)
    t = o.norm(o.sub(o.sqr(r), hhh, S1))
    t = o.norm(o.sub(t, o.dbl(v), S2))
    one = o.one()
    sx = o.mul(t, one)
    t = o.norm(o.sub(v, t, S2C))
    t = o.norm(o.sub(o.mul(r, t), ay, S1))
    return (sx, o.mul(t, one)), (v, ay), h


def xadic_table8_chain_w(o, p, xpj):
    """The eight packed entries (slot u1 + 2 u2 + 4 u3) and the packed Z* from p = (x, y) and xpj = (X, Y, Z)
    as fw_from_fq leaves them, in the order of curve.h xadic_table8_chain_w."""
    beta = o.const(G.BETA)
    pk = lambda e: (o.pack(e[0]), o.pack(e[1]))
    up = lambda e: (o.unpack(e[0]), o.unpack(e[1]))
    z = xpj[2]
    z2 = o.sqr(z)
    z3 = o.mul(z2, z)
    pw = (o.mul(p[0], z2), o.mul(p[1], z3))
    sw, xw, h = coz_add_w(o, (xpj[0], xpj[1]), pw)
    T = {"S": pk(sw), "X": pk(xw)}
    st = {"h2": o.sqr(h)}
    st["h3"] = o.mul(st["h2"], h)
    T["P"] = pk((o.mul(pw[0], st["h2"]), o.mul(pw[1], st["h3"])))
    st["zs"] = o.mul(z, h)

    def rescale(*names):
        for n in names:
            e = up(T[n])
            T[n] = pk((o.mul(e[0], st["h2"]), o.mul(e[1], st["h3"])))

    def sum_(out, U, V):
        v = up(T[V])
        mv = (o.mul(v[0], beta), v[1])
        s, u, h = coz_add_w(o, up(T[U]), mv)
        T[out], T[U] = pk(s), pk(u)
        st["h2"] = o.sqr(h)
        st["h3"] = o.mul(st["h2"], h)
        st["zs"] = o.mul(st["zs"], h)

    sum_(4, "P", "X")
    rescale("X", "S")
    sum_(5, "S", "X")
    rescale("P", 4)
    sum_(2, "P", "P")
    rescale("S", 4, 5)
    sum_(3, "S", "P")
    rescale("P", 2, 4, 5)
    sum_(6, "P", "S")
    rescale("S", 2, 3, 4, 5)
    sum_(7, "S", "S")
    rescale("P", 2, 3, 4, 5, 6)
    tab = [T["P"], T["S"]] + [T[k] for k in range(2, 8)]
    return tab, o.pack(st["zs"])


def sac_recode(k0, d, nbits):
    """curve.h xadic_sac_recode: bit i of m[j] = u_(j+1)[i]"""
    m = []
    for k in d:
        mk = 0
        for i in range(nbits + 1):
            odd = k & 1
            negi = ((~k0 >> (i + 1)) & 1) if i < nbits else 0
            mk |= odd << i
            k = (k >> 1) + (odd & negi)
        m.append(mk)
    return m


def column(o, acc, e, negate):
    """one column: a doubling, then the mixed addition of the unpacked entry, its y negated or not"""
    acc = jacw_dbl(o, acc)
    x, y = o.unpack(e[0]), o.unpack(e[1])
    y = o.sel(negate, neg(o, y), y)
    return jacw_madd_generic(o, acc, x, y)


def xadic_mul_sac8_w(o, p, xpj, d, nbits):
    """[d0 + d1 x + d2 mu + d3 mu x] p as curve.h xadic_mul_sac8_w runs it; the three coordinates as
    fw_to_fq's product by R leaves them, still on 13 limbs"""
    tab, zsp = xadic_table8_chain_w(o, p, xpj)
    k0 = d[0] | 1
    m = sac_recode(k0, d[1:], nbits)
    ent = lambda i: tab[((m[0] >> i) & 1) + 2 * ((m[1] >> i) & 1) + 4 * ((m[2] >> i) & 1)]
    e = ent(nbits)
    acc = (o.unpack(e[0]), o.unpack(e[1]), o.one())
    for i in range(nbits - 1, -1, -1):
        acc = column(o, acc, ent(i), ((k0 >> (i + 1)) & 1) == 0)
    return correction_and_exit(o, acc, tab[0], zsp, d)


def correction_and_exit(o, acc, p0, zsp, d):
    even, zero = d[0] & 1 == 0, not any(d)
    n = jacw_madd_generic(o, acc, o.unpack(p0[0]), neg(o, o.unpack(p0[1])))
    acc = tuple(o.sel(even, a, b) for a, b in zip(n, acc))
    z = o.sel(zero, o.zero(), acc[2])
    z = o.mul(z, o.unpack(zsp))
    kout = o.const(G.K_OUT * pow(G.ONE, -1, P) % P)
    return tuple(o.mul(c, kout) for c in (acc[0], acc[1], z))


# --------------------------------------------------------------------------------- closure
def paths():
    yield {}
    yield {"p_inf": True}
    yield {"q_inf": True}
    yield {"h_zero": True, "r_zero": True}
    yield {"h_zero": True, "r_zero": False}


def check_closure(formulas=None, verbose=False):
    """Every coordinate of every output of the three formulas, on every exit, inside ENTRY again."""
    f = formulas or (jacw_dbl, jacw_add_aff, jacw_add)
    ent = entry()
    acc = (ent, ent, ent)
    aff = (strict(Fraction(3, 2)), strict(Fraction(3, 2)))     # fqr_from_fq: a product result < 1.5 p
    base = (entry(BASE_V),) * 3
    for forced in paths():
        o = Bounds(forced)
        for name, out in (("dbl", f[0](o, acc)), ("add_aff", f[1](o, acc, aff)), ("add", f[2](o, acc, base))):
            for c, b in zip("XYZ", out):
                if verbose and not forced:
                    print("%-8s %s: %r" % (name, c, b))
                if not b.within(ent):
                    raise BoundsError("%s %s leaves the entry bound on path %s: %r" % (name, c, forced, b))
    o = Bounds()
    jacw_eq_aff(o, acc, aff[0], o.norm(o.sub(o.zero(), aff[1], S1)))   # (beta x, -y) of the decode
    inf = jacw_set_inf(o)
    assert all(b.within(ent) for b in inf)
    return True


def check_items_closure(verbose=False):
    """xadic_mul_sac8_w: the table chain from fw_from_fq's outputs (every packed value a product result
    below 1.5p: Bounds.pack refuses anything else), then from the entry bound one column -- a doubling and
    the mixed addition of an entry whose y is negated or not -- back inside the entry bound, the first
    column from the entry itself, the even-d0 correction and the exit."""
    o = Bounds()
    fq = strict(PACK_V)                                        # fw_from_fq: a product result < 1.5 p
    tab, zsp = xadic_table8_chain_w(o, (fq, fq), (fq, fq, fq))
    assert len(tab) == 8
    ent = entry()
    e = (strict(PACK_V), strict(PACK_V))
    for start in ((ent, ent, ent), (o.unpack(e[0]), o.unpack(e[1]), o.one())):
        out = column(o, start, e, True)
        for c, b in zip("XYZ", out):
            if verbose:
                print("column   %s: %r" % (c, b))
            if not b.within(ent):
                raise BoundsError("column %s leaves the entry bound: %r" % (c, b))
    out = correction_and_exit(o, (ent, ent, ent), e, zsp, (0, 0, 0, 0))
    for c, b in zip("XYZ", out):
        if verbose:
            print("exit     %s: %r" % (c, b))
        if max(b.l) > M or b.v >= 2:
            raise BoundsError("exit %s is not a product result below 2p: %r" % (c, b))
    return True


def check_walk_closure(verbose=False):
    """The G1 bucket walk over JacW (hbtc_msm.hip k_msm_buckets<Fq>, msm_walk.h).  Every point the walk
    holds -- run, tot, a snapshot -- starts as jacw_set_inf and is only ever the output of one of the
    three formulas, so it is enough that each call maps the entry bound into itself on every exit:
      the step      run = jacw_add_aff(run, q), q = fw_from_fq of a 12 x 32 coordinate below 2p (a negated
                    term is negated before the conversion): a product result below 1.5p.  On the exit for
                    run = infinity the output is (q.x, q.y, 1);
      the flush     tot = jacw_add(tot, snapshot), the snapshot a stored value of run;
      walk_finish   acc = run; acc = jacw_dbl(acc); acc = jacw_add(acc, run); tot = jacw_add(tot, acc);
      the exit      jacw_to_jac: each coordinate times the constant K_OUT, a product of an operand inside
                    the relaxed blocks' bound, and the result below 2p as part[] holds it.
    The first three are the calls check_closure() covers (add_aff with an affine product result, add with
    a base inside the entry bound, dbl); they are run here again in the walk's order, on every exit."""
    ent = entry()
    q = (strict(PACK_V), strict(PACK_V))
    for forced in paths():
        o = Bounds(forced)
        inf = jacw_set_inf(o)
        for run in (inf, (ent, ent, ent)):
            for tot in (inf, (ent, ent, ent)):
                step = jacw_add_aff(o, run, q)
                flush = jacw_add(o, tot, step)
                acc = jacw_add(o, jacw_dbl(o, step), step)
                fin = jacw_add(o, flush, acc)
                worst = jacw_add(o, jacw_add(o, tot, run), jacw_add(o, jacw_dbl(o, run), run))  # from the bound itself
                for name, out in (("step", step), ("flush", flush), ("finish", acc), ("total", fin), ("entry", worst)):
                    for c, b in zip("XYZ", out):
                        if verbose and not forced and run[0] is ent and tot[0] is ent:
                            print("walk %-6s %s: %r" % (name, c, b))
                        if not b.within(ent):
                            raise BoundsError("walk %s %s leaves the entry bound on path %s: %r" % (name, c, forced, b))
    o = Bounds()
    kout = o.const(G.K_OUT * pow(G.ONE, -1, P) % P)
    for b in (o.mul(ent, kout),):
        if max(b.l) > M or b.v >= 2:
            raise BoundsError("walk exit is not a product result below 2p: %r" % (b,))
    return True


if __name__ == "__main__":
    check_closure(verbose=True)
    print("closure ok: entry %r" % entry())
    check_walk_closure(verbose=True)
    print("bucket walk: step, flush, finish and exit ok")
    check_items_closure(verbose=True)
    print("item pass: table chain, column, correction and exit ok")
