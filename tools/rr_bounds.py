#!/usr/bin/env python3
"""Bounds interpreter of the point formulas on the redundant 13 x 30 form (field.h FqW, curve.h
jacw_dbl / jacw_add_aff / jacw_add / jacw_eq_aff).

The formulas are written once, over an abstract set of field operations, in the order and with the
normalisations and subtraction constants of curve.h.  Two implementations of the operations run them:

  Bounds   pushes (per-limb maximum, value maximum in units of p) through every operation and
           refuses: a limb sum that could pass 2^32 - 1; a product operand outside the bound the
           relaxed blocks were generated for (gen_fq_rr.W_LIMBS); a subtraction constant with a limb
           below its subtrahend's bound; a zero test on anything but a product result below 2p.
  Limbs    runs them on actual limbs (the generator's simulator for the products), for the tests.

check_closure() shows that from the declared loop-entry bound ENTRY every output of jacw_dbl and of
both additions, with and without the special-case exits, is inside ENTRY again.

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


if __name__ == "__main__":
    check_closure(verbose=True)
    print("closure ok: entry %r" % entry())
