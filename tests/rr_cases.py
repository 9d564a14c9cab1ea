"""Case tables and the Python-integer reference of the 13 x 30 Fq code (field.h FqR, fq_rr.h),
shared by tests/test_rr_host.py (host build) and tests/test_gpu_rr.py (gfx950).  A value is the
integer its limbs spell: 13 limbs of 30 bits for an FqR (a R' mod p, R' = 2^390), 12 words of 32
bits for an Fq (a R mod p, R = 2^384).  The product's exact result is
    mont30(T) = (T + ((-T p^-1) mod 2^390) p) / 2^390
(product scanning yields exactly that quotient), so products are compared as exact integers; the
square root and the decode are compared as canonical residues against oracle/bls12_381.py."""
import ctypes
import functools
import random

from oracle import bls12_381 as B
import devarith_cases as D

P = B.P
W, NL = 30, 13
RP = 1 << (W * NL)
NP390 = (-pow(P, -1, RP)) % RP
K_IN = RP * RP * pow(D.R, -1, P) % P
K_OUT = D.R % P
ALL_MAX = RP - 1                      # every limb 2^30 - 1 (beyond the 16p value bound)
(RR_MUL, RR_SQR, RR_FROM_FQ, RR_TO_FQ, RR_ROUND, RR_CANON, RR_EQ, RR_SQRT, RR_SQRT_REF, RR_FQ_MUL,
 RR_FQ_CANON) = range(11)
OP_NAMES = ["mul", "sqr", "from_fq", "to_fq", "round", "canon", "eq", "sqrt_rr", "sqrt", "fq_mul", "fq_canon"]


def mont30(t):
    return (t + ((t * NP390) % RP) * P) >> (W * NL)


def limbs30(v):
    assert 0 <= v < RP
    return [(v >> (W * i)) & ((1 << W) - 1) for i in range(NL)]


def val30(ws):
    return sum(w << (W * i) for i, w in enumerate(ws))


def words32(v):
    assert 0 <= v < 1 << 384
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)] + [0]


def val32(ws):
    assert ws[12] == 0
    return sum(w << (32 * i) for i, w in enumerate(ws[:12]))


# ------------------------------------------------------------------------------------ the table
def table():
    """[(op, a, b)] with a, b integers.  Operands: tests/devarith_cases.py's E (0, 1, p - 1, p,
    2p - 1, limb-boundary values, random ones, all < 2p) plus 16p - 1 and all limbs 2^30 - 1."""
    e = list(D.E)
    wide = e + [16 * P - 1, ALL_MAX]
    rng = random.Random(0x30)
    t = [(RR_MUL, a, b) for a in wide for b in wide]
    t += [(RR_MUL, rng.randrange(16 * P), rng.randrange(16 * P)) for _ in range(300)]
    t += [(RR_SQR, a, 0) for a in wide] + [(RR_SQR, rng.randrange(16 * P), 0) for _ in range(100)]
    t += [(RR_FROM_FQ, a, 0) for a in e] + [(RR_ROUND, a, 0) for a in e]
    t += [(RR_TO_FQ, a, 0) for a in e + [16 * P - 1]]
    t += [(RR_CANON, a, 0) for a in e]
    t += [(RR_EQ, a, b) for a in D.E12 for b in D.E12]
    t += [(RR_EQ, a, a + P) for a in D.E12 if a < P] + [(RR_EQ, a, a - P) for a in D.E12 if a >= P]
    # square roots: E, squares of random values (both representatives), non-residues
    sq = []
    for i in range(12):
        v = rng.randrange(1, P)
        s = v * v % P
        sq.append(D.to_m(s, lazy=i % 2 == 1))
        n = rng.randrange(1, P)
        while pow(n, (P - 1) // 2, P) == 1:
            n = rng.randrange(1, P)
        sq.append(D.to_m(n, lazy=i % 3 == 1))
    t += [(RR_SQRT, a, 0) for a in e + sq]
    return t


def ref(op, a, b):
    """(exact integer or None, residue or None, flag)"""
    if op == RR_MUL:
        return mont30(a * b), None, 0
    if op == RR_SQR:
        return mont30(a * a), None, 0
    if op == RR_FROM_FQ:
        return mont30(a * K_IN), None, 0
    if op == RR_TO_FQ:
        return mont30(a * K_OUT), None, 0
    if op == RR_ROUND:
        return mont30(mont30(a * K_IN) * K_OUT), None, 0
    if op == RR_CANON:
        return (a - P if a >= P else a), None, 0
    if op == RR_EQ:
        return 0, None, int((a - b) % P == 0)
    if op == RR_SQRT:
        v = D.from_m(a)
        y = pow(v, (P + 1) // 4, P)
        return None, y, int(y * y % P == v)
    raise ValueError(op)


@functools.lru_cache(maxsize=None)
def cases():
    t = table()
    return t, [ref(*item) for item in t]


def run(fn, t):
    """fn(n, ops, a, b, out, flag) -> [(integer the out limbs spell, flag)]"""
    n = len(t)
    fq_in = (RR_FROM_FQ, RR_ROUND, RR_SQRT)
    fq_out = (RR_TO_FQ, RR_ROUND, RR_SQRT)
    a = [w for op, x, _ in t for w in (words32(x) if op in fq_in else limbs30(x))]
    b = [w for op, _, y in t for w in limbs30(y)]
    out, flag = (ctypes.c_uint32 * (NL * n))(), (ctypes.c_uint32 * n)()
    rc = fn(n, D.u32([x[0] for x in t]), D.u32(a), D.u32(b), out, flag)
    assert rc == 0, "harness status %d" % rc
    o = list(out)
    got = []
    for i, (op, _, _) in enumerate(t):
        ws = o[NL * i:NL * (i + 1)]
        got.append((val32(ws) if op in fq_out else val30(ws), ws, flag[i]))
    return got


def check(t, want, got):
    """Exact integers where the reference gives one, residues for the square root; the bounds of
    DESIGN.md: operands < 16p -> result < 1.5p on limbs < 2^30; an Fq coming out < 2p."""
    bad = []
    for (op, a, b), (wi, wr, wf), (g, ws, f) in zip(t, want, got):
        ok = f == wf
        if wi is not None:
            ok = ok and g == wi
        if wr is not None:
            ok = ok and D.from_m(g) == wr and g < 2 * P
        if op in (RR_MUL, RR_SQR, RR_FROM_FQ) and a < 16 * P and b < 16 * P:
            ok = ok and 2 * g < 3 * P and all(w < 1 << W for w in ws)
        if op in (RR_TO_FQ, RR_ROUND):
            ok = ok and g < 2 * P
        if op == RR_ROUND:
            ok = ok and g % P == a % P
        if op in (RR_MUL, RR_SQR):
            ok = ok and g % P == a * (a if op == RR_SQR else b) * pow(RP, -1, P) % P
        if not ok:
            bad.append((OP_NAMES[op], hex(a), hex(b), hex(g), f, wf))
    return bad


# --------------------------------------------------------------------------------------- decode
def _torsion_point(rng, prime):
    from test_native_arith import _small_component
    return _small_component(rng, 1, prime, B.H1)


@functools.lru_cache(maxsize=None)
def decode_cases():
    """[(tag, 48 bytes)]: what k_rlc_decode's g1_decompress(.., false) meets -- valid points of both
    y signs, x >= p, an x whose x^3 + 4 is a non-residue, a cleared compression flag, a valid and
    an invalid infinity encoding, (0, +-2) of order 3, a point of every prime order dividing the
    cofactor h1 and an on-curve point outside G1 (accepted here: the subgroup test follows)."""
    rng = random.Random(0xDEC)
    out = []
    for i in range(6):
        pt = B.g1_mul(B.G1_GEN, rng.randrange(1, B.R))
        out.append(("valid %d" % i, B.g1_compress(pt)))
        out.append(("valid %d negated" % i, B.g1_compress(B.g1_neg(pt))))
    big = bytearray((P + 5).to_bytes(48, "big"))
    big[0] |= 0x80
    out.append(("x >= p", bytes(big)))
    eq = bytearray(P.to_bytes(48, "big"))
    eq[0] |= 0x80
    out.append(("x = p", bytes(eq)))
    while True:
        x = rng.randrange(P)
        if B.fq_sqrt((x * x * x + 4) % P) is None:
            break
    nr = bytearray(x.to_bytes(48, "big"))
    nr[0] |= 0x80
    out.append(("non-residue", bytes(nr)))
    ok = bytearray(B.g1_compress(B.G1_GEN))
    ok[0] &= 0x7F
    out.append(("flag cleared", bytes(ok)))
    out.append(("infinity", B.g1_compress(None)))
    inf = bytearray(B.g1_compress(None))
    inf[47] = 1
    out.append(("infinity with a set bit", bytes(inf)))
    out.append(("(0, 2)", B.g1_compress((0, 2))))
    out.append(("(0, -2)", B.g1_compress((0, P - 2))))
    primes = [3, 11, 10177, 859267, 52437899]
    assert B.H1 == 3 * (11 * 10177 * 859267 * 52437899) ** 2
    for prime in primes:
        out.append(("order %d" % prime, B.g1_compress(_torsion_point(rng, prime))))
    while True:
        pt = B.g1_point_from_x(rng.randrange(P), False)
        if pt and not B.g1_in_subgroup(pt):
            break
    out.append(("outside G1", B.g1_compress(pt)))
    return out


def decode_ref(data):
    """(ok, inf, x, y) of g1_decompress(data, check_subgroup=False) by the oracle"""
    try:
        pt = B.g1_decompress(data, check_subgroup=False)
    except B.DecodeError:
        return (0, None, None, None)
    if pt is None:
        return (1, 1, 0, 0)
    return (1, 0, pt[0], pt[1])


def run_decode(fn, rr):
    cs = decode_cases()
    n = len(cs)
    out, flags = (ctypes.c_uint32 * (24 * n))(), (ctypes.c_uint32 * n)()
    rc = fn(n, rr, b"".join(c for _, c in cs), out, flags)
    assert rc == 0, "harness status %d" % rc
    v = D.ints(out)
    return [(flags[i] & 1, (flags[i] >> 1) & 1, v[2 * i], v[2 * i + 1]) for i in range(n)]


def check_decode(got):
    bad = []
    for (tag, data), (ok, inf, x, y) in zip(decode_cases(), got):
        wok, winf, wx, wy = decode_ref(data)
        if ok != wok or (ok and (inf != winf or (not inf and (x >= P or y >= P or (D.from_m(x), D.from_m(y)) != (wx, wy))))):
            bad.append(tag)
    return bad
