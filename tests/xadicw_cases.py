"""Case table and integer reference of the item pass's x-adic multiplication on the redundant 13 x 30
form (curve.h xadic_mul_sac8_w), shared by tests/test_xadicw_host.py (host build, every bound
asserted) and tests/test_gpu_xadicw.py (gfx950).  An item is a base point P in G1, four digits below
2^nbits (nbits 16 or 32: the 64- and 128-bit scalars) and the lane whose column of the LDS-layout
buffer it uses; the result is [d0 + d1 x + d2 mu + d3 mu x] P with x the BLS parameter and mu = -x^2."""
import ctypes
import functools
import random

from oracle import bls12_381 as B
import devarith_cases as D

P = B.P
X = -0xd201000000010000
MU = -X * X
ITEM_WORDS, OUT_WORDS = 18, 72
W, NL = 30, 13


def scalar(d):
    return (d[0] + d[1] * X + d[2] * MU + d[3] * MU * X) % B.R


@functools.lru_cache(maxsize=None)
def base_points():
    """two G1 points whose compressed encodings carry different y signs"""
    rng = random.Random(0x7C)
    while True:
        p = B.g1_mul(B.G1_GEN, rng.randrange(1, B.R))
        q = B.g1_neg(p)
        if {B.g1_compress(p)[0] & 0x20, B.g1_compress(q)[0] & 0x20} == {0, 0x20}:
            return [p, q]


def digit_vectors(nbits, rng, n_random):
    top, full = 1 << (nbits - 1), (1 << nbits) - 1
    r = lambda: rng.randrange(1 << nbits)
    vs = [(0, 0, 0, 0), (1, 0, 0, 0), (2 * (r() // 2) or 2, r(), r(), r()), (0, r() | 1, r() | 1, r() | 1),
          (1, 1, 1, 1), (full, full, full, full), (top, top, top, top)]
    return vs + [(r(), r(), r(), r()) for _ in range(n_random)]


@functools.lru_cache(maxsize=None)
def table(n_random=200, lanes=(5, 63)):
    """[(point, digits, nbits, lane)]: every edge vector for both points, both digit sizes and both lanes;
    the random vectors spread over them"""
    rng = random.Random(0x7D)
    t = []
    for nbits in (16, 32):
        vs = digit_vectors(nbits, rng, 0)
        for pt in base_points():
            for lane in lanes:
                t += [(pt, d, nbits, lane) for d in vs]
    for i in range(n_random):
        nbits = (16, 32)[i & 1]
        d = tuple(rng.randrange(1 << nbits) for _ in range(4))
        t.append((base_points()[(i >> 1) & 1], d, nbits, lanes[(i >> 2) & 1]))
    return t


def words(items):
    flat = []
    for pt, d, nbits, lane in items:
        c = B.g1_compress(pt)
        flat += [int.from_bytes(c[4 * k:4 * k + 4], "little") for k in range(12)] + list(d) + [nbits, lane]
    return flat


def g1j(ws):
    """36 words of a 12 x 32 Montgomery G1J -> affine point or None"""
    x, y, z = [D.from_m(sum(w << (32 * k) for k, w in enumerate(ws[12 * c:12 * c + 12]))) for c in range(3)]
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def run(fn, items):
    """fn(n, items, out, flags) -> [(flags, the 72 output words)]"""
    n = len(items)
    out, flags = (ctypes.c_uint32 * (OUT_WORDS * n))(), (ctypes.c_uint32 * n)()
    rc = fn(n, D.u32(words(items)), out, flags)
    assert rc == 0, "harness status %d" % rc
    o = list(out)
    return [(flags[i], o[OUT_WORDS * i:OUT_WORDS * (i + 1)]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def expected():
    return [B.g1_mul(pt, scalar(d)) if scalar(d) else None for pt, d, _, _ in table()]


def spell(v):
    return [(v >> (W * i)) & ((1 << W) - 1) for i in range(NL)]


# 3p is odd: (3p) // 2 is the largest integer below 1.5p, the bound of everything that is packed
PACK_VALUES = [0, 1, P - 1, (3 * P) // 2 - 1, (3 * P) // 2, P, (1 << 360) - 1]


def run_pack(fn):
    """-> [(packed integer, unpacked limbs)] of PACK_VALUES"""
    n = len(PACK_VALUES)
    out = (ctypes.c_uint32 * (25 * n))()
    rc = fn(n, D.u32([w for v in PACK_VALUES for w in spell(v)]), out)
    assert rc == 0, "harness status %d" % rc
    o = list(out)
    return [(sum(w << (32 * k) for k, w in enumerate(o[25 * i:25 * i + 12])), o[25 * i + 12:25 * i + 25])
            for i in range(n)]
