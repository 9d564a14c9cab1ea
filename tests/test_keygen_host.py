"""keygen.h (the arithmetic of hbtc_keygen.hip's kernels: the column sum, the Fr interpolation at
0, the commitment evaluation by Horner, the shared-inversion affine conversion) compiled for the
HOST, its workgroups replayed lane by lane, and checked against Python integers and the Python
oracle.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_keygen_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_keygen_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f)
    for f in ("keygen.h", "enc.h", "hash_hd.h", "field.h", "curve.h", "bls_constants.h")]

R = B.R
INF = bytes([0xC0]) + bytes(47)
EDGE_VALUES = [0, R - 1, R, (1 << 256) - 1]


@pytest.fixture(scope="module")
def kh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_keygen_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    lib.kh_block_size.restype = lib.kh_segment_len.restype = ctypes.c_uint32
    return lib


def buf(n):
    return ctypes.create_string_buffer(max(n, 1))


def u32s(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def lagrange_at_zero(items):
    """Poly::interpolate(items).evaluate(0) in Python integers."""
    acc = 0
    for x, y in items:
        num = den = 1
        for x0, _ in items:
            if x0 != x:
                num = num * x0 % R
                den = den * (x0 - x) % R
        acc = (acc + y * num * pow(den, R - 2, R)) % R
    return acc


def interp(kh, xs, ys):
    out = buf(32)
    dup = kh.kh_interp(len(xs), u32s(xs), b"".join(int(y).to_bytes(32, "little") for y in ys), out)
    return dup, int.from_bytes(out.raw[:32], "little")


def abscissae(m, kind, rng):
    if kind == "dense":
        return list(range(1, m + 1))
    base = [2, 5, 9] if kind == "gapped" else [70000, (1 << 32) - 1, 3]
    xs = list(base[:m])
    while len(xs) < m:  # the named abscissae first, then distinct fillers of the same kind
        x = xs[-1] + rng.randrange(1, 7) if kind == "gapped" else rng.randrange(1, 1 << 32)
        if x not in xs and x < (1 << 32):
            xs.append(x)
    return xs


@pytest.mark.parametrize("m", [0, 1, 2, 255, 256, 257, 300])
def test_interpolation_at_zero(kh, m):
    """Counts around the 256 lanes of the workgroup (a lane holds a second item from 257 on), the
    three kinds of abscissae, and the edge values taken mod r."""
    assert kh.kh_block_size() == 256
    rng = random.Random(100 + m)
    for kind in ("dense", "gapped", "sparse"):
        xs = abscissae(m, kind, rng)
        ys = [EDGE_VALUES[i % 4] if i < 8 or rng.random() < 0.2 else rng.randrange(1 << 256) for i in range(m)]
        dup, got = interp(kh, xs, ys)
        assert dup == 0, (m, kind)
        assert got == lagrange_at_zero([(x, y % R) for x, y in zip(xs, ys)]), (m, kind)


def test_interpolation_small_sets(kh):
    """The named sets as they are, every edge value in every position of {2, 5, 9}."""
    for xs in ([2, 5, 9], [70000, (1 << 32) - 1, 3], [9, 2, 5]):
        for k in range(4):
            ys = [EDGE_VALUES[(k + i) % 4] for i in range(3)]
            dup, got = interp(kh, xs, ys)
            assert dup == 0 and got == lagrange_at_zero([(x, y % R) for x, y in zip(xs, ys)]), (xs, k)
    assert interp(kh, [], []) == (0, 0)
    assert interp(kh, [7], [R + 5]) == (0, 5)  # one point: the constant polynomial


def test_duplicate_x_is_flagged(kh):
    assert interp(kh, [4, 9, 4], [1, 2, 3])[0] == 1
    assert interp(kh, [3, 3], [1, 1])[0] == 1
    xs = list(range(1, 301))
    xs[299] = 44  # the repeat sits on a lane's second item
    assert interp(kh, xs, [1] * 300)[0] == 1
    assert interp(kh, list(range(1, 301)), [1] * 300)[0] == 0


# ---------------------------------------------------------------------------------------- points
def evaluate(kh, commit, xs):
    out = buf(48 * len(xs))
    assert kh.kh_eval(len(commit), b"".join(commit), len(xs), u32s(xs), out) == 0
    return [out.raw[48 * k:48 * k + 48] for k in range(len(xs))]


def horner_oracle(points, x):
    acc = None
    for c in reversed(points):
        acc = B.g1_add(B.g1_mul(acc, x), c)
    return B.g1_compress(acc)


XS = [1, 2, 255, 256, 257, (1 << 32) - 1]


@pytest.mark.parametrize("t1", [1, 2, 3])
def test_horner_against_the_oracle(kh, t1):
    rng = random.Random(200 + t1)
    pts = [B.g1_mul(B.G1_GEN, rng.randrange(1, R)) for _ in range(t1)]
    got = evaluate(kh, [B.g1_compress(p) for p in pts], XS)
    for x, g in zip(XS, got):
        assert g == horner_oracle(pts, x), (t1, x)


def test_horner_doubling_and_cancellation(kh):
    rng = random.Random(210)
    c = B.g1_mul(B.G1_GEN, rng.randrange(1, R))
    cb, nb = B.g1_compress(c), B.g1_compress(B.g1_neg(c))
    assert evaluate(kh, [cb, cb], [1]) == [B.g1_compress(B.g1_mul(c, 2))]
    assert evaluate(kh, [cb, nb], [1]) == [INF]
    # the cancellation in the middle of a longer chain: (C - C) x + C = C
    assert evaluate(kh, [cb, cb, nb], [1]) == [cb]


@pytest.mark.parametrize("pos", [0, 1, 2])
def test_horner_infinity_coefficient(kh, pos):
    rng = random.Random(220 + pos)
    pts = [B.g1_mul(B.G1_GEN, rng.randrange(1, R)) for _ in range(3)]
    pts[pos] = None
    got = evaluate(kh, [B.g1_compress(p) for p in pts], [1, 2, 257])
    assert got == [horner_oracle(pts, x) for x in (1, 2, 257)]
    assert evaluate(kh, [INF, INF, INF], [3]) == [INF]


def test_horner_across_segments(kh):
    """A commitment longer than one segment and one that ends on a segment boundary, from known
    scalars: the evaluation is [sum_j c_j x^j] G."""
    seg = kh.kh_segment_len()
    rng = random.Random(230)
    for t1 in (seg, seg + 1, 2 * seg + 1):
        cs = [rng.randrange(R) for _ in range(t1)]
        cs[seg - 1] = 0  # an infinity coefficient at the end of the first segment
        commit = [B.g1_compress(B.g1_mul(B.G1_GEN, c)) for c in cs]
        xs = [1, 3, 1000, (1 << 32) - 1]
        got = evaluate(kh, commit, xs)
        for x, g in zip(xs, got):
            want = sum(c * pow(x, j, R) for j, c in enumerate(cs)) % R
            assert g == B.g1_compress(B.g1_mul(B.G1_GEN, want)), (t1, x)


def colsum(kh, rows):
    t1 = len(rows[0])
    out = buf(48 * t1)
    assert kh.kh_colsum(len(rows), t1, b"".join(p for r in rows for p in r), out) == 0
    return [out.raw[48 * j:48 * j + 48] for j in range(t1)]


def test_column_sum_edge_cases(kh):
    rng = random.Random(240)
    p = B.g1_mul(B.G1_GEN, rng.randrange(1, R))
    pb, nb = B.g1_compress(p), B.g1_compress(B.g1_neg(p))
    # the four cases as the four columns of two Parts: [P, P], [P, -P], [O, P], [O, O]
    got = colsum(kh, [[pb, pb, INF, INF], [pb, nb, pb, INF]])
    assert got == [B.g1_compress(B.g1_mul(p, 2)), INF, pb, INF]


def test_column_sum_many_parts(kh):
    """More Parts than the 64 lanes of a column: lanes add a second point, then the tree."""
    rng = random.Random(250)
    ks = [[rng.randrange(R) for _ in range(2)] for _ in range(70)]
    base = [B.g1_mul(B.G1_GEN, k) for k in range(1, 5)]
    # points from a small pool of multiples (the oracle's products are slow): scalar = 1 + k mod 4
    rows = [[B.g1_compress(base[k % 4]) for k in r] for r in ks]
    got = colsum(kh, rows)
    for j in range(2):
        want = sum(1 + r[j] % 4 for r in ks) % R
        assert got[j] == B.g1_compress(B.g1_mul(B.G1_GEN, want))


def test_bad_point_is_refused(kh):
    bad = bytes([0x17]) + B.g1_compress(B.G1_GEN)[1:]  # no compression flag
    assert kh.kh_colsum(1, 1, bad, buf(48)) == -1
    assert kh.kh_eval(1, bad, 1, u32s([1]), buf(48)) == -1
