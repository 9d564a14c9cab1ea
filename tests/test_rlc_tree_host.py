"""rlc_tree.h (the body of hbtc_rlc.hip's k_rlc_tree: the DecryptionShare tile sums as a lane-dense
tree over a group of tiles) compiled for the HOST and replayed merge by merge.  Every output of
every tile -- eighths, left quarters, halves, tile, on both sides -- is compared as an affine point
with a plain restatement inside the harness (A = sum q_i, B = sum bitrev_k(i) q_i inside each
group of 2^k), and a sample of them with the Python oracle from the scalars.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_tree_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_tree_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in ("rlc_tree.h", "field.h", "curve.h", "bls_constants.h")]

R = B.R
N_PK = 70
COUNTS = [1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64]
# TileSums as an array of points (hbtc_kernels.h): member -> first entry
TS = dict(S=0, P=9, SW=18, PW=27, SH=36, SHW=38, PH=40, PHW=42, SQ=44, SQW=46, PQ=48, PQW=50)


@pytest.fixture(scope="module")
def th():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_tree_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    lib.th_group_tiles.restype = lib.th_sums_points.restype = ctypes.c_uint32
    assert lib.th_sums_points() == 52
    return lib


def all_of(count):
    return (1 << count) - 1


def masks_of(count):
    """all, none, one lane, alternating, only the last lane"""
    return [all_of(count), 0, 1 << (count // 2), all_of(count) & 0x5555555555555555, 1 << (count - 1)]


def run(th, rng, counts, masks, identity_s=(), reverse=0):
    """One group.  A lane outside the mask carries the identity on both sides (what k_rlc_items
    leaves); the lanes of identity_s (tile, position) carry an identity S beside their P.
    Returns (mismatches, outputs per tile, S scalars per tile, P scalars per tile)."""
    s_scal, idx, qs, qp = [], [], [], []
    p_scal = [rng.randrange(1, 1 << 64) for _ in range(N_PK)]
    for t, (c, m) in enumerate(zip(counts, masks)):
        ts, tp = [0] * 64, [0] * 64
        for i in range(c):
            sender = rng.randrange(N_PK)
            idx.append(sender)
            inside = (m >> i) & 1
            ts[i] = rng.randrange(1, 1 << 64) if inside and (t, i) not in identity_s else 0
            tp[i] = p_scal[sender] if inside else 0
            s_scal.append(ts[i])
        qs.append(ts)
        qp.append(tp)
    n = len(counts)
    out = ctypes.create_string_buffer(n * 52 * 48)
    bad = th.th_run(n, (ctypes.c_uint32 * n)(*counts), (ctypes.c_uint64 * n)(*masks),
                    (ctypes.c_uint64 * len(s_scal))(*s_scal), (ctypes.c_uint32 * len(idx))(*idx), N_PK,
                    (ctypes.c_uint64 * N_PK)(*p_scal), reverse, out)
    pts = [[out.raw[48 * (52 * t + j):48 * (52 * t + j + 1)] for j in range(52)] for t in range(n)]
    return bad, pts, qs, qp


def bitrev(i, k):
    return int(format(i, "0%db" % k)[::-1], 2)


def expect(q, lo, k, weighted):
    """[sum w_i q_i] G for the scalars q of positions [lo, lo + 2^k)"""
    s = sum((bitrev(i, k) if weighted else 1) * q[lo + i] for i in range(1 << k)) % R
    return B.g1_compress(B.g1_mul(B.G1_GEN, s) if s else None)


def oracle_sample(pts, qs, qp):
    """The tile sums, the second half, the last left quarter and the last eighth of one tile against
    the oracle, on both sides."""
    for side, w, q in (("S", "SW", qs), ("P", "PW", qp)):
        assert pts[TS[side] + 8] == expect(q, 0, 6, False)
        assert pts[TS[w] + 8] == expect(q, 0, 6, True)
        assert pts[TS[side] + 7] == expect(q, 56, 3, False)
        assert pts[TS[w] + 7] == expect(q, 56, 3, True)
        assert pts[TS[side + "H"] + 1] == expect(q, 32, 5, False)
        assert pts[TS[side + "HW"] + 1] == expect(q, 32, 5, True)
        assert pts[TS[side + "Q"] + 1] == expect(q, 32, 4, False)
        assert pts[TS[side + "QW"] + 1] == expect(q, 32, 4, True)


@pytest.mark.parametrize("count", COUNTS)
def test_single_tile_counts_and_masks(th, count):
    rng = random.Random(800 + count)
    for k, m in enumerate(masks_of(count)):
        bad, pts, qs, qp = run(th, rng, [count], [m])
        assert bad == 0, (count, hex(m))
        if k == 0:
            oracle_sample(pts[0], qs[0], qp[0])
    # an identity S beside a non-identity P, at the first and the last position; merges backwards
    bad, pts, qs, qp = run(th, rng, [count], [all_of(count)], identity_s={(0, 0), (0, count - 1)}, reverse=1)
    assert bad == 0
    oracle_sample(pts[0], qs[0], qp[0])


def test_weights_are_the_bit_reversed_positions(th):
    """One share alone in a full tile, at every position of a sample: each weighted output is that
    share times the bit-reversed position inside its group."""
    rng = random.Random(811)
    for pos in (0, 1, 2, 5, 8, 17, 31, 32, 47, 62, 63):
        bad, pts, qs, qp = run(th, rng, [64], [1 << pos])
        assert bad == 0, pos
        s = qs[0][pos]
        assert pts[0][TS["SW"] + 8] == expect(qs[0], 0, 6, True)
        w = bitrev(pos, 6)
        assert pts[0][TS["SW"] + 8] == B.g1_compress(B.g1_mul(B.G1_GEN, w * s % R) if w else None), pos
        w8 = bitrev(pos % 8, 3)
        assert pts[0][TS["SW"] + pos // 8] == B.g1_compress(B.g1_mul(B.G1_GEN, w8 * s % R) if w8 else None), pos


def test_groups_of_tiles(th):
    """Groups of G, G - 1 and 1 tiles with mixed counts and masks: a ragged tile's missing positions
    are the next tile's slots and must stay untouched."""
    G = th.th_group_tiles()
    rng = random.Random(820)
    for n in sorted({G, max(G - 1, 1), 1}):
        counts = [COUNTS[(7 * t + n) % len(COUNTS)] for t in range(n)]
        masks = [all_of(c) if t % 3 == 0 else rng.getrandbits(64) & all_of(c) for t, c in enumerate(counts)]
        for reverse in (0, 1):
            bad, pts, qs, qp = run(th, rng, counts, masks, reverse=reverse)
            assert bad == 0, (n, reverse)
        oracle_sample(pts[n - 1], qs[n - 1], qp[n - 1])


def test_bad_requests_are_refused(th):
    one = (ctypes.c_uint64 * 1)(0)
    idx = (ctypes.c_uint32 * 1)(0)
    out = ctypes.create_string_buffer(52 * 48)
    G = th.th_group_tiles()
    assert th.th_run(1, (ctypes.c_uint32 * 1)(65), one, one, idx, 1, one, 0, out) == -1
    assert th.th_run(1, (ctypes.c_uint32 * 1)(3), (ctypes.c_uint64 * 1)(8), one, idx, 1, one, 0, out) == -1
    assert th.th_run(G + 1, (ctypes.c_uint32 * (G + 1))(), one, one, idx, 1, one, 0, out) == -1
