"""msm_walk.h (the lane-uniform bucket walk of hbtc_msm.hip's k_msm_buckets) compiled for the HOST:
one wave of up to 64 lane states replayed in lockstep, the wave votes computed in loops.

Group (a), integers modulo 2^61 - 1: every lane's result is compared exactly with
sum_{e in slice} bucket(e) * term(e) from plain arithmetic over the same sort (largest bucket
first, index order inside a bucket, equal slices of the list).
Group (b), curve.h's G1: every lane is compared inside the harness, after normalisation, with the
nested loops of rounds 1-9, and every window's sum here with [sum d_i a_i] G from the Python oracle.
Slots 1, 2 and 4.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_msm_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_msm_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in ("msm_walk.h", "field.h", "curve.h", "bls_constants.h")]

R = B.R
NB = 64  # buckets per window (c = 7)
SLOTS = [1, 2, 4]


@pytest.fixture(scope="module")
def mh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_msm_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    lib.mh_toy_modulus.restype = ctypes.c_uint64
    return lib


def lanes_expected(digits, vals, S, mod):
    """Per lane of one window: sum over its slice of |d| * (+-v), the sort restated."""
    order = sorted((i for i, d in enumerate(digits) if d), key=lambda i: (NB - abs(digits[i]), i))
    total = len(order)
    out = []
    for s in range(S):
        sl = order[total * s // S:total * (s + 1) // S]
        out.append(sum(digits[i] * vals[i] for i in sl) % mod)
    return out, [total * (s + 1) // S - total * s // S for s in range(S)]


def run_toy(mh, digits, vals, S, slots):
    n_win, n = len(digits), len(vals)
    flat = [d for w in digits for d in w]
    out = (ctypes.c_uint64 * (n_win * S))()
    stats = (ctypes.c_uint32 * 4)()
    rc = mh.mh_toy(n_win, n, NB, S, slots, (ctypes.c_int16 * len(flat))(*flat), (ctypes.c_uint64 * n)(*vals),
                   (ctypes.c_uint8 * n)(*[int(v == 0) for v in vals]), out, stats)
    assert rc == 0
    return list(out), list(stats)


def run_g1(mh, digits, scal, S, slots):
    n_win, n = len(digits), len(scal)
    flat = [d for w in digits for d in w]
    out = ctypes.create_string_buffer(48 * n_win)
    stats = (ctypes.c_uint32 * 4)()
    rc = mh.mh_g1(n_win, n, NB, S, slots, (ctypes.c_int16 * len(flat))(*flat), (ctypes.c_uint64 * n)(*scal),
                  out, stats)
    assert rc == 0, "lanes that differ from the nested loops: %d" % rc
    return [out.raw[48 * w:48 * w + 48] for w in range(n_win)], list(stats)


def check(mh, digits, vals, S=8, g1=True):
    """Both groups at every slot count.  vals: the toy residues and, for G1, the scalars a_i of
    the points [a_i] G (0: the identity).  Returns the statistics of the one-slot toy run."""
    mod = mh.mh_toy_modulus()
    first = None
    for slots in SLOTS:
        got, stats = run_toy(mh, digits, vals, S, slots)
        for w, dw in enumerate(digits):
            want, lens = lanes_expected(dw, vals, S, mod)
            assert got[w * S:(w + 1) * S] == want, (slots, w)
        longest = max(max(lanes_expected(dw, vals, S, mod)[1]) for dw in digits)
        assert stats[0] == longest  # the wave runs as many steps as its longest slice, no more
        first = first or stats
        if g1:
            sums, _ = run_g1(mh, digits, vals, S, slots)
            for w, dw in enumerate(digits):
                k = sum(d * a for d, a in zip(dw, vals)) % R
                assert sums[w] == B.g1_compress(B.g1_mul(B.G1_GEN, k) if k else None), (slots, w)
    return first


def rand_digits(rng, n):
    return [rng.randrange(-NB, NB + 1) for _ in range(n)]


def test_random_windows(mh):
    """The C3 shape: 8 windows of 668 terms fill the wave's 64 lanes."""
    rng = random.Random(1001)
    n = 668
    check(mh, [rand_digits(rng, n) for _ in range(8)], [rng.randrange(1, 1 << 64) for _ in range(n)])


def test_empty_and_short_windows(mh):
    rng = random.Random(1002)
    vals = [rng.randrange(1, 1 << 64) for _ in range(20)]
    check(mh, [[0] * 20, [0] * 20], vals)  # total = 0
    few = [0] * 20
    few[3], few[9], few[17] = 5, -NB, 1  # total < S: five lanes with p0 == p1
    check(mh, [few, [0] * 20], vals)


def test_all_terms_in_one_bucket(mh):
    rng = random.Random(1003)
    n = 100
    stats = check(mh, [[17 if i & 1 else -17 for i in range(n)]], [rng.randrange(1, 1 << 64) for _ in range(n)])
    assert stats[1] == 0  # every slice inside one rank: no snapshot, no flush in the loop


def test_first_slice_crosses_every_rank(mh):
    """One term in bucket B, the rest in bucket 1: the first slice leaves B - 1 ranks at one position
    (the same `run` stored again and again, a flush whenever the slots are full)."""
    rng = random.Random(1004)
    n = 84
    vals = [rng.randrange(1, 1 << 64) for _ in range(n)]
    digits = [[NB if i == 40 else 1 for i in range(n)]]
    for slots in SLOTS:
        _, stats = run_toy(mh, digits, vals, 8, slots)
        assert stats[1] == (NB - 1 - 1) // slots  # the last pending snapshots wait for the final flush
    check(mh, digits, vals)


def test_walks_of_0_1_and_84_in_one_wave(mh):
    rng = random.Random(1005)
    n = 672
    vals = [rng.randrange(1, 1 << 64) for _ in range(n)]
    one = [1 + 9 * i if i < 8 else 0 for i in range(n)]
    full = [d or 1 for d in rand_digits(rng, n)]
    check(mh, [[0] * n, one, full], vals)


def test_run_returns_to_the_identity_and_doublings(mh):
    """One lane per window (S = 1).  P then -P at the head of a bucket; the same point twice in one
    bucket (the mixed addition's doubling); a rank of one point followed by an empty rank, so the
    second snapshot equals tot (the full addition's doubling); an identity point as a term."""
    check(mh, [[33, -33, 20, 20, 7, 5, 5, 0]], [11, 11, 23, 23, 5, 9, 9, 3], S=1)
    check(mh, [[NB, NB - 2]], [7, 0], S=1)
    check(mh, [[NB - 2]], [7], S=1)
    check(mh, [[1, -1]], [7, 7], S=1)  # the whole window cancels


def test_bad_requests_are_refused(mh):
    one16, one64, one8 = (ctypes.c_int16 * 1)(NB + 1), (ctypes.c_uint64 * 1)(1), (ctypes.c_uint8 * 1)(0)
    out, stats = (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 4)()
    assert mh.mh_toy(1, 1, NB, 8, 1, one16, one64, one8, out, stats) == -1  # |digit| > B
    assert mh.mh_toy(9, 1, NB, 8, 1, one16, one64, one8, out, stats) == -1  # more than 64 lanes
    assert mh.mh_toy(1, 1, NB, 8, 0, one16, one64, one8, out, stats) == -1  # no slot
