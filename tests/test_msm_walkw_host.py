"""The G1 bucket walk on the redundant 13 x 30 form (msm_walk.h over curve.h's JacW, as hbtc_msm.hip's
k_msm_buckets<Fq> runs it) compiled for the HOST under HBTC_RR_ASSERT: one wave of up to 64 lane states
in lockstep, both bounds of every FqW asserted at every operation (a violated bound aborts the process).

Every lane's result, after jacw_to_jac and normalisation, is compared inside the harness with the
12 x 32 walk over the same sorted list, and every window's sum here with [sum d_i a_i] G from the Python
oracle.  tools/rr_bounds.py's closure of the walk is run as well.  Slots 1, 2 and 4.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from oracle import bls12_381 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_msmw_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_msmw_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in ("msm_walk.h", "field.h", "curve.h", "fq_rr.h")]

R = B.R
NB = 64  # buckets per window (c = 7)
SLOTS = [1, 2, 4]
INF = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def mh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_msmw_hosttest.so"])
    return ctypes.CDLL(LIB)


def run(mh, digits, scal, S, slots):
    n_win, n = len(digits), len(scal)
    flat = [d for w in digits for d in w]
    lanes = ctypes.create_string_buffer(48 * n_win * S)
    wins = ctypes.create_string_buffer(48 * n_win)
    stats = (ctypes.c_uint32 * 4)()
    rc = mh.mhw_g1(n_win, n, NB, S, slots, (ctypes.c_int16 * len(flat))(*flat), (ctypes.c_uint64 * n)(*scal),
                   lanes, wins, stats)
    assert rc == 0, "mhw_g1 returned %d" % rc
    return ([lanes.raw[48 * i:48 * i + 48] for i in range(n_win * S)],
            [wins.raw[48 * w:48 * w + 48] for w in range(n_win)], list(stats))


def g1(k):
    k %= R
    return B.g1_compress(B.g1_mul(B.G1_GEN, k)) if k else INF


def check(mh, digits, scal, S=8):
    """Every lane equal to the 12 x 32 walk (inside the harness), every window sum equal to the oracle's"""
    out = None
    for slots in SLOTS:
        lanes, wins, stats = run(mh, digits, scal, S, slots)
        assert wins == [g1(sum(d * a for d, a in zip(dw, scal))) for dw in digits], slots
        out = out or (lanes, stats)
    return out


def rand_digits(rng, n):
    return [rng.randrange(-NB, NB + 1) for _ in range(n)]


def test_sixty_four_lanes(mh):
    """8 windows of 8 slices: the wave's 64 lanes, slices of 10 or 11 terms over most ranks"""
    rng = random.Random(1601)
    n = 84
    check(mh, [rand_digits(rng, n) for _ in range(8)], [rng.randrange(1, 1 << 64) for _ in range(n)])


def test_doubling_infinity_and_empty_ranks(mh):
    """One lane per window.  Equal consecutive points in one bucket (the mixed addition's doubling), a
    point and its negation at the head of a bucket (run returns to infinity, then restarts from the next
    term), a rank of one point followed by empty ranks (the same snapshot twice: the full addition's
    doubling), an infinity term, and a window that cancels."""
    check(mh, [[33, -33, 20, 20, 7, 5, 5, 0]], [11, 11, 23, 23, 5, 9, 9, 3], S=1)
    check(mh, [[NB, NB - 2]], [7, 0], S=1)
    check(mh, [[1, -1]], [7, 7], S=1)
    check(mh, [[9, 9, 9, 9]], [5, 5, 5, 5], S=1)  # P + P = 2P, 2P + P, 3P + P


def test_slices_of_one_and_none(mh):
    """Three terms over eight slices: five lanes with an empty slice beside slices of one term; an empty
    window beside them."""
    rng = random.Random(1602)
    scal = [rng.randrange(1, 1 << 64) for _ in range(20)]
    few = [0] * 20
    few[3], few[9], few[17] = 5, -NB, 1
    lanes, _ = check(mh, [few, [0] * 20], scal)
    assert lanes[8:] == [INF] * 8 and lanes[:8].count(INF) == 5
    assert sorted(x for x in lanes[:8] if x != INF) == sorted([g1(5 * scal[3]), g1(-NB * scal[9]), g1(scal[17])])


def test_first_slice_crosses_every_rank(mh):
    """One term in bucket B, the rest in bucket 1: the first slice stores the same run B - 2 times."""
    rng = random.Random(1603)
    n = 84
    scal = [rng.randrange(1, 1 << 64) for _ in range(n)]
    digits = [[NB if i == 40 else 1 for i in range(n)]]
    for slots in SLOTS:
        _, _, stats = run(mh, digits, scal, 8, slots)
        assert stats[1] == (NB - 1 - 1) // slots
    check(mh, digits, scal)


def test_walk_closure_of_the_bounds_interpreter():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import rr_bounds
    finally:
        sys.path.pop(0)
    assert rr_bounds.check_walk_closure()
