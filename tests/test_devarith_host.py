"""The Fq, lazy-accumulator and GT case tables of tests/devarith_cases.py run through the HOST
fallback of the kernel headers (tests/native/libhbtc_hosttest.so: CIOS product, the C++ fq_acc_*,
fq_mul2 as mul + mul + add, the lane simulator for gt6.h) and compared with the Python-integer
reference.  This proves the tables and the reference right without a GPU (and that every input
respects the documented preconditions: the reference asserts them), and covers the fallback at
the edge operands.  tests/test_gpu_devarith.py runs the same tables on the device."""
import ctypes
import os
import subprocess

import pytest

import devarith_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_hosttest.so")
HDRS = ("field.h", "curve.h", "pairing.h", "pair.h", "bls_constants.h", "gt6.h", "fq_fips.h")


@pytest.fixture(scope="module")
def ht():
    srcs = [os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in HDRS]
    srcs += [os.path.join(ROOT, "tests", "native", f) for f in ("gt_sim.cpp", "hbtc_hosttest.cpp")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-s", "-C", ROOT, "hosttest"])
    return ctypes.CDLL(LIB)


def test_reference_constants():
    """The reference's own constants against field.h's documented bounds."""
    assert 4 * C.P < C.R and C.K24 == 24 * C.P ** 2
    assert 12 * (C.TWO_P - 1) ** 2 < 48 * C.P ** 2
    top = C.TWO_P - 1
    assert C.mont(2 * top * top) < C.TWO_P                      # mont_mul2 of maximal operands
    assert C.mont(48 * C.P ** 2 - 1) < 6 * C.P                  # a maximal accumulator: < 6p
    assert C.redc(48 * C.P ** 2 - 1) < C.TWO_P
    assert len(C.E) >= 50 and sum(1 for x in C.E_RANDOM if x >= C.P) >= 3


def test_fq_table_on_host_fallback(ht):
    table, want = C.fq_cases()
    got = C.run_fq(ht.ht_fq_op, table)
    bad = C.check_fq(table, want, got, mul2_exact=False)
    assert not bad, (len(bad), bad[:5])


def test_accumulator_table_on_host_fallback(ht):
    table, want = C.acc_cases()
    bad = []
    for fn, sel in ((ht.ht_acc_op, lambda m: m != C.ACC_KARA), (ht.ht_acc_kara, lambda m: m == C.ACC_KARA)):
        idx = [i for i, t in enumerate(table) if sel(t[0])]
        part = [table[i] for i in idx]
        bad += C.check_acc(part, [want[i] for i in idx], C.run_acc(fn, part))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("rep", [1, 3])
def test_gt_table_on_lane_simulator(ht, rep):
    table, want = C.gt_cases()
    a, b = C.gt_arrays(table)
    out = C.out_words(144 * len(table))
    assert ht.ht_gt_op_raw(len(table), rep, C.u32([t[0] for t in table]), a, b, out) == 0
    vals = C.ints(out)
    got = [[(vals[12 * i + 2 * k], vals[12 * i + 2 * k + 1]) for k in range(6)]
           for i in range(len(table))]
    bad = C.check_gt(table, want, got)
    assert not bad, bad
