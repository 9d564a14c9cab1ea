"""The 13 x 30 Fq code on gfx950 (fq_rr.h's inline-asm product and squaring under field.h FqR): the
operand table and the decode cases of tests/test_rr_host.py, one item per lane on 64-lane
workgroups (tests/native/hbtc_rr_devtest.hip, built with the flags of the k_rlc_decode object).
Products and conversions are compared as exact integers with Python, square roots and decoded
points as canonical residues with oracle/bls12_381.py: representatives may differ from the
12 x 32 chain's."""
import ctypes
import os
import subprocess

import pytest

import rr_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_rr_devtest.so")


@pytest.fixture(scope="module")
def rd():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_rr_devtest.so"])
    lib = ctypes.CDLL(LIB)
    lib.rd_decode_g1.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.rd_devices() >= 1
    return lib


def test_operations_against_python_integers(rd):
    table, want = C.cases()
    assert len(table) % 64 != 0 and len(table) > 64   # a partial last workgroup
    assert C.check(table, want, C.run(rd.rd_ops, table)) == []


def test_g1_decode_with_the_30_bit_square_root(rd):
    got = C.run_decode(rd.rd_decode_g1, 1)
    assert C.check_decode(got) == []
    assert got == C.run_decode(rd.rd_decode_g1, 0)   # the same bytes as the 12 x 32 chain
