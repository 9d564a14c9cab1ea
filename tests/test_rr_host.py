"""The 13 x 30 Fq code (field.h FqR over fq_rr.h) compiled for the HOST, every MAD checked for a
carry-out, against Python integers: conversion round trips, product and squaring on
tests/devarith_cases.py's Fq operands plus 16p - 1 and all-limbs-maximal, the square root on
residues and non-residues, and k_rlc_decode's G1 decode with its square root on 30-bit limbs
against oracle/bls12_381.py.  Runs without a GPU."""
import ctypes
import os
import subprocess

import pytest

import rr_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_rr_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", f) for f in ("hbtc_rr_hosttest.cpp", "hbtc_rr_ops.h")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in ("fq_rr.h", "curve.h", "field.h", "bls_constants.h")]


@pytest.fixture(scope="module")
def rh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_rr_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    lib.rr_decode_g1.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_operations_against_python_integers(rh):
    table, want = C.cases()
    assert C.check(table, want, C.run(rh.rr_ops, table)) == []


def test_reference_bounds():
    """The reference itself: operands < 16p give a product < 1.5p; the conversions' constants."""
    assert 16 * C.P * 16 * C.P + (C.RP - 1) * C.P < 3 * C.P * C.RP // 2
    assert C.mont30((C.D.M) * C.K_IN) % C.P == C.RP % C.P        # one: R -> R'
    assert C.mont30((C.RP % C.P) * C.K_OUT) % C.P == C.D.M


def test_g1_decode_with_the_30_bit_square_root(rh):
    got = C.run_decode(rh.rr_decode_g1, 1)
    assert C.check_decode(got) == []
    assert got == C.run_decode(rh.rr_decode_g1, 0)   # the same bytes as the 12 x 32 chain
