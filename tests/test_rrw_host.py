"""The redundant 13 x 30 form (field.h FqW, curve.h jacw_*) compiled for the HOST with HBTC_RR_ASSERT:
every value carries its per-limb and value bounds and every operation asserts them (an abort fails
the test), every MAD is checked for a carry-out.  Against Python integers and oracle/bls12_381.py:
add, sub, neg, dbl and normalise on operands at the limb and value bounds; the zero test on every
multiple of p up to the value bound, in canonical and borrowed spellings, and on +-1 beside each; the
three point formulas with their special cases; [|x|] P and the subgroup verdict on G1 points,
torsion points of every prime order dividing the cofactor, composite order, P + T and a point outside
G1.  Runs without a GPU."""
import ctypes
import os
import struct
import subprocess

import pytest

import rrw_cases as C
from oracle import bls12_381 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_rrw_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", f) for f in ("hbtc_rrw_hosttest.cpp", "hbtc_rrw_ops.h")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in ("fq_rr.h", "curve.h", "field.h", "bls_constants.h")]


@pytest.fixture(scope="module")
def rh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_rrw_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    lib.rrw_subgroup.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_the_cases_reach_every_branch():
    """The integer walk of [|x|] q for the bits of |x| = 0xd201000000010000."""
    cs = dict(C.subgroup_cases())
    acc, n = C.walk(cs["(0, 2)"])
    assert n == dict(dbl_inf=12, add_inf=3, eq=1, neg=2)
    assert acc == B.g1_neg(cs["(0, 2)"])          # t1 = -P: the second chain sees the same on a Jacobian base
    assert C.walk(cs["order 11"])[1]["eq"] == 1
    for prime in (11, 10177, 859267):
        assert C.X_ABS % prime == prime - 1
    _, g = C.walk(cs["G1 0"])
    assert g == dict(dbl_inf=1, add_inf=1, eq=0, neg=0)


def test_field_operations_against_python_integers(rh):
    table, want, _ = C.cases()
    assert C.check_fields(table, want, C.run(rh.rrw_ops, table)) == []


def test_point_formulas_against_the_oracle(rh):
    _, _, table = C.cases()
    got = C.run(rh.rrw_ops, [(op, ins) for op, ins, _, _ in table])
    assert C.check_points(table, got) == []


def test_x_chains_and_subgroup_verdict(rh):
    got = C.run_subgroup(rh.rrw_subgroup)
    assert C.check_subgroup(got) == []
    verdicts = [(f >> 2) & 1 for f, _, _ in got]
    assert verdicts == [1] * 6 + [0] * (len(got) - 6)


def test_the_same_table_under_asan_and_ubsan(rh, tmp_path):
    """`make sanitize-rrw` with the table: the stand-alone program's every output equals the library's."""
    ft, _, pt = C.cases()
    items = list(ft) + [(op, ins) for op, ins, _, _ in pt]
    enc = [B.g1_compress(p) for _, p in C.subgroup_cases()]
    path = tmp_path / "table.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for op, ins in items:
            ins = list(ins) + [C.Z13] * (6 - len(ins))
            f.write(struct.pack("<79I", op, *[w for s in ins for w in s]))
        f.write(struct.pack("<I", len(enc)))
        f.write(b"".join(enc))
    out = subprocess.run(["make", "-s", "-C", ROOT, "sanitize-rrw", "RRW_TABLE=%s" % path], check=True,
                         capture_output=True, text=True).stdout
    lines = [[int(x) for x in ln.split()] for ln in out.strip().splitlines()]
    assert len(lines) == len(items) + len(enc)
    got = C.run(rh.rrw_ops, items)
    for ln, (outs, flag) in zip(lines, got):
        assert ln == [flag] + [w for o in outs for w in o]
    n = len(enc)
    so, sf = (ctypes.c_uint32 * (72 * n))(), (ctypes.c_uint32 * n)()
    assert rh.rrw_subgroup(n, b"".join(enc), so, sf) == 0
    for i, ln in enumerate(lines[len(items):]):
        assert ln == [sf[i]] + list(so)[72 * i:72 * (i + 1)]
