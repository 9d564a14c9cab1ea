"""The item pass's x-adic multiplication on the redundant 13 x 30 form (curve.h xadic_mul_sac8_w: the
packed co-Z table chain, the column of jacw_dbl + jacw_madd_generic, the even-d0 correction, the
exit) compiled for the HOST with HBTC_RR_ASSERT: every FqW carries its per-limb and value bounds and
every operation asserts them (an abort fails the test), everything that is packed is asserted to be a
product result below 1.5p, every MAD is checked for a carry-out.  [d0 + d1 x + d2 mu + d3 mu x] P
against oracle/bls12_381.py and against xadic_mul_sac8<Fq, true> on the same inputs, on the LDS-layout
buffer at lanes 5 and 63, for digits of 16 and 32 bits, base points of both y signs, the edge digit
vectors (all zero, d0 = 1 alone, d0 even, d0 = 0, all ones, all bits set, the top bit of every digit)
and 200 random ones; pack -> unpack round trips.  Runs without a GPU."""
import ctypes
import os
import struct
import subprocess

import pytest

import xadicw_cases as C
from oracle import bls12_381 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_xadicw_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", f) for f in ("hbtc_xadicw_hosttest.cpp", "hbtc_xadicw_ops.h")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in ("fq_rr.h", "curve.h", "field.h", "bls_constants.h")]


@pytest.fixture(scope="module")
def xh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_xadicw_hosttest.so"])
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def got(xh):
    return C.run(xh.xadicw_mul, C.table())


def test_the_table_holds_the_cases():
    t = C.table()
    assert len(t) == 2 * 2 * 2 * 7 + 200
    assert {(nb, lane) for _, _, nb, lane in t} == {(16, 5), (16, 63), (32, 5), (32, 63)}
    assert len({B.g1_compress(p)[0] & 0x20 for p in C.base_points()}) == 2
    for nbits in (16, 32):
        ds = [d for _, d, nb, _ in t[:56] if nb == nbits]
        assert (0, 0, 0, 0) in ds and (1, 0, 0, 0) in ds and (1, 1, 1, 1) in ds
        assert any(d[0] and d[0] % 2 == 0 for d in ds) and any(d[0] == 0 and all(d[1:]) for d in ds)
        assert (1 << (nbits - 1),) * 4 in ds and ((1 << nbits) - 1,) * 4 in ds


def test_results_equal_the_oracle(got):
    bad = [(i, it[1:]) for i, (it, (f, o), want) in enumerate(zip(C.table(), got, C.expected()))
           if not f & 1 or C.g1j(o[:36]) != want]
    assert bad == []
    # compressed, as the library's callers see a point
    for (f, o), want in list(zip(got, C.expected()))[:8]:
        pt = C.g1j(o[:36])
        assert (B.g1_compress(pt) if pt else None) == (B.g1_compress(want) if want else None)


def test_results_equal_the_12x32_form(got):
    assert [i for i, (f, o) in enumerate(got) if f != 3 or C.g1j(o[:36]) != C.g1j(o[36:])] == []


def test_the_zero_scalar_is_infinity_with_z_zero(got):
    zeros = [i for i, (_, d, _, _) in enumerate(C.table()) if not any(d)]
    assert len(zeros) == 8
    for i in zeros:
        assert got[i][1][24:36] == [0] * 12


def test_pack_unpack_round_trips(xh):
    for v, (packed, limbs) in zip(C.PACK_VALUES, C.run_pack(xh.xadicw_pack)):
        assert packed == v and limbs == C.spell(v)


def test_the_same_table_under_asan_and_ubsan(xh, got, tmp_path):
    """`make sanitize-xadicw` with the table: the stand-alone program's every output equals the library's."""
    t = C.table()
    path = tmp_path / "table.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(t)))
        f.write(struct.pack("<%dI" % (C.ITEM_WORDS * len(t)), *C.words(t)))
        f.write(struct.pack("<I", len(C.PACK_VALUES)))
        for v in C.PACK_VALUES:
            f.write(struct.pack("<13I", *C.spell(v)))
    out = subprocess.run(["make", "-s", "-C", ROOT, "sanitize-xadicw", "XADICW_TABLE=%s" % path], check=True,
                         capture_output=True, text=True).stdout
    lines = [[int(x) for x in ln.split()] for ln in out.strip().splitlines()]
    assert len(lines) == len(t) + len(C.PACK_VALUES)
    assert [(ln[0], ln[1:]) for ln in lines[:len(t)]] == got
    packs = C.run_pack(xh.xadicw_pack)
    for ln, (packed, limbs) in zip(lines[len(t):], packs):
        assert sum(w << (32 * k) for k, w in enumerate(ln[:12])) == packed and ln[12:] == limbs
