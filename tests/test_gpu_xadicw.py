"""The item pass's x-adic multiplication on the redundant 13 x 30 form on gfx950 (curve.h
xadic_mul_sac8_w over fq_rr.h's relaxed-bound inline-asm blocks): the table of tests/test_xadicw_host.py,
one item per lane on 64-lane workgroups with the table's three LDS entries in the workgroup's own LDS,
laid out as k_rlc_items has them (tests/native/hbtc_xadicw_devtest.hip, built with the flags of the
k_rlc_items object).  The G1J words must equal the host build's of the same code bit for bit (the plain
C++ schedule with every bound asserted, run at the lane the device ran the item at); the points are also
checked against oracle/bls12_381.py directly."""
import ctypes
import os
import subprocess

import pytest

import xadicw_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "tests", "native", "libhbtc_xadicw_devtest.so")
HOST = os.path.join(ROOT, "tests", "native", "libhbtc_xadicw_hosttest.so")


@pytest.fixture(scope="module")
def libs():
    for path in (DEV, HOST):
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", ROOT, os.path.relpath(path, ROOT)])
    dev, host = ctypes.CDLL(DEV), ctypes.CDLL(HOST)
    assert dev.xwd_devices() >= 1
    return dev, host


def test_g1j_words_equal_the_host_build(libs):
    dev, host = libs
    # the device runs item i at lane i % 64: the host build gets the same lane
    table, want = C.table() + C.table()[:5], C.expected() + C.expected()[:5]
    items = tuple((pt, d, nbits, i % 64) for i, (pt, d, nbits, _) in enumerate(table))
    assert len(items) > 3 * 64 and len(items) % 64        # several workgroups, a partial last one
    got = C.run(dev.xwd_mul, items)
    ref = C.run(host.xadicw_mul, items)
    assert [i for i, ((f, o), (hf, ho)) in enumerate(zip(got, ref)) if f != 1 or hf != 3 or o[:36] != ho[:36]] == []
    assert [i for i, ((f, o), w) in enumerate(zip(got, want)) if C.g1j(o[:36]) != w] == []


def test_pack_unpack_round_trips(libs):
    dev, host = libs
    got = C.run_pack(dev.xwd_pack)
    assert got == C.run_pack(host.xadicw_pack)
    for v, (packed, limbs) in zip(C.PACK_VALUES, got):
        assert packed == v and limbs == C.spell(v)
