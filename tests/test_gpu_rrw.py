"""The redundant 13 x 30 form on gfx950 (field.h FqW over fq_rr.h's relaxed-bound inline-asm blocks,
curve.h jacw_*): the tables of tests/test_rrw_host.py, one item per lane on 64-lane workgroups
(tests/native/hbtc_rrw_devtest.hip, built with the flags of the k_rlc_decode object).  Results must
equal the host build's (the plain C++ schedule with every bound asserted) as canonical residues, the
flags exactly; they are also checked against Python integers and oracle/bls12_381.py directly."""
import ctypes
import os
import subprocess

import pytest

import rrw_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "tests", "native", "libhbtc_rrw_devtest.so")
HOST = os.path.join(ROOT, "tests", "native", "libhbtc_rrw_hosttest.so")


def _load(path, target, fn):
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", ROOT, target])
    lib = ctypes.CDLL(path)
    getattr(lib, fn).argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def libs():
    dev = _load(DEV, "tests/native/libhbtc_rrw_devtest.so", "rwd_subgroup")
    host = _load(HOST, "tests/native/libhbtc_rrw_hosttest.so", "rrw_subgroup")
    assert dev.rwd_devices() >= 1
    return dev, host


def _residues(got):
    return [([C.val(o) % C.P for o in outs], f) for outs, f in got]


def test_operations_equal_the_host_build(libs):
    dev, host = libs
    ft, want, pt = C.cases()
    items = list(ft) + [(op, ins) for op, ins, _, _ in pt]
    assert len(items) % 64 != 0 and len(items) > 64   # more than one workgroup, a partial last one
    got = C.run(dev.rwd_ops, items)
    assert _residues(got) == _residues(C.run(host.rrw_ops, items))
    assert C.check_fields(ft, want, got[:len(ft)]) == []
    assert C.check_points(pt, got[len(ft):]) == []


def test_x_chains_and_subgroup_verdict(libs):
    dev, host = libs
    got = C.run_subgroup(dev.rwd_subgroup)
    assert C.check_subgroup(got) == []
    assert got == C.run_subgroup(host.rrw_subgroup)
