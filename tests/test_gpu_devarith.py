"""The case tables of tests/devarith_cases.py run ON THE DEVICE through the test-only harness
tests/native/libhbtc_devtest.so (tests/native/hbtc_devtest.hip: the arithmetic headers compiled
for gfx950 once per variant of the Fq product) and compared with the Python-integer reference:
the generated asm in its three forms (shared subroutines on fixed registers, the one-block inline
product, the out-of-line call), the lazy-accumulator subroutines, the lane-pair Fq2 / G2 code
(DPP exchanges) and the 6-lane GT operations (LDS staging, ds_bpermute), at edge operands that
random scalars reach with probability ~2^-32.  tests/test_devarith_host.py proves the same tables
and reference on the host fallback.  One launch per (family, variant)."""
import ctypes
import glob
import os
import subprocess

import pytest

import devarith_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_devtest.so")


@pytest.fixture(scope="module")
def dt():
    srcs = glob.glob(os.path.join(ROOT, "hbbft_amd", "csrc", "*.h"))
    srcs.append(os.path.join(ROOT, "tests", "native", "hbtc_devtest.hip"))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-s", "-j3", "-C", ROOT, "devtest"])
    lib = ctypes.CDLL(LIB)  # a missing library is an error, not a skip
    n = lib.dt_devices_sr()
    if n < 1:
        raise RuntimeError("no GPU for the device-arithmetic tests (device query returned %d)" % n)
    return lib


@pytest.fixture(scope="module")
def ht():
    """The host build of the same headers: the one-lane reference of the Miller-line walk."""
    lib = os.path.join(ROOT, "tests", "native", "libhbtc_hosttest.so")
    srcs = glob.glob(os.path.join(ROOT, "hbbft_amd", "csrc", "*.h"))
    srcs += [os.path.join(ROOT, "tests", "native", f) for f in ("gt_sim.cpp", "hbtc_hosttest.cpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-s", "-C", ROOT, "hosttest"])
    return ctypes.CDLL(lib)


@pytest.mark.parametrize("variant", ["sr", "inl", "call"])
def test_fq_ops_on_device(dt, variant):
    """Fq family, one item per lane, 13,132 items in blocks of 64 (the last block partial): exact
    integers and < 2p; fq_mul2 is the asm only in the subroutine build, elsewhere the fallback
    (congruence mod p and < 2p)."""
    table, want = C.fq_cases()
    assert len(table) % 64 != 0
    got = C.run_fq(getattr(dt, "dt_fq_" + variant), table)
    bad = C.check_fq(table, want, got, mul2_exact=(variant == "sr"))
    assert not bad, (len(bad), bad[:5])


def test_lazy_accumulators_on_device(dt):
    """fq_mac_sr / fq_redc_sr, the second accumulator's pair, macsub, subsub and the Karatsuba
    form, up to the 48 p^2 bound: exact integers and < 2p."""
    table, want = C.acc_cases()
    bad = C.check_acc(table, want, C.run_acc(dt.dt_acc_sr, table))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("variant", ["sr", "inl"])
def test_fq2_lane_pairs_on_device(dt, variant):
    """pair.h field operations on lane pairs (an odd item count: even and odd pair slots, a
    partial last wave) against the oracle's Fq2."""
    table, want = C.fq2_cases()
    assert len(table) % 2 == 1
    bad = C.check_fq2(table, want, C.run_fq2(getattr(dt, "dt_f2_" + variant), table))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("variant", ["sr", "inl"])
def test_g2_lane_pairs_on_device(dt, ht, variant):
    """Jacobian doubling / additions with their special cases, psi, the Miller-line walk with the
    psi subgroup test and the cofactor clearing (with the points of order 13 and 23 that make
    g(P) infinity) in pair form against the oracle's curve arithmetic; the walk's line triples
    against the one-lane line table of the host build."""
    table = C.g2_cases()
    assert len(table) % 2 == 1
    bad = C.check_g2(table, C.run_g2(getattr(dt, "dt_g2_" + variant), table), ht)
    assert not bad, bad


@pytest.mark.parametrize("rep", [1, 3])
def test_gt_ops_on_device(dt, rep):
    """The ten GT operations on real lanes: rep = 1 is the staged lazy path (10 groups per wave,
    lanes 60..63 idle), rep = 3 the replicated layout; the last wave of an operation has fewer
    live groups than it holds."""
    table, want = C.gt_cases()
    assert any(cnt < 64 // (6 * rep) for _op, _first, cnt in C.gt_blocks(table, rep)[1])
    bad = C.check_gt(table, want, C.run_gt_device(dt.dt_gt_sr, table, rep))
    assert not bad, bad
