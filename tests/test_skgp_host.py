"""skgp.h (the item bodies of hbtc_skgp.hip's kernels: the paired commitment from the generator's
comb table, the Horner over the packed triangle, the Poly and FieldWrap frames) compiled for the
HOST, each kernel replayed lane by lane, and checked against Python integers, hbbft_amd/wire.py
and jac_mul_fr.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from hbbft_amd import wire
from hbbft_amd.skg import coeff_pos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_skgp_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_skgp_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f)
    for f in ("skgp.h", "enc.h", "hash_hd.h", "field.h", "curve.h", "bls_constants.h")]

R = wire.R
INF = bytes([0xC0]) + bytes(47)
GEN = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac58"
                    "6c55e83ff97a1aeffb3af00adb22c6bb")
EDGE = [0, 1, R - 1, R, R + 1, (1 << 256) - 1]


@pytest.fixture(scope="module")
def sh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_skgp_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    lib.sh_coeff_pos.restype = ctypes.c_uint32
    lib.sh_row_bytes.restype = ctypes.c_uint64
    return lib


def le32(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def commit(sh, coeffs):
    n = len(coeffs)
    out, ref = ctypes.create_string_buffer(48 * n), ctypes.create_string_buffer(48 * n)
    sh.sh_commit(n, le32(coeffs), out, ref)
    return [out.raw[48 * i:48 * i + 48] for i in range(n)], [ref.raw[48 * i:48 * i + 48] for i in range(n)]


def rows(sh, n_rows, t, b):
    rb = sh.sh_row_bytes(t + 1)
    assert rb == 8 + 40 * (t + 1)
    out = ctypes.create_string_buffer(rb * n_rows)
    sh.sh_rows(n_rows, t + 1, le32(b), out)
    return [out.raw[rb * i:rb * (i + 1)] for i in range(n_rows)]


def vals(sh, row_list, n_nodes):
    n_rows, n_coeff = len(row_list), len(row_list[0])
    out = ctypes.create_string_buffer(40 * n_rows * n_nodes)
    sh.sh_vals(n_rows, n_nodes, n_coeff, le32([c for r in row_list for c in r]) or None, out)
    return [out.raw[40 * i:40 * i + 40] for i in range(n_rows * n_nodes)]


def row_ints(b, t, x):
    """Row x of the packed triangle b by Python integers (any 256-bit entries, taken mod r)."""
    return [sum(b[coeff_pos(k, j)] * pow(x, j, R) for j in range(t + 1)) % R for k in range(t + 1)]


def test_coeff_pos_matches_the_python_form(sh):
    for i in range(12):
        for j in range(12):
            assert sh.sh_coeff_pos(i, j) == coeff_pos(i, j)


@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_paired_commitment_against_jac_mul_fr(sh, n):
    rng = random.Random(100 + n)
    got, ref = commit(sh, [rng.randrange(R) for _ in range(n)])
    assert got == ref
    assert len(set(got)) == n and INF not in got


def test_commitment_edges(sh):
    # a zero paired with a non-zero coefficient in either place of the lane, an odd count whose last
    # lane holds one point, and every scalar the reduction has to handle
    got, ref = commit(sh, [0, 5, 7, 0, 0, 0, 9])
    assert got == ref
    assert [g == INF for g in got] == [True, False, False, True, True, True, False]
    got, ref = commit(sh, EDGE + [0])
    assert got == ref
    assert got[0] == INF and got[3] == INF and got[6] == INF     # 0, r, 0
    assert got[1] == GEN and got[4] == GEN                       # 1, r + 1
    assert got[5] == commit(sh, [((1 << 256) - 1) % R])[0][0]
    assert got[2] == bytes([GEN[0] ^ 0x20]) + GEN[1:]            # (r - 1) G = -G


@pytest.mark.parametrize("n_rows,t", [(1, 0), (4, 1), (7, 2), (5, 3), (33, 10), (3, 40)])
def test_rows_against_python_integers_and_wire(sh, n_rows, t):
    rng = random.Random(1000 * n_rows + t)
    b = [rng.randrange(R) for _ in range((t + 1) * (t + 2) // 2)]
    got = rows(sh, n_rows, t, b)
    for x in range(1, n_rows + 1):
        assert got[x - 1] == wire.poly_to_wire(row_ints(b, t, x)), x


def test_rows_edge_scalars(sh):
    b = EDGE                                                     # t = 2: six entries
    got = rows(sh, 4, 2, b)
    for x in range(1, 5):
        assert got[x - 1] == wire.poly_to_wire(row_ints(b, 2, x))
    assert wire.poly_from_wire(rows(sh, 2, 1, [0, 0, 0])[1]) == [0, 0]


@pytest.mark.parametrize("n_rows,n_nodes,n_coeff", [(1, 4, 2), (3, 7, 3), (2, 5, 1), (2, 300, 4)])
def test_values_against_python_integers_and_wire(sh, n_rows, n_nodes, n_coeff):
    rng = random.Random(n_rows * 31 + n_nodes)
    rl = [[rng.randrange(R) for _ in range(n_coeff)] for _ in range(n_rows)]
    got = vals(sh, rl, n_nodes)
    for a in range(n_rows):
        for i in range(n_nodes):
            want = sum(c * pow(i + 1, k, R) for k, c in enumerate(rl[a])) % R
            assert got[a * n_nodes + i] == wire.fr_to_wire(want), (a, i)


def test_values_edges(sh):
    got = vals(sh, [EDGE], 3)
    for i in range(3):
        assert got[i] == wire.fr_to_wire(sum(c * pow(i + 1, k, R) for k, c in enumerate(EDGE)) % R)
    assert vals(sh, [[], []], 3) == [wire.fr_to_wire(0)] * 6    # no coefficients: every value is 0
