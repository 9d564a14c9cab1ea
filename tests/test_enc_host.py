"""enc.h (the arithmetic of hbtc_enc.hip's kernels: the generator's window table, the comb and
GLV multiplications, the pad's block addressing, Fr Horner) compiled for the HOST and checked
against the Python oracle.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_enc_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_enc_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f)
    for f in ("enc.h", "hash_hd.h", "field.h", "curve.h", "bls_constants.h")]

R = B.R
EDGE_SCALARS = [1, 2, 255, 256, 1 << 64, R - 1, R, R + 1, (1 << 256) - 1]
LENGTHS = [0, 1, 15, 16, 17, 40, 64, 65, 136, 137, 1000]


@pytest.fixture(scope="module")
def eh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_enc_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    for name in ("eh_table_entry", "eh_split", "eh_pad_blocks", "eh_pad_serial", "eh_fr_horner"):
        getattr(lib, name).restype = None
    lib.eh_pad_blocks.argtypes = lib.eh_pad_serial.argtypes = [ctypes.c_char_p, ctypes.c_uint64,
                                                              ctypes.c_char_p]
    return lib


def buf(n):
    return ctypes.create_string_buffer(max(n, 1))


def le32(k):
    return int(k).to_bytes(32, "little")


def scalars(seed, n):
    rng = random.Random(seed)
    return EDGE_SCALARS + [rng.randrange(R) for _ in range(n)]


def test_table_entries(eh):
    """tab[w][v] = v 2^(8w) G1, at the corners of the table and a few random entries."""
    rng = random.Random(11)
    cases = [(0, 1), (0, 255), (1, 1), (31, 1), (31, 255)] + \
        [(rng.randrange(32), rng.randrange(1, 256)) for _ in range(6)]
    for w, v in cases:
        o = buf(96)
        eh.eh_table_entry(w, v, o)
        want = B.g1_mul(B.G1_GEN, (v << (8 * w)) % R)
        assert (int.from_bytes(o.raw[:48], "big"), int.from_bytes(o.raw[48:96], "big")) == want, (w, v)
    o = buf(96)
    eh.eh_table_entry(5, 0, o)
    assert o.raw[:96] == bytes(96)


def test_split_by_x2(eh):
    x2 = B.X * B.X
    for k in scalars(2, 20):
        k0, k1 = buf(16), buf(16)
        eh.eh_split(le32(k), k0, k1)
        a, b = int.from_bytes(k0.raw[:16], "little"), int.from_bytes(k1.raw[:16], "little")
        assert a < x2 and a + b * x2 == k % R, hex(k)


def test_comb_and_glv_against_jac_mul_fr(eh):
    """u = r G1 (comb) and g = r pk (GLV) equal jac_mul_fr's products and the oracle's, for the
    edge scalars (r = 0 mod the order gives the point at infinity) and random ones; keys: the
    generator, a random point, the point at infinity."""
    rng = random.Random(3)
    pk_rand = B.g1_mul(B.G1_GEN, rng.randrange(1, R))
    inf = bytes([0xC0]) + bytes(47)
    for pk_pt, pk in ((B.G1_GEN, B.g1_compress(B.G1_GEN)), (pk_rand, B.g1_compress(pk_rand)), (None, inf)):
        for k in scalars(4, 4):
            u, g, ru, rg = buf(48), buf(48), buf(48), buf(48)
            assert eh.eh_enc_g1(pk, le32(k), u, g, ru, rg) == 0
            assert u.raw[:48] == ru.raw[:48] and g.raw[:48] == rg.raw[:48], hex(k)
            assert u.raw[:48] == B.g1_compress(B.g1_mul(B.G1_GEN, k % R)), hex(k)
            want_g = B.g1_compress(B.g1_mul(pk_pt, k % R)) if pk_pt is not None else inf
            assert g.raw[:48] == want_g, hex(k)
    bad = bytes.fromhex("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac58"
                        "6c55e83ff97a1aeffb3af00adb22c6bb")  # no compression flag
    assert eh.eh_enc_g1(bad, le32(1), buf(48), buf(48), buf(48), buf(48)) == -1


def test_g2_glv_against_jac_mul_fr(eh):
    """[r] H by the GLV split with m(H) = (zeta x, -y) = [x^2] H on G2."""
    rng = random.Random(5)
    H = B.g2_mul(B.G2_GEN, rng.randrange(1, R))
    hb = B.g2_compress(H)
    inf = bytes([0xC0]) + bytes(95)
    for k in scalars(6, 3):
        o, r = buf(96), buf(96)
        assert eh.eh_g2_glv(hb, le32(k), o, r) == 0
        assert o.raw[:96] == r.raw[:96], hex(k)
        want = B.g2_compress(B.g2_mul(H, k % R)) if k % R else inf
        assert o.raw[:96] == want, hex(k)


def test_pad_block_addressing(eh):
    """The pad built block by block (counter-mode) equals the serial next_u32 stream of the host
    hash_bytes and the oracle's hash_bytes, for lengths around the 16-byte block."""
    rng = random.Random(7)
    g = B.g1_mul(B.G1_GEN, rng.randrange(1, R))
    gb = B.g1_compress(g)
    for n in LENGTHS + [13368]:
        a, b = buf(n), buf(n)
        eh.eh_pad_blocks(gb, n, a)
        eh.eh_pad_serial(gb, n, b)
        assert a.raw[:n] == b.raw[:n], n
        if n <= 137:
            assert a.raw[:n] == TC.hash_bytes(g, n), n


def test_fr_horner(eh):
    rng = random.Random(9)
    pool = [0, 1, R - 1, R, (1 << 256) - 1]

    def draw():
        return rng.choice(pool) if rng.random() < 0.5 else rng.randrange(1 << 256)
    for n_coeff in (1, 2, 5, 334):
        for _ in range(4):
            c = [draw() for _ in range(n_coeff)]
            x = draw()
            o = buf(32)
            eh.eh_fr_horner(n_coeff, b"".join(le32(v) for v in c), le32(x), o)
            want = sum(v * pow(x, k, R) for k, v in enumerate(c)) % R
            assert int.from_bytes(o.raw[:32], "little") == want
