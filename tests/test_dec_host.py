"""The decryption pad on the CPU: the bodies of k_dec_seed (enc.h dec_seed_item) and k_enc_pad
(enc.h enc_pad_lane) compiled for the HOST behind tests/native/hbtc_dec_hosttest.cpp's dh_dec_pad,
against oracle.threshold_crypto.hash_bytes.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_dec_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_dec_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f)
    for f in ("enc.h", "hash_hd.h")]

INF = bytes([0xC0]) + bytes(47)
# a gated-out item (NOT_ENOUGH_SHARES) between open ones, zero-length items at the start, in the
# middle and at the end, the infinity encoding, lengths around the 16-byte block, one long item
LENGTHS = [0, 1, 15, 16, 17, 40, 0, 64, 65, 136, 137, 1000, 2051, 0]
GATED = {4: 5, 11: 6}
INFINITY_AT = 7


@pytest.fixture(scope="module")
def eh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_dec_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    lib.dh_dec_pad.restype = None
    lib.dh_dec_pad.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 6
    return lib


@pytest.fixture(scope="module")
def batch():
    rng = random.Random(31337)
    pts = [B.g1_mul(B.G1_GEN, rng.randrange(1, B.R)) for _ in LENGTHS]
    pts[INFINITY_AT] = None
    gs = [B.g1_compress(p) for p in pts]
    assert gs[INFINITY_AT] == INF
    vs = [bytes(rng.randrange(256) for _ in range(n)) for n in LENGTHS]
    pads = [TC.hash_bytes(p, n) for p, n in zip(pts, LENGTHS)]  # the reference, computed once
    return gs, vs, pads


def _run(eh, gs, vs, gate):
    n = len(gs)
    g = np.frombuffer(b"".join(gs), np.uint8).copy()
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(v) for v in vs])
    v = np.frombuffer(b"".join(vs), np.uint8).copy()
    out = np.full(v.size + 16, 0xAA, np.uint8)  # 16 guard bytes behind the last range
    gate_out = np.full(n, -1, np.int32)
    gt = None if gate is None else np.asarray(gate, np.int32)
    eh.dh_dec_pad(n, g.ctypes.data, None if gt is None else gt.ctypes.data, off.ctypes.data,
                  v.ctypes.data, out.ctypes.data, gate_out.ctypes.data)
    assert (out[v.size:] == 0xAA).all()
    return [out[off[i]:off[i + 1]].tobytes() for i in range(n)], gate_out


def test_batch_with_gate_equals_hash_bytes(eh, batch):
    gs, vs, pads = batch
    gate = [GATED.get(i, 0) for i in range(len(gs))]
    out, gate_out = _run(eh, gs, vs, gate)
    for i, (v, pad) in enumerate(zip(vs, pads)):
        if i in GATED:
            assert out[i] == bytes(len(v)), i  # zero-filled, the neighbours untouched by it
            assert gate_out[i] != 0
        else:
            assert out[i] == bytes(a ^ b for a, b in zip(v, pad)), i
            assert gate_out[i] == 0


def test_null_gate_passes_every_item(eh, batch):
    gs, vs, pads = batch
    out, gate_out = _run(eh, gs, vs, None)
    assert (gate_out == 0).all()
    assert out == [bytes(a ^ b for a, b in zip(v, pad)) for v, pad in zip(vs, pads)]


def test_infinity_encoding_is_hashed_as_bytes(eh, batch):
    """hash_bytes(O, n): the reference hashes the 48 bytes 0xC0 00.. like any other point."""
    gs, vs, pads = batch
    out, _ = _run(eh, [INF], [bytes(40)], None)
    assert out[0] == TC.hash_bytes(None, 40) == pads[INFINITY_AT][:40]
