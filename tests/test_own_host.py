"""own_host.h (the secret scalar of hbtc_decrypt_shares / hbtc_sign_shares on the host: reduction
mod r, the x^2 split behind k_pb_mul_glv, the base-|x| digits of curve.h gls_u_digits behind
k_sig_share, and the wiping of every copy) compiled for the HOST and checked against Python
integers.  Runs without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_own_hosttest.so")
SRC = [os.path.join(ROOT, "tests", "native", "hbtc_own_hosttest.cpp")] + [
    os.path.join(ROOT, "hbbft_amd", "csrc", f) for f in ("own_host.h", "curve.h", "field.h", "bls_constants.h")]

R = B.R
U = 0xd201000000010000  # |x|
X2 = U * U
assert abs(B.X) == U and R == U ** 4 - U ** 2 + 1
# canonical scalars: 0, 1, r - 1, the digit edges |x| -+ 1, |x|^2 - 1, around x^2, |x|^3 -+ 1, and
# all digits at their maximum below r
EDGE_CANONICAL = [0, 1, 2, R - 1, R - 2, U - 1, U, U + 1, X2 - 1, X2, X2 + 1, U ** 3 - 1, U ** 3, U ** 3 + 1,
                  (U - 1) * (1 + U + X2), 1 << 64, (1 << 64) - 1, 1 << 128, (1 << 128) - 1, (1 << 192) + 1]
EDGE_ANY = EDGE_CANONICAL + [R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, (1 << 255), (1 << 256) - 1]


@pytest.fixture(scope="module")
def oh():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in SRC):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_own_hosttest.so"])
    lib = ctypes.CDLL(LIB)
    for name in ("oh_mod_r", "oh_split_x2", "oh_u_digits", "oh_wipe"):
        getattr(lib, name).restype = None
    lib.oh_secret_scalar.restype = ctypes.c_uint32
    lib.oh_wipe.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    return lib


def le32(k):
    return int(k).to_bytes(32, "little")


def _canonical(seed, n):
    rng = random.Random(seed)
    return EDGE_CANONICAL + [rng.randrange(R) for _ in range(n)] + [rng.randrange(1 << b) for b in (1, 63, 65, 127, 129, 191)]


def _digits(oh, k):
    d = (ctypes.c_uint64 * 4)()
    oh.oh_u_digits(le32(k), d)
    return list(d)


def test_scalar_mod_r(oh):
    rng = random.Random(1)
    for k in EDGE_ANY + [rng.randrange(1 << 256) for _ in range(200)]:
        out = ctypes.create_string_buffer(32)
        oh.oh_mod_r(le32(k), out)
        assert int.from_bytes(out.raw, "little") == k % R, hex(k)


def test_split_by_x2(oh):
    for k in _canonical(2, 200):
        k0, k1 = ctypes.create_string_buffer(16), ctypes.create_string_buffer(16)
        oh.oh_split_x2(le32(k), k0, k1)
        a, b = int.from_bytes(k0.raw, "little"), int.from_bytes(k1.raw, "little")
        assert (a, b) == (k % X2, k // X2), hex(k)


def test_gls_u_digits(oh):
    """k = sum d_j |x|^j with every d_j < |x|: the base-|x| digits, unique."""
    for k in _canonical(3, 300):
        want = [(k // U ** j) % U for j in range(4)]
        assert _digits(oh, k) == want, hex(k)
    assert _digits(oh, R - 1) == [0, 0, U - 1, U - 1]  # r - 1 = x^2 (x^2 - 1)


def test_secret_scalar_forms_and_wipe(oh):
    """The object a call holds: the three forms of sk mod r for any 256-bit sk, and nothing of
    them left in its storage after its destructor."""
    rng = random.Random(4)
    for sk in EDGE_ANY + [rng.randrange(1 << 256) for _ in range(50)]:
        k, k0, k1 = (ctypes.create_string_buffer(n) for n in (32, 16, 16))
        d = (ctypes.c_uint64 * 4)()
        after = ctypes.create_string_buffer(b"\xaa" * 256, 256)
        size = oh.oh_secret_scalar(le32(sk), k, k0, k1, d, after, 256)
        kr = sk % R
        assert int.from_bytes(k.raw, "little") == kr
        assert (int.from_bytes(k0.raw, "little"), int.from_bytes(k1.raw, "little")) == (kr % X2, kr // X2)
        assert list(d) == [(kr // U ** j) % U for j in range(4)]
        assert 96 <= size <= 256 and after.raw[:size] == bytes(size), hex(sk)


def test_wipe_words(oh):
    buf = (ctypes.c_uint32 * 9)(*([0xdeadbeef] * 9))
    oh.oh_wipe(ctypes.byref(buf, 4), 7)  # the inner seven words only
    assert list(buf) == [0xdeadbeef] + [0] * 7 + [0xdeadbeef]
