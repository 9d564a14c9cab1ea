"""hbtc_decrypt_shares and hbtc_sign_shares are part of the C ABI: declared in include/hbtc.h and in
the generated Rust FFI, bound in hbbft_amd._native, exported by libhbtc.so, and refuse a null
context (no GPU needed)."""
import ctypes
import os
import re

import numpy as np

from hbbft_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hbtc_decrypt_shares", "hbtc_sign_shares")


def _strip_comments(src, line_comment):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(line_comment + r".*", "", src)


def test_declared_in_header():
    src = _strip_comments(open(os.path.join(ROOT, "include", "hbtc.h")).read(), "//")
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*hbtc_ctx\s*\*" % name, src), name


def test_named_in_the_header_tables():
    """The mapping table at the top of the header and the timing comment name the new calls."""
    src = open(os.path.join(ROOT, "include", "hbtc.h")).read()
    head = src[:src.index("#ifndef HBTC_H")]
    for name in NAMES:
        assert name in head, name
    timing = src[src.index("---- kernel timing"):]
    assert '"own_dec"' in timing and '"own_sig"' in timing


def test_declared_in_rust_ffi():
    src = _strip_comments(open(os.path.join(ROOT, "rust", "hbtc-sys", "src", "ffi.rs")).read(), "//")
    for name in NAMES:
        assert re.search(r"\bpub\s+fn\s+%s\s*\(" % name, src), name


def test_bound_and_exported():
    lib = N.load()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert callable(N.Context.decrypt_shares) and callable(N.Context.sign_shares)


def test_null_context_is_an_argument_error():
    lib = N.load()
    null = ctypes.c_void_p(0)
    sk = np.zeros(32, np.uint8)
    off = np.zeros(2, np.uint32)
    u, w = np.zeros(48, np.uint8), np.zeros(96, np.uint8)
    g, H, st = np.zeros(48, np.uint8), np.zeros(96, np.uint8), np.zeros(1, np.int32)
    assert lib.hbtc_decrypt_shares(null, 1, N._ptr(sk), N._ptr(u), null, N._ptr(off), N._ptr(w),
                                   N._ptr(g), N._ptr(H), N._ptr(st)) == -1  # HBTC_ERR_ARG
    assert lib.hbtc_decrypt_shares(null, 0, null, null, null, null, null, null, null, null) == -1
    sig = np.zeros(96, np.uint8)
    assert lib.hbtc_sign_shares(null, 1, N._ptr(sk), null, N._ptr(off), N._ptr(sig), N._ptr(H)) == -1
    assert lib.hbtc_sign_shares(null, 0, null, null, null, null, null) == -1
