"""hbtc_encrypt and hbtc_fr_poly_eval are part of the C ABI: declared in include/hbtc.h and in the
generated Rust FFI, exported by libhbtc.so, and refuse a null context (no GPU needed)."""
import ctypes
import os
import re

import numpy as np

from hbbft_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hbtc_encrypt", "hbtc_fr_poly_eval")


def _strip_comments(src, line_comment):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(line_comment + r".*", "", src)


def test_declared_in_header():
    src = _strip_comments(open(os.path.join(ROOT, "include", "hbtc.h")).read(), "//")
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*hbtc_ctx\s*\*" % name, src), name


def test_declared_in_rust_ffi():
    src = _strip_comments(open(os.path.join(ROOT, "rust", "hbtc-sys", "src", "ffi.rs")).read(), "//")
    for name in NAMES:
        assert re.search(r"\bpub\s+fn\s+%s\s*\(" % name, src), name


def test_bound_and_exported():
    lib = N.load()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name


def test_null_context_is_an_argument_error():
    lib = N.load()
    null = ctypes.c_void_p(0)
    pk = np.zeros(48, np.uint8)
    r = np.zeros(32, np.uint8)
    off = np.zeros(2, np.uint32)
    u, w, st = np.zeros(48, np.uint8), np.zeros(96, np.uint8), np.zeros(1, np.int32)
    assert lib.hbtc_encrypt(null, 1, N._ptr(pk), 0, N._ptr(r), null, N._ptr(off), N._ptr(u), null,
                            N._ptr(w), N._ptr(st)) == -1  # HBTC_ERR_ARG
    out = np.zeros(32, np.uint8)
    assert lib.hbtc_fr_poly_eval(null, 1, 1, N._ptr(r), 1, N._ptr(r), N._ptr(out)) == -1
