"""hbtc_skg_part and hbtc_skg_acks are part of the C ABI: declared in include/hbtc.h and in the
generated Rust FFI, bound in hbbft_amd/_native.py, exported by libhbtc.so, and refuse a null
context (no GPU needed)."""
import ctypes
import os
import re

import numpy as np

from hbbft_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hbtc_skg_part", "hbtc_skg_acks")


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


def test_safe_rust_wrappers_exist():
    src = _strip_comments(open(os.path.join(ROOT, "rust", "hbtc-sys", "src", "lib.rs")).read(), "//")
    for name in NAMES:
        assert re.search(r"\bpub\s+fn\s+%s\s*\(" % name[len("hbtc_"):], src), name
        assert "ffi::%s(" % name in src, name


def test_bound_and_exported():
    lib = N.load()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert hasattr(N.Context, "skg_part") and hasattr(N.Context, "skg_acks")
    assert N.SKG_ACKS_MAX_ITEMS == 1 << 20


def test_null_context_is_an_argument_error():
    lib = N.load()
    null = ctypes.c_void_p(0)
    b, r = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    cm, u, v, w = np.zeros(48, np.uint8), np.zeros(48, np.uint8), np.zeros(48, np.uint8), np.zeros(96, np.uint8)
    st = np.zeros(1, np.int32)
    assert lib.hbtc_skg_part(null, 0, 0, N._ptr(b), N._ptr(r), N._ptr(cm), N._ptr(u), N._ptr(v), N._ptr(w),
                             N._ptr(st)) == -1  # HBTC_ERR_ARG
    assert lib.hbtc_skg_acks(null, 0, 1, 1, N._ptr(b), N._ptr(r), N._ptr(u), N._ptr(v), N._ptr(w),
                             N._ptr(st)) == -1
