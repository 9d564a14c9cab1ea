"""hbtc_threshold_decrypt, hbtc_pad_xor_dev and hbtc_dec_epoch_submit_plain are part of the C ABI:
declared in include/hbtc.h and in the generated Rust FFI, bound in SIGNATURES, exported by
libhbtc.so, and refuse a null context (no GPU needed)."""
import ctypes
import os
import re

import numpy as np

from hbbft_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hbtc_threshold_decrypt", "hbtc_pad_xor_dev", "hbtc_dec_epoch_submit_plain")


def _strip_comments(src, line_comment):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(line_comment + r".*", "", src)


def test_declared_in_header():
    src = _strip_comments(open(os.path.join(ROOT, "include", "hbtc.h")).read(), "//")
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*hbtc_ctx\s*\*" % name, src), name


def test_timing_family_listed_in_header():
    src = open(os.path.join(ROOT, "include", "hbtc.h")).read()
    families = src[src.index("/* Families:"):src.index("int hbtc_timing_enable")]
    assert '"dec_pad"' in families


def test_declared_in_rust_ffi():
    src = _strip_comments(open(os.path.join(ROOT, "rust", "hbtc-sys", "src", "ffi.rs")).read(), "//")
    for name in NAMES:
        assert re.search(r"\bpub\s+fn\s+%s\s*\(" % name, src), name


def test_bound_and_exported():
    lib = N.load()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    for method in ("threshold_decrypt", "pad_xor", "dec_epoch_submit_plain"):
        assert callable(getattr(N.Context, method)), method


def test_null_context_is_an_argument_error():
    lib = N.load()
    null = ctypes.c_void_p(0)
    g2 = np.zeros(96, np.uint8)
    off = np.asarray([0, 1], np.uint32)
    voff = np.asarray([0, 4], np.uint32)
    idx = np.zeros(1, np.uint32)
    share, v, plain = np.zeros(48, np.uint8), np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    st, cst, g = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(48, np.uint8)
    p = N._ptr
    assert lib.hbtc_threshold_decrypt(null, 1, 1, p(g2), p(g2), p(off), p(idx), p(share), 1, p(v), p(voff),
                                      p(st), p(g), p(plain), p(cst)) == -1  # HBTC_ERR_ARG
    assert lib.hbtc_pad_xor_dev(null, 1, null, null, p(voff), null, null) == -1
    tk = ctypes.c_uint64()
    assert lib.hbtc_dec_epoch_submit_plain(null, 1, 1, p(g2), p(g2), p(off), p(idx), p(share), 1, p(v), p(voff),
                                           p(st), p(g), p(plain), p(cst), ctypes.byref(tk)) == -1
