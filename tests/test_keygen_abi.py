"""hbtc_skg_generate is part of the C ABI: declared in include/hbtc.h and in the generated Rust
FFI, bound in the ctypes signatures, exported by libhbtc.so, and refuses a null context (no GPU
needed)."""
import ctypes
import os
import re

import numpy as np

from hbbft_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hbtc_skg_generate"


def _strip_comments(src, line_comment):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(line_comment + r".*", "", src)


def test_declared_in_header():
    src = _strip_comments(open(os.path.join(ROOT, "include", "hbtc.h")).read(), "//")
    m = re.search(r"\bint\s+%s\s*\(\s*hbtc_ctx\s*\*([^;]*)\)\s*;" % NAME, src)
    assert m, NAME
    # 13 parameters, as the ctypes signature binds them
    assert m.group(1).count(",") + 1 == len(N.SIGNATURES[NAME][1])


def test_declared_in_rust_ffi_and_wrapped():
    rust = os.path.join(ROOT, "rust", "hbtc-sys", "src")
    src = _strip_comments(open(os.path.join(rust, "ffi.rs")).read(), "//")
    assert re.search(r"\bpub\s+fn\s+%s\s*\(" % NAME, src)
    lib = _strip_comments(open(os.path.join(rust, "lib.rs")).read(), "//")
    assert re.search(r"\bpub\s+fn\s+skg_generate\s*\(", lib) and "ffi::%s" % NAME in lib


def test_bound_and_exported():
    lib = N.load()
    assert NAME in N.SIGNATURES
    assert hasattr(lib, NAME)
    assert hasattr(N.Context, "skg_generate")


def test_null_context_is_an_argument_error():
    lib = N.load()
    null = ctypes.c_void_p(0)
    row0, commit, pk = np.zeros(48, np.uint8), np.zeros(48, np.uint8), np.zeros(48, np.uint8)
    off, x = np.array([0, 1], np.uint32), np.array([1], np.uint32)
    val, sk = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    kid, st = ctypes.c_uint32(7), ctypes.c_int32(-9)
    rc = lib.hbtc_skg_generate(null, 1, 0, N._ptr(row0), N._ptr(off), N._ptr(x), N._ptr(val), 1,
                               N._ptr(commit), N._ptr(pk), N._ptr(sk), ctypes.byref(kid), ctypes.byref(st))
    assert rc == -1  # HBTC_ERR_ARG
    assert kid.value == 7 and st.value == -9 and not commit.any() and not sk.any()


def test_timing_family_is_documented():
    src = open(os.path.join(ROOT, "include", "hbtc.h")).read()
    fam = src[src.index("/* Families:"):src.index("int hbtc_timing_enable")]
    assert '"keygen"' in fam
