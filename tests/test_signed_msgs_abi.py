"""hbtc_verify_signed_msgs is part of the C ABI: declared in include/hbtc.h and in the generated Rust
FFI, exported by libhbtc.so and bound in _native.py with the header's argument list, and it refuses
a null context whatever else it is given -- NULL arrays, bad offsets -- before touching a GPU (no
GPU needed; the argument errors behind a live context: tests/test_gpu_signed_msgs.py)."""
import ctypes
import os
import re

import numpy as np

from hbbft_amd import _native as N
from hbbft_amd import dhb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hbtc_verify_signed_msgs"


def _strip_comments(src, line_comment):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(line_comment + r".*", "", src)


def test_declared_in_header_with_the_documented_arguments():
    src = _strip_comments(open(os.path.join(ROOT, "include", "hbtc.h")).read(), "//")
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["hbtc_ctx* ctx", "uint32_t keyset_id", "uint32_t n", "const uint32_t* signer",
                    "const uint8_t* msgs", "const uint32_t* offsets", "const uint8_t* sig_c96",
                    "int32_t* status"]


def test_declared_in_rust_ffi_and_wrapped():
    src = _strip_comments(open(os.path.join(ROOT, "rust", "hbtc-sys", "src", "ffi.rs")).read(), "//")
    assert re.search(r"\bpub\s+fn\s+%s\s*\(" % NAME, src)
    lib_rs = open(os.path.join(ROOT, "rust", "hbtc-sys", "src", "lib.rs")).read()
    assert re.search(r"\bpub\s+fn\s+verify_signed_msgs\s*\(", lib_rs) and "ffi::%s" % NAME in lib_rs


def test_bound_and_exported():
    lib = N.load()
    assert NAME in N.SIGNATURES and len(N.SIGNATURES[NAME][1]) == 8
    assert hasattr(lib, NAME)
    assert callable(N.Context.verify_signed_msgs) and callable(dhb.verify_signed)


def test_null_context_is_an_argument_error():
    lib = N.load()
    null = ctypes.c_void_p(0)
    who, st = np.zeros(1, np.uint32), np.zeros(1, np.int32)
    msg, sig = np.zeros(4, np.uint8), np.zeros(96, np.uint8)
    off = np.array([0, 4], np.uint32)
    f = getattr(lib, NAME)
    assert f(null, 1, 1, N._ptr(who), N._ptr(msg), N._ptr(off), N._ptr(sig), N._ptr(st)) == -1  # HBTC_ERR_ARG
    assert f(null, 1, 0, null, null, null, null, null) == -1       # even the empty call
    assert f(null, 1, 1, null, null, null, null, null) == -1       # NULL arrays
    bad = np.array([4, 0], np.uint32)                               # offsets[0] != 0, decreasing
    assert f(null, 1, 1, N._ptr(who), N._ptr(msg), N._ptr(bad), N._ptr(sig), N._ptr(st)) == -1
    assert st[0] == 0  # nothing was written
