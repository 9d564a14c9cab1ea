"""The Fq product / squaring on 13 limbs of 30 bits (tools/gen_fq_rr.py) on the CPU: the generator's
simulator runs both schedules on the edge operands (0, 1, p - 1, p, 2p - 1, 16p - 1, all limbs
2^30 - 1) and 300 random pairs against Python integers and raises on any v_mad_u64_u32 carry-out;
the committed header is exactly what the generator emits; the MAD counts are the reasoned ones."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen_fq_rr.py")


def _run(*args):
    return subprocess.run([sys.executable, GEN, *args], check=True, capture_output=True, text=True).stdout


def _gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_fq_rr as g
    finally:
        sys.path.pop(0)
    return g


def test_generator_selftest_rr():
    out = _run("--selftest-rr")
    assert "selftest_rr product ok" in out and "selftest_rr squaring ok" in out
    assert "selftest_rr conversions ok" in out


def test_committed_header_matches_generator():
    with open(os.path.join(ROOT, "hbbft_amd", "csrc", "fq_rr.h")) as f:
        assert f.read() == _run(), "fq_rr.h differs from tools/gen_fq_rr.py output"


def test_mad_counts_and_splits():
    """169 + 169 (product) and 91 + 169 (squaring) MADs plus one per overflow split; splits only in
    the middle columns; no carry instruction anywhere."""
    g = _gen()
    for square, macs in ((False, 338), (True, 260)):
        ops, info = g.schedule(square)
        kinds = [op[0] for op in ops]
        assert kinds.count("mad") + kinds.count("mad0") == macs
        assert kinds.count("madh") == kinds.count("split32") == len(info["splits"]) <= 6
        assert all(8 <= k <= 16 for k in info["splits"])
        assert info["max"] < 1 << 64
        text = "\n".join(g.asm_lines(ops, square))
        assert "addc" not in text and "v_add" not in text
        assert text.count("v_mad_u64_u32") == macs + len(info["splits"])
        assert text.count("v_mul_lo_u32") == 13


def test_simulator_rejects_a_carry_out():
    """The simulator's overflow check is live: the schedule with its splits removed overflows on
    all-limbs-maximal operands."""
    import pytest
    g = _gen()
    ops, _ = g.schedule(False)
    stripped = [op for op in ops if op[0] not in ("split32", "madh")]
    m = [g.M] * g.N
    with pytest.raises(OverflowError):
        g.run(stripped, m, m)
    g.run(ops, m, m)
