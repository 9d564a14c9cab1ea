"""tools/gen_fq_rr.py's relaxed-bound blocks and tools/rr_bounds.py, the bounds interpreter of the point
formulas on the redundant 13 x 30 form.  Runs without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fq_rr as G  # noqa: E402
import rr_bounds as R  # noqa: E402

from oracle import bls12_381 as B  # noqa: E402


def test_relaxed_blocks_selftest(capsys):
    """0, 1, p - 1, p, k p - 1 up to the declared value bound, every limb at its declared maximum and
    300 random pairs on the simulator, which treats any MAD carry-out as an error."""
    G.selftest_w(300)
    assert "constants ok" in capsys.readouterr().out


def test_squaring_doubled_limbs_fit_32_bits():
    assert all(2 * w < 1 << 32 for w in G.W_LIMBS)
    with pytest.raises(AssertionError):
        G.schedule(True, [1 << 31] * G.N)


def test_a_carry_out_is_an_error():
    ops, _ = G.schedule(False, G.W_LIMBS, G.W_LIMBS)
    with pytest.raises(OverflowError):
        G.run(ops, [0xFFFFFFFF] * G.N, [0xFFFFFFFF] * G.N)


def test_old_bound_regenerates_the_committed_blocks():
    """With every limb bounded by 2^30 - 1 the generator emits mont_mul / mont_sqr byte for byte."""
    text = open(os.path.join(ROOT, "hbbft_amd", "csrc", "fq_rr.h")).read()
    old = [G.M] * G.N
    for name, sq in (("mont_mul", False), ("mont_sqr", True)):
        assert G.asm_block(name + "_asm", sq, old, old) == G.asm_block(name + "_asm", sq)
        assert G.asm_block(name + "_asm", sq, old, old) + "\n" in text
        assert G.cxx_block(name + "_cxx", sq, old, old) + "\n" in text
        assert G.asm_block(name + "_w_asm", sq, G.W_LIMBS, G.W_LIMBS) + "\n" in text
        assert G.cxx_block(name + "_w_cxx", sq, G.W_LIMBS, G.W_LIMBS) + "\n" in text
    for b, k in G.SUB_CONSTS:
        assert G.arr("RR_SUB_%d_%d" % (b, k), G.sub_const(b, k)) in text


def test_closure_of_the_loop_invariant():
    assert R.check_closure()


class _NoNorm(R.Bounds):
    """a scratch copy of the schedule with the n-th normalisation removed"""

    def __init__(self, forced, skip):
        super().__init__(forced)
        self.skip, self.seen = skip, 0

    def norm(self, a):
        self.seen += 1
        return a if self.seen == self.skip else super().norm(a)


def test_a_removed_normalisation_is_refused():
    ent = R.entry()
    refused = 0
    for skip in range(1, 8):            # jacw_dbl has seven
        try:
            out = R.jacw_dbl(_NoNorm({}, skip), (ent, ent, ent))
            if not all(b.within(ent) for b in out):
                raise R.BoundsError("closure")
        except R.BoundsError:
            refused += 1
    assert refused == 7


def test_a_lowered_subtraction_constant_is_refused(monkeypatch):
    ent = R.entry()
    for const in (R.S2, R.S2B, R.S2C):
        low = dict(R.Bounds.consts)
        low[const] = G.sub_const(1, const[1])        # one unit lent instead of two
        monkeypatch.setattr(R.Bounds, "consts", low)
        with pytest.raises(R.BoundsError):
            R.jacw_dbl(R.Bounds(), (ent, ent, ent))
    low = dict(R.Bounds.consts)
    low[R.S2D] = G.sub_const(2, 11)                  # a multiple of p below the subtrahend's value
    monkeypatch.setattr(R.Bounds, "consts", low)
    with pytest.raises(R.BoundsError):
        R.jacw_add_aff(R.Bounds(), (ent, ent, ent), (R.strict(1.5), R.strict(1.5)))


def test_the_schedule_on_actual_limbs_matches_the_oracle():
    """tools/rr_bounds.py's formulas (the ones the interpreter checks) compute [|x|] P and [x^2] P."""
    o = R.Limbs()
    rp = 1 << G.RBITS
    g = B.G1_GEN

    def aff(j):
        x, y, z = [R.val(c) * pow(rp, -1, B.P) % B.P for c in j]
        zi = pow(z, -1, B.P)
        return (x * zi * zi % B.P, y * zi * zi * zi % B.P)

    t1 = R.jacw_mul_x(o, (G.limbs(g[0] * rp % B.P), G.limbs(g[1] * rp % B.P)), True)
    assert aff(t1) == B.g1_mul(g, R.X_ABS)
    assert aff(R.jacw_mul_x(o, t1, False)) == B.g1_mul(g, R.X_ABS ** 2)
