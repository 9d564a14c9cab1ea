"""tools/rr_bounds.py on the item pass's x-adic multiplication on the redundant 13 x 30 form (curve.h
xadic_mul_sac8_w): the packed co-Z table chain, the column (a doubling, then the mixed addition of an
entry whose y may be negated), the even-d0 correction and the exit.  The invariant closes; the checks
refuse a schedule with a normalisation removed, a lowered subtraction constant, or something packed
that is not a product result; the same schedules on actual limbs compute [r] P.  Runs without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fq_rr as G  # noqa: E402
import rr_bounds as R  # noqa: E402

from oracle import bls12_381 as B  # noqa: E402

X = -R.X_ABS
MU = -X * X


def test_generator_emits_beta_and_the_header_is_current():
    text = open(os.path.join(ROOT, "hbbft_amd", "csrc", "fq_rr.h")).read()
    assert G.arr("RR_BETA", G.limbs(G.BETA * G.ONE % G.P_MOD)) in text
    g = B.G1_GEN
    assert (G.BETA * g[0] % B.P, g[1]) == B.g1_mul(g, MU % B.R)       # phi(P) = [mu] P
    for b, k in G.SUB_CONSTS:
        assert G.arr("RR_SUB_%d_%d" % (b, k), G.sub_const(b, k)) in text


def test_closure_of_the_item_pass():
    assert R.check_items_closure()


class _NoNorm(R.Bounds):
    def __init__(self, skip):
        super().__init__()
        self.skip, self.seen = skip, 0

    def norm(self, a):
        self.seen += 1
        return a if self.seen == self.skip else super().norm(a)


def test_a_removed_normalisation_of_the_column_is_refused():
    """jacw_dbl has seven, fw_neg one, jacw_madd_generic three and the tail six."""
    ent, e = R.entry(), (R.strict(R.PACK_V), R.strict(R.PACK_V))
    counter = _NoNorm(0)
    R.column(counter, (ent, ent, ent), e, True)
    assert counter.seen == 17
    refused = 0
    for skip in range(1, counter.seen + 1):
        try:
            out = R.column(_NoNorm(skip), (ent, ent, ent), e, True)
            if not all(b.within(ent) for b in out):
                raise R.BoundsError("closure")
        except R.BoundsError:
            refused += 1
    assert refused == counter.seen


def test_a_removed_normalisation_of_the_co_z_sum_is_refused():
    a = (R.strict(R.PACK_V), R.strict(R.PACK_V))
    counter = _NoNorm(0)
    R.coz_add_w(counter, a, a)
    assert counter.seen == 6
    for skip in range(1, 7):
        with pytest.raises(R.BoundsError):
            s, u, h = R.coz_add_w(_NoNorm(skip), a, a)
            o = R.Bounds()
            for c in s + u:
                o.pack(c)
            o.sqr(h)


def test_packing_anything_but_a_product_result_is_refused():
    o = R.Bounds()
    with pytest.raises(R.BoundsError):
        o.pack(o.add(R.strict(1), R.strict(1)))                  # a sum: limbs may pass 2^30 - 1
    with pytest.raises(R.BoundsError):
        o.pack(R.strict(2))                                      # a value that may pass 1.5p
    with pytest.raises(R.BoundsError):
        o.pack(o.norm(o.sub(R.strict(1), R.strict(1), R.S1)))    # a difference, even normalised
    o.pack(o.mul(R.entry(), R.entry()))                          # (144 / 630 + 1) p


def test_a_lowered_subtraction_constant_is_refused(monkeypatch):
    a = (R.strict(R.PACK_V), R.strict(R.PACK_V))
    low = dict(R.Bounds.consts)
    low[R.S2C] = G.sub_const(2, 8)                               # v - x3 with x3 up to 9.1p
    monkeypatch.setattr(R.Bounds, "consts", low)
    with pytest.raises(R.BoundsError):
        R.coz_add_w(R.Bounds(), a, a)


@pytest.mark.parametrize("nbits,d", [(16, (0x8001, 0xFFFF, 3, 0x8000)), (16, (0x1234, 0, 77, 1)), (16, (0, 0, 0, 0)),
                                     (32, (0xFFFFFFFE, 0x80000000, 0x12345678, 1))])
def test_the_schedule_on_actual_limbs_matches_the_oracle(nbits, d):
    """The formulas the interpreter checks compute [d0 + d1 x + d2 mu + d3 mu x] P (odd and even d0, the
    zero scalar), every pack on limbs below 2^30 and an integer below 2^384."""
    o = R.Limbs()
    rp = 1 << G.RBITS
    g = B.g1_mul(B.G1_GEN, 0xC0FFEE)
    xp = B.g1_mul(g, X % B.R)
    z = 0x1234567 * rp % B.P
    zr = 0x1234567
    lim = lambda v: G.limbs(v * rp % B.P)
    xpj = (lim(xp[0] * zr * zr), lim(xp[1] * zr ** 3), G.limbs(z))
    out = R.xadic_mul_sac8_w(o, (lim(g[0]), lim(g[1])), xpj, d, nbits)
    x, y, zz = [R.val(c) * pow(1 << 384, -1, B.P) % B.P for c in out]      # 12 x 32 Montgomery values
    k = (d[0] + d[1] * X + d[2] * MU + d[3] * MU * X) % B.R
    if k == 0:
        assert zz == 0
    else:
        zi = pow(zz, -1, B.P)
        assert (x * zi * zi % B.P, y * zi ** 3 % B.P) == B.g1_mul(g, k)
