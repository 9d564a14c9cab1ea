"""GPU checks of the G1 bucket walk on the redundant 13 x 30 form (k_msm_buckets<Fq> over curve.h's JacW)
through the public API, against the Python oracle: the decryption combines through Pippenger at t = 65
(the smallest t past the one-workgroup combines) and t = 100, and one MSM whose buckets see the same
point several times in a row (the mixed addition's doubling case at the step) beside a point and its
negation and an infinity encoding.

Bar: byte-identical compressed points (integer arithmetic, no tolerance).  The walk's other shapes
(idle lanes, a lane leaving every rank, crowded windows) are tests/test_gpu_msm_walk.py's, which runs
on the same kernel.
"""
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
INF = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def _gen(ctx, vals):
    """[v] G compressed through the library (hbtc_g1_mul, checked against the oracle in test_gpu_parity)"""
    red = [v % R for v in vals]
    out, st = ctx.g1_mul(G1, [v or 1 for v in red])
    assert not st.any()
    return [bytes(out[48 * i:48 * i + 48]) if v else INF for i, v in enumerate(red)]


def _oracle(k):
    k %= R
    return B.g1_compress(B.g1_mul(B.G1_GEN, k)) if k else INF


@pytest.mark.parametrize("t", [65, 100])
def test_decrypt_combine_through_pippenger(ctx, t):
    """2 instances of t shares at scattered indices of N = 128: the combine is [f(0) r_k] G."""
    rng = random.Random(1600 + t)
    n_inst = 2
    coeffs = [rng.randrange(1, R) for _ in range(t)]
    idx, scal, rs = [], [], []
    for k in range(n_inst):
        r = rng.randrange(1, R)
        rs.append(r)
        ix = sorted(rng.sample(range(128), t))
        idx += ix
        scal += [sum(c * pow(i + 1, j, R) for j, c in enumerate(coeffs)) % R * r % R for i in ix]
    g, st = ctx.combine_dec([t] * n_inst, idx, _gen(ctx, scal), t)
    assert list(st) == [N.ACCEPT] * n_inst
    assert g == [_oracle(coeffs[0] * r) for r in rs]


def test_msm_with_repeated_points_in_a_bucket(ctx):
    """n = 12 under one scalar: P four times in a row, Q and -Q, an infinity encoding, then five points
    of their own.  Every window's bucket of the shared digit sees P + P, 2P + P, 3P + P at the step."""
    rng = random.Random(1699)
    p, q = rng.randrange(1, R), rng.randrange(1, R)
    a = [p, p, p, p, q, R - q, 0] + [rng.randrange(1, R) for _ in range(5)]
    k0 = rng.randrange(1, R)
    k = [k0] * 7 + [k0, k0] + [rng.randrange(1, R) for _ in range(3)]
    out, st = ctx.g1_msm(1, len(a), _gen(ctx, a), k)
    assert list(st) == [N.ACCEPT]
    assert out == [_oracle(sum(x * y for x, y in zip(k, a)))]
