"""k_rlc_decode with both |x| chains of its subgroup test on the redundant 13 x 30 form, through the
public API: one ciphertext of 80 DecryptionShares (a full tile and a ragged tile of 16) through
hbtc_verify_dec_shares and hbtc_combine_dec_verified_dev with exact_below = 0, so every share takes
the batched path.

Both tiles hold, among valid shares of both y signs (and one wrong share in the first): (0, 2) and
(0, -2) of order 3, a point of each prime order 3, 11, 10177, 859267 and 52437899 dividing the
cofactor, a point of order 33, P + T with P in G1 and T of order 3, and an on-curve point outside G1
-- the points whose chains meet the doubling of infinity, the addition into infinity and both exits
of the additions (tests/rrw_cases.py walk).  Every one of them must come out DECODE_ERR.

Reference: oracle/ -- G1Compressed::into_affine for the decode verdicts, PublicKeyShare::
verify_decryption_share (two pairings) for the wrong share and two valid ones of both signs, share ==
sk_i u for the other valid ones, PublicKeySet::decrypt's interpolation over the first t accepted
shares for the combined point.  The per-share mode (HBTC_MODE_PER_SHARE: the 12 x 32 subgroup test of
k_g1_decode, one pairing check per share) must give the same statuses and the same point."""
import random

import numpy as np
import pytest

import rrw_cases as C
from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

N_SHARES = 80
T = 24
FIRST = [3, 9, 14, 20, 27, 33, 38, 44, 51, 62]     # the special shares' places in the full tile
SECOND = [64, 65, 67, 68, 70, 71, 73, 74, 76, 79]  # and in the ragged one


def _build():
    rng = random.Random(0x12B)
    coeffs = [rng.randrange(1, B.R) for _ in range(T)]
    sks = [TC.poly_evaluate(coeffs, i + 1) for i in range(N_SHARES)]
    pks = [B.g1_mul(B.G1_GEN, s) for s in sks]
    r, h = rng.randrange(1, B.R), rng.randrange(1, B.R)
    u = B.g1_mul(B.G1_GEN, r)
    H = B.g2_mul(B.G2_GEN, h)
    w = B.g2_mul(H, r)
    shares = [B.g1_compress(B.g1_mul(u, s)) for s in sks]
    special = [p for tag, p in C.subgroup_cases() if not tag.startswith("G1")]
    assert len(special) == len(FIRST) == len(SECOND) == 10
    for place, pt in zip(FIRST + SECOND, special + special[::-1]):
        shares[place] = B.g1_compress(pt)
    shares[5] = B.g1_compress(B.g1_mul(u, (sks[5] + 1) % B.R))
    valid = [j for j in range(N_SHARES) if j not in FIRST + SECOND + [5]]
    signs = {j: (shares[j][0] >> 5) & 1 for j in valid}
    for tile in (range(64), range(64, N_SHARES)):
        assert {signs[j] for j in tile if j in signs} == {0, 1}     # both y signs in both tiles
    pairing = [5] + [next(j for j in valid if signs[j] == s) for s in (0, 1)]
    status = []
    for j, c in enumerate(shares):
        try:
            pt = B.g1_decompress(c)
        except B.DecodeError:
            status.append("DECODE_ERR")
            continue
        ok = TC.verify_decryption_share_h(pks[j], pt, H, w) if j in pairing else pt == B.g1_mul(u, sks[j])
        status.append("ACCEPT" if ok else "REJECT")
    good = [(j, B.g1_decompress(shares[j])) for j in range(N_SHARES) if status[j] == "ACCEPT"]
    g = B.g1_compress(TC.interpolate(T, good, 1))
    assert g == B.g1_compress(B.g1_mul(u, coeffs[0]))
    return dict(pk=[B.g1_compress(p) for p in pks], H=B.g2_compress(H), w=B.g2_compress(w), shares=shares,
                status=status, g=g)


@pytest.fixture(scope="module")
def case():
    return _build()


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    c.set_exact_below(0)
    yield c
    c.close()


def _run(ctx, case, mode):
    ctx.set_verify_mode(mode)
    ks, bad = ctx.keyset_load(case["pk"])
    assert bad == 0
    n = N_SHARES
    idx = np.arange(n, dtype=np.uint32)
    off = np.array([0, n], dtype=np.uint32)
    d = {k: ctx.dev_alloc(sz) for k, sz in (("H", 96), ("w", 96), ("idx", 4 * n), ("sh", 48 * n), ("st", 4 * n),
                                             ("g", 48), ("c", 4))}
    try:
        ctx.dev_upload(d["idx"], idx)
        ctx.dev_upload(d["H"], np.frombuffer(case["H"], np.uint8))
        ctx.dev_upload(d["w"], np.frombuffer(case["w"], np.uint8))
        ctx.dev_upload(d["sh"], np.frombuffer(b"".join(case["shares"]), np.uint8))
        ctx._check(ctx.lib.hbtc_verify_dec_shares_dev(ctx.h, ks, 1, d["H"], d["w"], N._ptr(off), d["idx"], d["sh"],
                                                      d["st"]), "verify")
        ctx._check(ctx.lib.hbtc_combine_dec_verified_dev(ctx.h, 1, N._ptr(off), d["idx"], d["sh"], d["st"], T,
                                                         d["g"], d["c"]), "combine")
        ctx.sync()
        st, g, c = np.empty(n, np.int32), np.empty(48, np.uint8), np.empty(1, np.int32)
        ctx.dev_download(st, d["st"])
        ctx.dev_download(g, d["g"])
        ctx.dev_download(c, d["c"])
    finally:
        for p in d.values():
            ctx.dev_free(p)
        ctx.set_verify_mode(N.MODE_RLC)
    return [N.STATUS_NAMES[int(s)] for s in st], bytes(g), int(c[0])


def test_reference_covers_every_kind(case):
    st = case["status"]
    assert st[5] == "REJECT"
    assert [st[j] for j in FIRST + SECOND] == ["DECODE_ERR"] * 20
    assert st.count("ACCEPT") == N_SHARES - 21


def test_batched_path_matches_the_oracle(ctx, case):
    st, g, c = _run(ctx, case, N.MODE_RLC)
    assert [st[j] for j in FIRST + SECOND] == ["DECODE_ERR"] * 20
    assert st == case["status"]
    assert c == N.ACCEPT and g == case["g"]


def test_batched_path_matches_the_per_share_mode(ctx, case):
    assert _run(ctx, case, N.MODE_RLC) == _run(ctx, case, N.MODE_PER_SHARE)
