"""k_rlc_items with its x-adic multiplication on the redundant 13 x 30 form (curve.h
xadic_mul_sac8_w), through the public API: one ciphertext of 80 DecryptionShares (a full tile and a
ragged tile of 16) with exact_below = 0, so every share takes the batched path, at 64- and 128-bit RLC
scalars.  Cases: all valid; one wrong share in each tile; a sender repeated inside a tile; a share at
infinity; a share with a bad encoding.

Reference: oracle/ -- PublicKeyShare::verify_decryption_share (two pairings) for the wrong shares, the
share at infinity and one valid share, share == sk_i u for the other valid ones, G1Compressed::
into_affine for the bad encoding, PublicKeySet::decrypt's interpolation over the first t accepted
shares for the combined point.  The per-share mode (one pairing check per share, 12 x 32 arithmetic
throughout) must give the same statuses and the same point.

A wrong S_i is not caught by statuses alone: its tile's group check fails, the tile falls back to exact
checks and the statuses stay right.  So every call's number of exact leaf checks (rlc_last_leaves) must
be the one the 12 x 32 item pass gives for the same call: LEAVES below, measured on a build with
HBTC_FQ_RR=2.  An all-valid call has none."""
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

N_SHARES = 80
T = 24
WRONG = (5, 70)          # one in each tile
REPEAT = (12, 30)        # position 30 carries sender 12's share again
INF_AT = 40
BROKEN_AT = 66
CASES = ("valid", "wrong", "repeat", "infinity", "badenc")
# exact leaf checks per call on the HBTC_FQ_RR=2 build, the same at 64 and 128 bits: a lone wrong share of
# a tile is located by the tile's weighted sums (none); the later copy of a repeated sender takes the exact
# path (one)
LEAVES = {"valid": 0, "wrong": 0, "repeat": 1, "infinity": 0, "badenc": 0}
INF48 = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def base():
    rng = random.Random(0x13B)
    coeffs = [rng.randrange(1, B.R) for _ in range(T)]
    sks = [TC.poly_evaluate(coeffs, i + 1) for i in range(N_SHARES)]
    pks = [B.g1_mul(B.G1_GEN, s) for s in sks]
    r, h = rng.randrange(1, B.R), rng.randrange(1, B.R)
    u = B.g1_mul(B.G1_GEN, r)
    H = B.g2_mul(B.G2_GEN, h)
    w = B.g2_mul(H, r)
    shares = [B.g1_compress(B.g1_mul(u, s)) for s in sks]
    wrong = {j: B.g1_compress(B.g1_mul(u, (sks[j] + 1 + j) % B.R)) for j in WRONG}
    # the pairing verdicts, once: the wrong shares, the share at infinity, one valid share
    verdict = {(j, c): TC.verify_decryption_share_h(pks[j], B.g1_decompress(c), H, w)
               for j, c in [(j, wrong[j]) for j in WRONG] + [(INF_AT, INF48), (0, shares[0])]}
    return dict(sks=sks, u=u, pk=[B.g1_compress(p) for p in pks], H=B.g2_compress(H), w=B.g2_compress(w),
                shares=shares, wrong=wrong, verdict=verdict, g=B.g1_compress(B.g1_mul(u, coeffs[0])))


def _case(base, name):
    """-> (idx, shares, oracle statuses, oracle combined point)"""
    idx, shares = list(range(N_SHARES)), list(base["shares"])
    if name == "wrong":
        for j in WRONG:
            shares[j] = base["wrong"][j]
    elif name == "repeat":
        idx[REPEAT[1]], shares[REPEAT[1]] = REPEAT[0], shares[REPEAT[0]]
    elif name == "infinity":
        shares[INF_AT] = INF48
    elif name == "badenc":
        shares[BROKEN_AT] = bytes([shares[BROKEN_AT][0] & 0x7F]) + shares[BROKEN_AT][1:]
    status = []
    for j, (i, c) in enumerate(zip(idx, shares)):
        try:
            pt = B.g1_decompress(c)
        except B.DecodeError:
            status.append(N.DECODE_ERR)
            continue
        ok = base["verdict"][(i, c)] if (i, c) in base["verdict"] else pt == B.g1_mul(base["u"], base["sks"][i])
        status.append(N.ACCEPT if ok else N.REJECT)
    good = [(i, B.g1_decompress(c)) for i, c, s in zip(idx, shares, status) if s == N.ACCEPT]
    assert len({i for i, _ in good[:T]}) == T
    return idx, shares, status, B.g1_compress(TC.interpolate(T, good, 1))


@pytest.fixture(scope="module")
def env(base):
    ctx = N.Context(0)
    ctx.set_exact_below(0)
    ctx.set_sender_tracking(False)
    ks, bad = ctx.keyset_load(base["pk"])
    assert bad == 0
    yield ctx, ks
    ctx.set_rlc_bits(128)
    ctx.close()


def _run(env, base, idx, shares, mode, bits):
    ctx, ks = env
    ctx.set_verify_mode(mode)
    ctx.set_rlc_bits(bits)
    try:
        st = ctx.verify_dec_shares(ks, [base["H"]], [base["w"]], [N_SHARES], idx, shares)
        leaves = ctx.rlc_last_leaves() if mode == N.MODE_RLC else None
        g, cst = ctx.combine_dec_verified([N_SHARES], idx, shares, st, T)
    finally:
        ctx.set_verify_mode(N.MODE_RLC)
        ctx.set_rlc_bits(128)
    return [int(s) for s in st], g[0], int(cst[0]), leaves


def test_the_reference_covers_every_kind(base):
    assert all(base["verdict"][(j, base["wrong"][j])] is False for j in WRONG)
    assert base["verdict"][(INF_AT, INF48)] is False and base["verdict"][(0, base["shares"][0])] is True
    want = {"valid": {}, "wrong": {j: N.REJECT for j in WRONG}, "repeat": {}, "infinity": {INF_AT: N.REJECT},
            "badenc": {BROKEN_AT: N.DECODE_ERR}}
    for name in CASES:
        _, _, status, g = _case(base, name)
        assert status == [want[name].get(j, N.ACCEPT) for j in range(N_SHARES)], name
        assert g == base["g"], name


@pytest.mark.parametrize("bits", (64, 128))
@pytest.mark.parametrize("name", CASES)
def test_batched_path_matches_the_oracle_and_the_per_share_mode(env, base, name, bits):
    idx, shares, status, g = _case(base, name)
    st, got_g, cst, leaves = _run(env, base, idx, shares, N.MODE_RLC, bits)
    print("leaves", name, bits, leaves)
    assert st == status
    assert cst == N.ACCEPT and got_g == g
    assert leaves == LEAVES[name], (name, bits, leaves)
    ref = _run(env, base, idx, shares, N.MODE_PER_SHARE, bits)
    assert (st, got_g, cst) == ref[:3]
