"""k_rlc_decode with its square root on 30-bit limbs, through the public API: one ciphertext of 70
DecryptionShares (a full tile and a ragged tile of 6) through hbtc_verify_dec_shares and
hbtc_combine_dec_verified_dev with exact_below = 0, so every share takes the batched path.

The shares hold valid shares of both y signs, a wrong share, x >= p, an x whose x^3 + 4 is a
non-residue, a cleared compression flag, a valid and an invalid infinity encoding, (0, 2) of order
3 and an on-curve point outside G1.

Reference: oracle/ -- G1Compressed::into_affine for the decode verdicts, PublicKeyShare::
verify_decryption_share (two pairings) for the wrong share, the infinity share and four valid
ones of both signs, share == sk_i u for the other valid ones (the same statement, by the
pairing's non-degeneracy), PublicKeySet::decrypt's interpolation over the first t accepted shares
for the combined point.  The per-share mode (HBTC_MODE_PER_SHARE: the 12 x 32 decode of
k_g1_decode, one pairing check per share) must give the same statuses and the same point."""
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

N_SHARES, N_KEYS = 70, 70
T = 24


def _build():
    rng = random.Random(0x11A)
    coeffs = [rng.randrange(1, B.R) for _ in range(T)]
    sks = [TC.poly_evaluate(coeffs, i + 1) for i in range(N_KEYS)]
    pks = [B.g1_mul(B.G1_GEN, s) for s in sks]
    r, h = rng.randrange(1, B.R), rng.randrange(1, B.R)
    u = B.g1_mul(B.G1_GEN, r)
    H = B.g2_mul(B.G2_GEN, h)
    w = B.g2_mul(H, r)
    shares = [B.g1_compress(B.g1_mul(u, s)) for s in sks]
    want = [None] * N_SHARES          # None: valid by construction
    signs = [(c[0] >> 5) & 1 for c in shares]
    assert 0 in signs and 1 in signs  # both y signs among the valid shares
    # the special shares, in both tiles (positions 64..69 are the ragged tile)
    shares[5] = B.g1_compress(B.g1_mul(u, (sks[5] + 1) % B.R))
    want[5] = "pairing"
    big = bytearray((B.P + 9).to_bytes(48, "big"))
    big[0] |= 0x80
    shares[11] = bytes(big)
    while True:
        x = rng.randrange(B.P)
        if B.fq_sqrt((x * x * x + 4) % B.P) is None:
            break
    nr = bytearray(x.to_bytes(48, "big"))
    nr[0] |= 0x80
    shares[17] = bytes(nr)
    cleared = bytearray(shares[23])
    cleared[0] &= 0x7F
    shares[23] = bytes(cleared)
    shares[30] = B.g1_compress(None)
    want[30] = "pairing"
    inf = bytearray(B.g1_compress(None))
    inf[40] = 0x10
    shares[31] = bytes(inf)
    shares[66] = B.g1_compress((0, 2))
    while True:
        pt = B.g1_point_from_x(rng.randrange(B.P), bool(rng.getrandbits(1)))
        if pt and not B.g1_in_subgroup(pt):
            break
    shares[68] = B.g1_compress(pt)
    first = {s: signs.index(s) for s in (0, 1)}
    for j in (first[0], first[1], 64, 69):
        if want[j] is None:
            want[j] = "pairing"
    status = []
    for j, c in enumerate(shares):
        try:
            pt = B.g1_decompress(c)
        except B.DecodeError:
            status.append("DECODE_ERR")
            continue
        if want[j] == "pairing":
            ok = TC.verify_decryption_share_h(pks[j], pt, H, w)
        else:
            ok = pt == B.g1_mul(u, sks[j])
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
    assert st[5] == "REJECT" and st[30] == "REJECT"
    assert [st[j] for j in (11, 17, 23, 31, 66, 68)] == ["DECODE_ERR"] * 6
    assert st.count("ACCEPT") == N_SHARES - 8 and st[64] == st[69] == "ACCEPT"


def test_batched_path_matches_the_oracle(ctx, case):
    st, g, c = _run(ctx, case, N.MODE_RLC)
    assert st == case["status"]
    assert c == N.ACCEPT and g == case["g"]


def test_batched_path_matches_the_per_share_mode(ctx, case):
    assert _run(ctx, case, N.MODE_RLC) == _run(ctx, case, N.MODE_PER_SHARE)
