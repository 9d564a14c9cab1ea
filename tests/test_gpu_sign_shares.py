"""hbtc_sign_shares (SecretKeyShare::sign, batched under one secret key: the candidate draw, then
k_sig_share's cofactor clearing and psi-split multiplication on lane pairs) on the GPU.

All-items comparisons go against the library's own calls (hash_g2_batch on the GPU, g2_mul);
oracle/threshold_crypto.sign checks four (sk, msg) pairs; the round trip takes the produced shares
through verify_sig_shares, coin_decide, combine_sigs and verify_sigs.  Lane-pair code has no host
form, so these tests are k_sig_share's only check."""
import json
import os
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
G2_INF = bytes([0xC0]) + bytes(95)
X_ABS = 0xd201000000010000  # |x|, the BLS12-381 parameter
X2 = X_ABS * X_ABS          # sk = sum d_j |x|^j: x^2 is the digit d2's weight
assert X2 == 0xac45a4010001a4020000000100000000
# 1, 2, r - 1; 0, r (infinity), r + 1, 2^256 - 1 (reduced first); around x^2 (the psi split's
# digits d0, d1 all ones | d2 = 1) and its digit edges |x|, |x|^2 - 1
EDGE_SCALARS = [1, 2, R - 1, 0, R, R + 1, (1 << 256) - 1, X2 - 1, X2, X2 + 1, X_ABS, X_ABS * X_ABS - 1]
LENGTHS = [0, 1, 64, 65, 135, 136, 137]  # 136 = the SHA3-256 rate
COIN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_coin.json")))
NONCE = bytes.fromhex(COIN["nonce"])


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def _msgs(rng, n):
    """n messages: every length of LENGTHS in turn, the coin nonce of the fixture among them."""
    out = [bytes(rng.randrange(256) for _ in range(LENGTHS[i % len(LENGTHS)])) for i in range(n)]
    if n > 1:
        out[n // 2] = NONCE
    return out


def _composed(ctx, sk, msgs):
    """hash_g2_batch + g2_mul: the two calls hbtc_sign_shares replaces."""
    H = ctx.hash_g2_batch(msgs)
    out, st = ctx.g2_mul(H, [sk] * len(msgs))
    assert not st.any()
    return [bytes(out[96 * i:96 * i + 96]) for i in range(len(msgs))], H


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_bytes_equal_hash_and_g2_mul(ctx, n):
    """32 items fill a wave of lane pairs: 31 | 32 | 33 is the wave edge, 65 a third block."""
    rng = random.Random(900 + n)
    sk = rng.randrange(1, R)
    msgs = _msgs(rng, n)
    sigs, H = ctx.sign_shares(sk, msgs)
    want_sigs, want_H = _composed(ctx, sk, msgs)
    assert H == want_H
    assert sigs == want_sigs
    if n > 1:
        assert H[n // 2] == bytes.fromhex(COIN["H"])  # the fixture's hash_g2(nonce)


def test_every_length_and_the_fixture_nonce(ctx):
    rng = random.Random(7)
    sk = rng.randrange(1, R)
    msgs = [bytes(rng.randrange(256) for _ in range(n)) for n in LENGTHS] + [NONCE]
    sigs, H = ctx.sign_shares(sk, msgs)
    want_sigs, want_H = _composed(ctx, sk, msgs)
    assert (sigs, H) == (want_sigs, want_H)


def test_without_the_hash_output(ctx):
    """out_H_c96 = NULL: the signatures alone, the same bytes."""
    rng = random.Random(8)
    sk = rng.randrange(1, R)
    msgs = _msgs(rng, 33)
    sigs, H = ctx.sign_shares(sk, msgs, want_H=False)
    assert H is None
    assert sigs == ctx.sign_shares(sk, msgs)[0] == _composed(ctx, sk, msgs)[0]


@pytest.mark.parametrize("sk", EDGE_SCALARS, ids=lambda s: hex(s)[:20])
def test_edge_scalars(ctx, sk):
    rng = random.Random(11)
    msgs = _msgs(rng, 3)
    sigs, H = ctx.sign_shares(sk, msgs)
    want_sigs, want_H = _composed(ctx, sk, msgs)
    assert H == want_H  # H is written whatever the scalar
    assert sigs == want_sigs
    if sk % R == 0:
        assert sigs == [G2_INF] * 3


def test_against_the_restatement(ctx):
    """oracle.sign on four (sk, msg) pairs."""
    rng = random.Random(12)
    pairs = [(rng.randrange(1, R), NONCE), (R - 1, b""), (X2, bytes(range(137))),
             (rng.randrange(1, R), bytes(65))]
    for sk, msg in pairs:
        sigs, H = ctx.sign_shares(sk, [msg])
        assert H[0] == B.g2_compress(TC.hash_g2(msg))
        assert sigs[0] == B.g2_compress(TC.sign(sk, msg))


def test_argument_checks(ctx):
    lib, null = ctx.lib, N._ptr(None)
    sk = np.zeros(32, np.uint8)
    sig = np.zeros(96, np.uint8)
    off0 = np.zeros(2, np.uint32)
    assert lib.hbtc_sign_shares(ctx.h, 0, null, null, null, null, null) == 0
    assert lib.hbtc_sign_shares(ctx.h, 1, null, null, N._ptr(off0), N._ptr(sig), null) == -1
    assert lib.hbtc_sign_shares(ctx.h, 1, N._ptr(sk), null, null, N._ptr(sig), null) == -1
    assert lib.hbtc_sign_shares(ctx.h, 1, N._ptr(sk), null, N._ptr(off0), null, null) == -1
    bad_off = np.array([1, 1], np.uint32)
    assert lib.hbtc_sign_shares(ctx.h, 1, N._ptr(sk), N._ptr(sk), N._ptr(bad_off), N._ptr(sig), null) == -1
    off1 = np.array([0, 1], np.uint32)  # a message byte, but no message buffer
    assert lib.hbtc_sign_shares(ctx.h, 1, N._ptr(sk), null, N._ptr(off1), N._ptr(sig), null) == -1
    # the empty message is a message
    assert lib.hbtc_sign_shares(ctx.h, 1, N._ptr(sk), null, N._ptr(off0), N._ptr(sig), null) == 0
    assert bytes(sig) == G2_INF  # sk = 0


def test_round_trip_through_the_coin(ctx):
    """N = 4, t = 1: shares sk_i = f(i + 1) of a random degree-1 f; four sign_shares calls over
    three nonces; every share verifies, the coin is decided, and its parity is that of the combined
    signature, which passes under the master key f(0) G1."""
    rng = random.Random(13)
    n_nodes, t = 4, 1
    f = [rng.randrange(1, R) for _ in range(t + 1)]
    ev = ctx.fr_poly_eval([f], list(range(1, n_nodes + 1)))
    sks = [int.from_bytes(ev[0, j].tobytes(), "little") for j in range(n_nodes)]
    assert sks == [(f[0] + f[1] * x) % R for x in range(1, n_nodes + 1)]
    out, st = ctx.g1_mul(G1, sks + [f[0]])
    assert not st.any()
    pks = [bytes(out[48 * i:48 * i + 48]) for i in range(n_nodes)]
    master = bytes(out[48 * n_nodes:48 * n_nodes + 48])
    ks, bad = ctx.keyset_load(pks)
    assert bad == 0
    try:
        ctx.keyset_set_master(ks, master)
        nonces = [NONCE, b"Nonce for Honey Badger @1:0:0", b""]
        per_node = [ctx.sign_shares(sk, nonces) for sk in sks]
        Hs = per_node[0][1]
        assert all(p[1] == Hs for p in per_node)
        counts = [n_nodes] * len(nonces)
        idx = list(range(n_nodes)) * len(nonces)
        sigs = [per_node[i][0][k] for k in range(len(nonces)) for i in range(n_nodes)]
        vst = ctx.verify_sig_shares(ks, Hs, counts, idx, sigs)
        assert (np.asarray(vst) == N.ACCEPT).all()
        st, csig, par, cst = ctx.coin_decide(ks, Hs, counts, idx, sigs, t + 1)
        assert (np.asarray(st) == N.ACCEPT).all() and (np.asarray(cst) == N.ACCEPT).all()
        comb, cpar, cbst = ctx.combine_sigs(counts, idx, sigs, t + 1)
        assert not np.asarray(cbst).any()
        assert list(par) == list(cpar) and csig == comb
        mst = ctx.verify_sigs([master] * len(nonces), Hs, comb)
        assert (np.asarray(mst) == N.ACCEPT).all()
        # the combined signature is the master key's own signature
        msig, _ = ctx.sign_shares(f[0], nonces)
        assert msig == comb
    finally:
        ctx.keyset_free(ks)
