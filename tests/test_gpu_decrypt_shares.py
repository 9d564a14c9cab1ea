"""hbtc_decrypt_shares (SecretKeyShare::decrypt_share, batched under one secret key share: H =
hash_g1_g2(u, v), Ciphertext::verify and sk u back to back on the device) on the GPU.

All-items comparisons go against the library's own calls (hash_g1_g2_batch on the GPU,
verify_ciphertexts, g1_mul) in the three verification regimes; oracle/threshold_crypto.decrypt_share
checks four items; the round trip takes the produced shares and H through threshold_decrypt; and
hbtc_decrypt, whose stages the new call shares, must still give v XOR hash_bytes(share)."""
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
G1_INF = bytes([0xC0]) + bytes(47)
G2_INF = bytes([0xC0]) + bytes(95)
X_ABS = 0xd201000000010000
X2 = X_ABS * X_ABS
EDGE_SCALARS = [1, 2, R - 1, 0, R, R + 1, (1 << 256) - 1, X2 - 1, X2, X2 + 1, X_ABS, X_ABS * X_ABS - 1]
V_LENGTHS = [0, 1, 64, 65, 137]  # 64 | 65: hash_g1_g2 hashes a longer v first
CODEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec.json")))
BAD_G1 = [bytes.fromhex(e["enc"]) for e in CODEC["g1_bad"]]
BAD_G2 = [bytes.fromhex(e["enc"]) for e in CODEC["g2_bad"]]
# (verify mode, exact_below): the pair batch; the exact checks of a small RLC call (the default
# threshold); per-share mode
REGIMES = {"pair_batch": (N.MODE_RLC, 0), "rlc_small_exact": (N.MODE_RLC, 256),
           "per_share": (N.MODE_PER_SHARE, 256)}


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


@pytest.fixture
def regime(ctx, request):
    mode, below = REGIMES[request.param]
    ctx.set_verify_mode(mode)
    ctx.set_exact_below(below)
    yield request.param
    ctx.set_verify_mode(N.MODE_RLC)
    ctx.set_exact_below(256)


@pytest.fixture(scope="module")
def pool(ctx):
    """130 valid ciphertexts (u, v, w) under one key, every v length in turn, made once."""
    rng = random.Random(2024)
    sk = rng.randrange(1, R)
    pk, st = ctx.g1_mul(G1, [sk])
    assert not st.any()
    n = 130
    msgs = [bytes(rng.randrange(256) for _ in range(V_LENGTHS[i % len(V_LENGTHS)])) for i in range(n)]
    cts, st = ctx.encrypt(bytes(pk), [rng.randrange(1, R) for _ in range(n)], msgs)
    assert not st.any()
    return sk, bytes(pk), cts, msgs


def _check(ctx, sk, cts):
    """Every assertion of the issue for one call; returns (shares, H, status)."""
    us, vs, ws = [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]
    shares, H, st = ctx.decrypt_shares(sk, us, vs, ws)
    want_H = ctx.hash_g1_g2_batch(us, vs)
    assert H == want_H
    want_st = ctx.verify_ciphertexts(us, want_H, ws)
    assert list(st) == list(want_st)
    acc = [i for i in range(len(cts)) if st[i] == N.ACCEPT]
    if acc:
        g, gst = ctx.g1_mul([us[i] for i in acc], [sk] * len(acc))
        assert not gst.any()
        for j, i in enumerate(acc):
            assert shares[i] == bytes(g[48 * j:48 * j + 48]), i
    # the raw output of the other items is zero-filled
    raw = _raw(ctx, sk, us, vs, ws)
    for i in range(len(cts)):
        if st[i] != N.ACCEPT:
            assert shares[i] is None and raw[i] == bytes(48), i
        else:
            assert raw[i] == shares[i]
    return shares, H, st


def _raw(ctx, sk, us, vs, ws):
    """The share bytes as the C call writes them (into a buffer of 0xff)."""
    buf, off = N._msg_batch(vs)
    n = len(us)
    u, w = N._join(us, 48), N._join(ws, 96)
    g = np.full(48 * n, 0xff, np.uint8)
    st = np.zeros(n, np.int32)
    k = np.frombuffer(int(sk).to_bytes(32, "little"), np.uint8).copy()
    assert ctx.lib.hbtc_decrypt_shares(ctx.h, n, N._ptr(k), N._ptr(u), N._ptr(buf), N._ptr(off), N._ptr(w),
                                       N._ptr(g), N._ptr(None), N._ptr(st)) == 0  # out_H_c96 = NULL
    return [bytes(g[48 * i:48 * i + 48]) for i in range(n)]


def _flip_v(ct):
    u, v, w = ct
    return (u, bytes([v[0] ^ 1]) + v[1:], w)


@pytest.mark.parametrize("regime", list(REGIMES), indirect=True)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_sizes(ctx, pool, regime, n):
    """Pair batches are 64-item groups: 63 | 64 | 65, and 130 = two full groups and a tail.  Bad
    items at 0, 63, 64 and last, between good neighbours: w swapped for another ciphertext's
    (REJECT), a byte of v flipped (REJECT through H)."""
    sk, _, pool_cts, _ = pool
    cts = list(pool_cts[:n])
    bad = sorted(i for i in {0, 63, 64, n - 1} if i < n) if n > 1 else []
    for j, i in enumerate(bad):
        if j % 2 == 0 or not cts[i][1]:  # an empty v has no byte to flip
            cts[i] = (cts[i][0], cts[i][1], pool_cts[(i + 7) % 130][2])
        else:
            cts[i] = _flip_v(cts[i])
    _, _, st = _check(ctx, sk, cts)
    for i in range(n):
        assert st[i] == (N.REJECT if i in bad else N.ACCEPT), i


@pytest.mark.parametrize("regime", list(REGIMES), indirect=True)
@pytest.mark.parametrize("rot", [0, 4, 8, 12])
def test_bad_encodings_between_good_neighbours(ctx, pool, regime, rot):
    """Every bad G1 encoding of tests/golden/codec.json as u and every bad G2 encoding as w
    (DECODE_ERR), u = w = infinity, a swapped w and a flipped v, at 0, 63, 64, last and odd
    positions in between; the four rotations put every kind on one of 0, 63, 64, last."""
    sk, _, pool_cts, _ = pool
    n = 130
    cts = list(pool_cts)
    kinds = [("u", b) for b in BAD_G1] + [("w", b) for b in BAD_G2] + [("inf", None), ("swap", None),
                                                                      ("flip", None)]
    assert len(kinds) == 13
    kinds = kinds[rot:] + kinds[:rot]
    positions = [0, 63, 64, n - 1] + list(range(11, 11 + 2 * (len(kinds) - 4), 2))
    want = {}
    for (kind, enc), i in zip(kinds, positions):
        u, v, w = cts[i]
        if kind == "u":
            cts[i], want[i] = (enc, v, w), N.DECODE_ERR
        elif kind == "w":
            cts[i], want[i] = (u, v, enc), N.DECODE_ERR
        elif kind == "inf":
            cts[i], want[i] = (G1_INF, v, G2_INF), None  # whatever verify_ciphertexts says
        elif kind == "swap":
            cts[i], want[i] = (u, v, pool_cts[(i + 7) % n][2]), N.REJECT
        else:
            j = i if v else i + 1  # an item with a byte to flip (position 0 has an empty v)
            cts[j], want[j] = _flip_v(cts[j]), N.REJECT
    shares, _, st = _check(ctx, sk, cts)
    for i in range(n):
        if i in want:
            if want[i] is not None:
                assert st[i] == want[i], i
        else:
            assert st[i] == N.ACCEPT, i
    inf_pos = positions[[k for k, _ in kinds].index("inf")]
    if st[inf_pos] == N.ACCEPT:  # e(O, H) == e(G1, O): sk O = O
        assert shares[inf_pos] == G1_INF


@pytest.mark.parametrize("regime", ["pair_batch", "per_share"], indirect=True)
@pytest.mark.parametrize("sk", EDGE_SCALARS, ids=lambda s: hex(s)[:20])
def test_edge_scalars(ctx, pool, regime, sk):
    _, _, pool_cts, _ = pool
    shares, _, st = _check(ctx, sk, pool_cts[2:5])
    assert (st == N.ACCEPT).all()
    if sk % R == 0:
        assert shares == [G1_INF] * 3


def test_against_the_restatement(ctx, pool):
    """oracle.decrypt_share on four items, one of them rejected."""
    sk, _, pool_cts, _ = pool
    cts = [pool_cts[1], pool_cts[2], (pool_cts[3][0], pool_cts[3][1], pool_cts[4][2]), pool_cts[4]]
    shares, H, st = ctx.decrypt_shares(sk, [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts])
    for i, (u, v, w) in enumerate(cts):
        pu, pw = B.g1_decompress(u), B.g2_decompress(w)
        assert H[i] == B.g2_compress(TC.hash_g1_g2(pu, v))
        want = TC.decrypt_share(sk, (pu, v, pw))
        assert shares[i] == (None if want is None else B.g1_compress(want)), i
    assert list(st) == [N.ACCEPT, N.ACCEPT, N.REJECT, N.ACCEPT]


def test_argument_checks(ctx):
    lib, null = ctx.lib, N._ptr(None)
    sk, u, w = np.zeros(32, np.uint8), np.zeros(48, np.uint8), np.zeros(96, np.uint8)
    g, st = np.zeros(48, np.uint8), np.zeros(1, np.int32)
    off0, off1, bad = np.zeros(2, np.uint32), np.array([0, 1], np.uint32), np.array([1, 1], np.uint32)
    p = N._ptr
    assert lib.hbtc_decrypt_shares(ctx.h, 0, null, null, null, null, null, null, null, null) == 0
    full = [p(sk), p(u), null, p(off0), p(w), p(g), null, p(st)]
    for hole in (0, 1, 3, 4, 5, 7):  # sk, u, v_offsets, w, out_share, status
        args = list(full)
        args[hole] = null
        assert lib.hbtc_decrypt_shares(ctx.h, 1, *args) == -1, hole
    assert lib.hbtc_decrypt_shares(ctx.h, 1, p(sk), p(u), null, p(off1), p(w), p(g), null, p(st)) == -1
    assert lib.hbtc_decrypt_shares(ctx.h, 1, p(sk), p(u), p(sk), p(bad), p(w), p(g), null, p(st)) == -1
    # all-zero u and w do not decode: the call succeeds, the item is DECODE_ERR, the share zeros
    g[:] = 0xff
    assert lib.hbtc_decrypt_shares(ctx.h, 1, *full) == 0
    assert st[0] == N.DECODE_ERR and not g.any()


def test_round_trip_through_threshold_decrypt(ctx):
    """N = 4, t = 1: three messages encrypted to the master key; each node's decrypt_shares; the
    produced shares and the returned H give the messages back through threshold_decrypt."""
    rng = random.Random(77)
    n_nodes, t = 4, 1
    f = [rng.randrange(1, R) for _ in range(t + 1)]
    ev = ctx.fr_poly_eval([f], list(range(1, n_nodes + 1)))
    sks = [int.from_bytes(ev[0, j].tobytes(), "little") for j in range(n_nodes)]
    out, st = ctx.g1_mul(G1, sks + [f[0]])
    assert not st.any()
    pks = [bytes(out[48 * i:48 * i + 48]) for i in range(n_nodes)]
    master = bytes(out[48 * n_nodes:48 * n_nodes + 48])
    msgs = [b"the first proposal", bytes(range(200)), b"x"]
    cts, st = ctx.encrypt(master, [rng.randrange(1, R) for _ in msgs], msgs)
    assert not st.any()
    us, vs, ws = [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]
    per_node = [ctx.decrypt_shares(sk, us, vs, ws) for sk in sks]
    H = per_node[0][1]
    for shares, Hn, stn in per_node:
        assert Hn == H and (stn == N.ACCEPT).all()
    assert (np.asarray(ctx.prepare_g2(H)) == N.ACCEPT).all()
    ctx.unprepare_g2(H)
    ks, bad = ctx.keyset_load(pks)
    assert bad == 0
    try:
        counts = [n_nodes] * len(msgs)
        idx = list(range(n_nodes)) * len(msgs)
        shares = [per_node[i][0][k] for k in range(len(msgs)) for i in range(n_nodes)]
        sst, plain, _, cst = ctx.threshold_decrypt(ks, H, ws, counts, idx, shares, t + 1, vs)
        assert (np.asarray(sst) == N.ACCEPT).all() and (np.asarray(cst) == N.ACCEPT).all()
        assert plain == msgs
    finally:
        ctx.keyset_free(ks)


@pytest.mark.parametrize("regime", ["pair_batch", "per_share"], indirect=True)
def test_decrypt_still_pads_with_the_same_share(ctx, pool, regime):
    """hbtc_decrypt runs the stages the new call shares: on the same ciphertexts (one rejected) its
    plaintexts are v XOR hash_bytes(share) of the new call's shares."""
    sk, _, pool_cts, msgs = pool
    cts = list(pool_cts[:70])
    cts[5] = (cts[5][0], cts[5][1], pool_cts[99][2])
    us, vs, ws = [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]
    shares, _, st = ctx.decrypt_shares(sk, us, vs, ws)
    plain, dst = ctx.decrypt(sk, us, ws, vs)
    assert list(dst) == list(st)
    ok = [i for i in range(len(cts)) if st[i] == N.ACCEPT]
    assert len(ok) == len(cts) - 1
    want = N.xor_hash_bytes_batch([shares[i] for i in ok], [vs[i] for i in ok])
    assert [plain[i] for i in ok] == [bytes(x) for x in want] == [msgs[i] for i in ok]
    assert plain[5] is None
