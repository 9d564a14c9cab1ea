"""hbtc_verify_signed_msgs on the GPU: PublicKey::verify of DynamicHoneyBadger's signed votes and
key-generation messages, hashed and grouped by signer (hbtc_sv.hip).

Every test runs the grouped path (hbtc_set_exact_below(ctx, 0)); the ragged case repeats with the
default setting (the exact route below its threshold, the composed pair-batch route above it) and
in per-share mode, to show equal decisions.
Valid signatures come from hbtc_sign_shares, one call per signer's secret key; a bad signature
that is still a subgroup point is another message's or another signer's.  Expected statuses are
known by construction and are also what hbtc_verify_sigs gives on
(pk, hbtc_hash_g2_batch_gpu(msg), sig) per item."""
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
CODEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec.json")))
G2_BAD = {e["name"]: bytes.fromhex(e["enc"]) for e in CODEC["g2_bad"]}
LENGTHS = [9, 64, 65, 128, 135, 136, 137]  # 136 = the SHA3-256 rate; 128: a vote's size
N_KEYS = 70  # 64-signer tiles and 8-signer sub-tiles both with a remainder


def _ctx(exact_below=0):
    c = N.Context(0)
    if exact_below is not None:
        c.set_exact_below(exact_below)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


def _keys(ctx, rng, n):
    sks = [rng.randrange(1, R) for _ in range(n)]
    out, st = ctx.g1_mul(G1, sks)
    assert not st.any()
    return sks, [bytes(out[48 * i:48 * i + 48]) for i in range(n)]


def _msg(rng, k):
    return bytes(rng.randrange(256) for _ in range(LENGTHS[k % len(LENGTHS)]))


def _interleave(rng, runs):
    """A random merge of the signers' runs: every signer's items keep their order, so item k of a
    signer sits at slot k % 64 of that signer's tile k // 64."""
    left = [len(r) for r in runs]
    at = [0] * len(runs)
    order = []
    live = [j for j, r in enumerate(runs) if r]
    while live:
        j = rng.choice(live)
        order.append((j, at[j]))
        at[j] += 1
        left[j] -= 1
        if not left[j]:
            live.remove(j)
    return order


@pytest.fixture(scope="module")
def ragged(ctx):
    """About 600 items of a 70-key set: runs of 0, 1, 63, 64, 65 and 129 items among the signers,
    the bad items at the first and last slots of item tiles, in signers 0, 7, 8, 63, 64 and 69."""
    rng = random.Random(2024)
    sks, pks = _keys(ctx, rng, N_KEYS)
    lengths = {0: 129, 5: 1, 6: 0, 7: 65, 8: 64, 63: 63, 64: 65, 69: 64}
    runs = []
    for j in range(N_KEYS):
        msgs = [_msg(rng, rng.randrange(7)) for _ in range(lengths.get(j, 2))]
        if j == 69:
            msgs[0] = b""  # the empty message is a message
        sigs = ctx.sign_shares(sks[j], msgs, want_H=False)[0] if msgs else []
        runs.append([[j, m, s, N.ACCEPT] for m, s in zip(msgs, sigs)])

    def other_sig(j, k):  # signer j's valid signature of another message: a subgroup point
        return runs[j][(k + 1) % len(runs[j])][2]

    # signer 0, tiles of 64, 64 and 1 items
    runs[0][0][1] = b"not the signed bytes"                 # the wrong message, first slot
    runs[0][0][3] = N.REJECT
    runs[0][63][2], runs[0][63][3] = G2_INF, N.REJECT         # sigma = infinity, last slot
    runs[0][128][2] = ctx.sign_shares(sks[1], [runs[0][128][1]], want_H=False)[0][0]
    runs[0][128][3] = N.REJECT                                # the wrong signer, a tile of one item
    runs[7][63][2], runs[7][63][3] = G2_BAD["not_in_subgroup"], N.DECODE_ERR   # last slot
    runs[8][0][2], runs[8][0][3] = G2_BAD["x_not_reduced"], N.DECODE_ERR       # first slot
    runs[63][62][2], runs[63][62][3] = other_sig(63, 62), N.REJECT             # last item of a partial tile
    runs[64][64][2] = ctx.sign_shares(sks[65], [runs[64][64][1]], want_H=False)[0][0]
    runs[64][64][3] = N.REJECT                                # the wrong signer, first slot of tile 1
    runs[69][63][2], runs[69][63][3] = other_sig(69, 63), N.REJECT             # last slot
    # an item of nobody: signer[i] = 70
    runs.append([[N_KEYS, b"from a stranger", runs[3][0][2], N.UNKNOWN_SENDER]])
    items = [runs[j][k] for j, k in _interleave(rng, runs)]
    ks, bad = ctx.keyset_load(pks)
    assert bad == 0
    yield {"ks": ks, "pks": pks, "sks": sks, "signer": [i[0] for i in items], "msgs": [i[1] for i in items],
           "sigs": [i[2] for i in items], "want": np.array([i[3] for i in items], np.int32)}
    ctx.keyset_free(ks)


def test_ragged_layout(ctx, ragged):
    r = ragged
    assert 550 <= len(r["signer"]) <= 650 and b"" in r["msgs"]
    st = ctx.verify_signed_msgs(r["ks"], r["signer"], r["msgs"], r["sigs"])
    assert st.tolist() == r["want"].tolist()
    # the same as the composed calls give, item by item (signer 70 has no key to pass them)
    known = [i for i, s in enumerate(r["signer"]) if s < N_KEYS]
    H = ctx.hash_g2_batch([r["msgs"][i] for i in known])
    ref = ctx.verify_sigs([r["pks"][r["signer"][i]] for i in known], H, [r["sigs"][i] for i in known])
    assert st[known].tolist() == np.asarray(ref).tolist()
    assert sorted(set(r["want"].tolist())) == [N.ACCEPT, N.REJECT, N.DECODE_ERR, N.UNKNOWN_SENDER]
    assert (r["want"] != N.ACCEPT).sum() == 9  # every other item, the rest of a failing signer's too


def test_order(ctx, ragged):
    r = ragged
    n = len(r["signer"])
    p = list(range(n))
    random.Random(5).shuffle(p)
    st = ctx.verify_signed_msgs(r["ks"], [r["signer"][i] for i in p], [r["msgs"][i] for i in p],
                                [r["sigs"][i] for i in p])
    assert st.tolist() == r["want"][p].tolist()


def test_other_routes_decide_the_same(ragged):
    """The default context checks a call below its threshold (256 items) exactly and sends a larger
    one through the composed route (hash, then hbtc_verify_sigs' pair batch on the gathered keys);
    per-share mode checks every call exactly: the decisions of the grouped path, each time."""
    r = ragged
    c = _ctx(exact_below=None)
    try:
        ks, _ = c.keyset_load(r["pks"])
        head = 200
        st = c.verify_signed_msgs(ks, r["signer"][:head], r["msgs"][:head], r["sigs"][:head])
        assert st.tolist() == r["want"][:head].tolist()
        st = c.verify_signed_msgs(ks, r["signer"], r["msgs"], r["sigs"])
        assert st.tolist() == r["want"].tolist()
        c.set_verify_mode(N.MODE_PER_SHARE)
        st = c.verify_signed_msgs(ks, r["signer"], r["msgs"], r["sigs"])
        assert st.tolist() == r["want"].tolist()
    finally:
        c.close()


def test_skew(ctx):
    """One signer owns 65 * 64 + 1 items -- 66 tiles, more than one pass of the signers' tree at a
    fan-in of 64 -- with one bad item at the end; two other signers own one item each."""
    rng = random.Random(77)
    sks, pks = _keys(ctx, rng, 3)
    n_big = 65 * 64 + 1
    msgs = [b"vote %d" % i + bytes(rng.randrange(256) for _ in range(8)) for i in range(n_big)]
    sigs = ctx.sign_shares(sks[1], msgs, want_H=False)[0]
    sigs[-1] = sigs[0]  # another message's signature
    signer = [1] * n_big
    for j in (0, 2):
        m = b"the only message of signer %d" % j
        pos = rng.randrange(len(msgs))
        msgs.insert(pos, m)
        sigs.insert(pos, ctx.sign_shares(sks[j], [m], want_H=False)[0][0])
        signer.insert(pos, j)
    ks, _ = ctx.keyset_load(pks)
    try:
        st = ctx.verify_signed_msgs(ks, signer, msgs, sigs)
    finally:
        ctx.keyset_free(ks)
    want = [N.ACCEPT] * len(msgs)
    want[-1] = N.REJECT
    assert st.tolist() == want


def test_skew_all_valid(ctx):
    """The same shape without the bad item: the tree's sums alone decide 4.2 k items."""
    rng = random.Random(78)
    sks, pks = _keys(ctx, rng, 2)
    n_big = 65 * 64 + 1
    msgs = [b"ack %d" % i for i in range(n_big)] + [b"one more"]
    sigs = ctx.sign_shares(sks[0], msgs[:n_big], want_H=False)[0] + ctx.sign_shares(sks[1], msgs[n_big:], want_H=False)[0]
    ks, _ = ctx.keyset_load(pks)
    try:
        st = ctx.verify_signed_msgs(ks, [0] * n_big + [1], msgs, sigs)
    finally:
        ctx.keyset_free(ks)
    assert not st.any()


def test_cancellation():
    """One signer submits sigma_1 + D and sigma_2 - D with D in the subgroup: the unweighted sums
    verify, so only the per-item scalars catch it.  Both items are REJECT, on three fresh contexts
    (fresh ChaCha keys)."""
    rng = random.Random(31)
    for _ in range(3):
        c = _ctx()
        try:
            sks, pks = _keys(c, rng, 2)
            msgs = [b"first", b"second", b"third", b"fourth"]
            sg, H = c.sign_shares(sks[0], msgs[:3])
            other = c.sign_shares(sks[1], msgs[3:], want_H=False)[0]
            D = c.sign_shares(rng.randrange(1, R), [b"delta"], want_H=False)[0][0]
            (s1, s2), st = c.g2_msm(2, 2, [sg[0], D, sg[1], D], [1, 1, 1, R - 1])
            assert not st.any() and s1 != sg[0] and s2 != sg[1]
            (hsum, ssum), st = c.g2_msm(2, 2, [H[0], H[1], s1, s2], [1, 1, 1, 1])
            assert not st.any()
            assert c.verify_sigs([pks[0]], [hsum], [ssum]).tolist() == [N.ACCEPT]  # the plain sums agree
            ks, _ = c.keyset_load(pks)
            got = c.verify_signed_msgs(ks, [0, 0, 0, 1], msgs, [s1, s2, sg[2]] + other)
            assert got.tolist() == [N.REJECT, N.REJECT, N.ACCEPT, N.ACCEPT]
        finally:
            c.close()


def test_independent_oracle(ctx):
    """Four items signed by oracle.threshold_crypto.sign and judged by its verify: two valid, two
    not.  Nothing of the library made or judged them."""
    rng = random.Random(41)
    sks = [rng.randrange(1, R) for _ in range(2)]
    pts = [B.g1_mul(B.G1_GEN, sk) for sk in sks]
    msgs = [b"oracle vote", b"", bytes(range(137)), b"oracle part"]
    signer = [0, 1, 0, 1]
    sig_pts = [TC.sign(sks[0], msgs[0]), TC.sign(sks[1], msgs[1]),
               TC.sign(sks[1], msgs[2]),           # the other signer's key
               TC.sign(sks[1], b"another part")]   # another message
    want = [N.ACCEPT if TC.verify(pts[j], s, m) else N.REJECT for j, s, m in zip(signer, sig_pts, msgs)]
    assert want == [N.ACCEPT, N.ACCEPT, N.REJECT, N.REJECT]
    ks, bad = ctx.keyset_load([B.g1_compress(p) for p in pts])
    assert bad == 0
    try:
        st = ctx.verify_signed_msgs(ks, signer, msgs, [B.g2_compress(s) for s in sig_pts])
    finally:
        ctx.keyset_free(ks)
    assert st.tolist() == want


def test_empty_call_and_bad_key(ctx):
    lib, null = ctx.lib, N._ptr(None)
    assert lib.hbtc_verify_signed_msgs(ctx.h, 0, 0, null, null, null, null, null) == 0
    assert ctx.verify_signed_msgs(0, [], [], []).size == 0
    rng = random.Random(51)
    sks, pks = _keys(ctx, rng, 3)
    bad_pk = bytes.fromhex(CODEC["g1_bad"][0]["enc"])
    ks, bad = ctx.keyset_load([pks[0], bad_pk, pks[2]])
    assert bad == 1
    msgs = [b"m%d" % i for i in range(9)]
    signer = [i % 3 for i in range(9)]
    sigs = [ctx.sign_shares(sks[j], [m], want_H=False)[0][0] for j, m in zip(signer, msgs)]
    try:
        st = ctx.verify_signed_msgs(ks, signer, msgs, sigs)
    finally:
        ctx.keyset_free(ks)
    assert st.tolist() == [N.DECODE_ERR if j == 1 else N.ACCEPT for j in signer]


def test_argument_checks(ctx, ragged):
    lib, null = ctx.lib, N._ptr(None)
    ks = ragged["ks"]
    who = np.zeros(1, np.uint32)
    sig = np.frombuffer(ragged["sigs"][0], np.uint8).copy()
    st = np.zeros(1, np.int32)
    msg = np.zeros(4, np.uint8)
    off0, off1 = np.zeros(2, np.uint32), np.array([0, 4], np.uint32)
    f = lib.hbtc_verify_signed_msgs
    assert f(ctx.h, ks, 1, null, N._ptr(msg), N._ptr(off1), N._ptr(sig), N._ptr(st)) == -1
    assert f(ctx.h, ks, 1, N._ptr(who), N._ptr(msg), null, N._ptr(sig), N._ptr(st)) == -1
    assert f(ctx.h, ks, 1, N._ptr(who), N._ptr(msg), N._ptr(off1), null, N._ptr(st)) == -1
    assert f(ctx.h, ks, 1, N._ptr(who), N._ptr(msg), N._ptr(off1), N._ptr(sig), null) == -1
    assert f(ctx.h, ks, 1, N._ptr(who), null, N._ptr(off1), N._ptr(sig), N._ptr(st)) == -1  # bytes, no buffer
    for bad in (np.array([1, 4], np.uint32), np.array([4, 0], np.uint32)):
        assert f(ctx.h, ks, 1, N._ptr(who), N._ptr(msg), N._ptr(bad), N._ptr(sig), N._ptr(st)) == -1
    assert f(ctx.h, 0xFFFF, 1, N._ptr(who), N._ptr(msg), N._ptr(off1), N._ptr(sig), N._ptr(st)) == -3
    # the empty message without a buffer is a call like any other
    assert f(ctx.h, ks, 1, N._ptr(who), null, N._ptr(off0), N._ptr(sig), N._ptr(st)) == 0
    assert st[0] in (N.ACCEPT, N.REJECT)
