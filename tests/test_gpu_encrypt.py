"""hbtc_encrypt (PublicKey::encrypt_with_rng, batched and device-resident) and hbtc_fr_poly_eval
on the GPU, through hbbft_amd._native and ctypes.

Oracles: oracle/threshold_crypto.encrypt_with_rng (the pure-Python restatement, ~50 items per
test), the five primitive calls the fused path replaces (g1_mul, g1_mul, xor_hash_bytes_batch,
hash_g1_g2_batch_gpu, g2_mul), hbtc_decrypt / hbtc_verify_ciphertexts for the round trip, and
Python integers for the polynomials."""
import json
import os
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from hbbft_amd import skg, wire
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
G1_INF = bytes([0xC0]) + bytes(47)
G2_INF = bytes([0xC0]) + bytes(95)
EDGE_SCALARS = [1, 2, 255, 256, 1 << 64, R - 1, R, R + 1, (1 << 256) - 1]
LENGTHS = [0, 1, 15, 16, 17, 40, 64, 65, 136, 137, 1000]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec.json")


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def _point(pk_bytes):
    return None if pk_bytes == G1_INF else B.g1_decompress(pk_bytes)


def _restated(pk_bytes, r, msg):
    u, v, w = TC.encrypt_with_rng(_point(pk_bytes), r % R, msg)
    return (B.g1_compress(u), v, B.g2_compress(w) if w is not None else G2_INF)


def _keys(rng, n):
    return [B.g1_compress(B.g1_mul(B.G1_GEN, rng.randrange(1, R))) for _ in range(n)]


@pytest.fixture(scope="module")
def cases():
    """(shared-key batch, per-item-key batch), each (pks, rs, msgs, restated): every edge scalar,
    every length, random scalars; keys: random, the generator, the infinity encoding."""
    rng = random.Random(20250)
    msg = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    rs = EDGE_SCALARS + [rng.randrange(1, R) for _ in LENGTHS]
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(len(EDGE_SCALARS))] + LENGTHS
    shared_pk = _keys(rng, 1)[0]
    shared = (shared_pk, rs, [msg(n) for n in lens])
    pool = _keys(rng, 3) + [G1, G1_INF]
    rs2 = EDGE_SCALARS + [rng.randrange(1, R) for _ in LENGTHS] + [rng.randrange(1, R) for _ in range(4)]
    lens2 = LENGTHS[3:] + LENGTHS[:3] + [40] * (len(rs2) - len(LENGTHS))
    pks2 = [pool[i % len(pool)] for i in range(len(rs2))]
    per_item = (pks2, rs2, [msg(n) for n in lens2])
    out = []
    for pks, scal, msgs in (shared, per_item):
        ref = [_restated(pks if isinstance(pks, bytes) else pks[i], scal[i], msgs[i])
               for i in range(len(scal))]
        out.append((pks, scal, msgs, ref))
    return out


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("which", [0, 1], ids=["shared_key", "per_item_keys"])
def test_parity_with_restatement(ctx, cases, which):
    pks, rs, msgs, ref = cases[which]
    got, st = ctx.encrypt(pks, rs, msgs)
    assert not st.any()
    for i, (g, want) in enumerate(zip(got, ref)):
        assert g == want, (i, hex(rs[i]), len(msgs[i]))
    zero = [i for i, r in enumerate(rs) if r % R == 0]
    assert zero and all(got[i][0] == G1_INF and got[i][2] == G2_INF for i in zero)


# ------------------------------------------------------------------ 2. the composed path
def _composed(ctx, pks, rs, msgs):
    """The five primitive calls of the former skg.encrypt_batch."""
    n = len(msgs)
    sc = np.frombuffer(b"".join(int(r).to_bytes(32, "little") for r in rs), np.uint8).copy()
    u, st1 = ctx.g1_mul(G1, sc)
    g, st2 = ctx.g1_mul(pks, sc)
    assert not st1.any() and not st2.any()
    us = [bytes(u[48 * i:48 * i + 48]) for i in range(n)]
    gs = [bytes(g[48 * i:48 * i + 48]) for i in range(n)]
    vs = N.xor_hash_bytes_batch(gs, msgs)
    H = ctx.hash_g1_g2_batch(us, vs)
    w, st3 = ctx.g2_mul(H, sc)
    assert not st3.any()
    return [(us[i], vs[i], bytes(w[96 * i:96 * i + 96])) for i in range(n)]


@pytest.fixture(scope="module")
def key_pool(ctx):
    rng = random.Random(77)
    out, st = ctx.g1_mul(G1, [rng.randrange(1, R) for _ in range(130)])
    assert not st.any()
    return [bytes(out[48 * i:48 * i + 48]) for i in range(130)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_parity_with_composed_path(ctx, key_pool, n):
    rng = random.Random(1000 + n)
    rs = [rng.randrange(1, R) for _ in range(n)]
    msgs = [bytes(rng.randrange(256) for _ in range(LENGTHS[i % len(LENGTHS)] if i % 3 else 40))
            for i in range(n)]
    pks = key_pool[:n]
    got, st = ctx.encrypt(pks, rs, msgs)
    assert not st.any()
    assert got == _composed(ctx, pks, rs, msgs)
    shared, st = ctx.encrypt(pks[0], rs, msgs)
    assert not st.any()
    assert shared == _composed(ctx, [pks[0]] * n, rs, msgs)


# ------------------------------------------------------------------ 3. round trip
def test_round_trip_decrypt_and_verify(ctx):
    rng = random.Random(31)
    n = 70
    sk = rng.randrange(1, R)
    pk, st = ctx.g1_mul(G1, [sk])
    assert not st.any()
    rs = [rng.randrange(1, R) for _ in range(n)]
    msgs = [bytes(rng.randrange(256) for _ in range(LENGTHS[i % len(LENGTHS)])) for i in range(n)]
    cts, st = ctx.encrypt(bytes(pk), rs, msgs)
    assert not st.any()
    us, vs, ws = [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]
    plain, dst = ctx.decrypt(sk, us, ws, vs)
    assert (dst == N.ACCEPT).all()
    assert plain == msgs
    vst = ctx.verify_ciphertexts(us, ctx.hash_g1_g2_batch(us, vs), ws)
    assert (np.asarray(vst) == N.ACCEPT).all()


# ------------------------------------------------------------------ 4. bad keys
def test_bad_keys_are_rejected_like_g1_mul(ctx, key_pool):
    bad = [bytes.fromhex(e["enc"]) for e in json.load(open(GOLDEN))["g1_bad"]]
    assert bad
    rng = random.Random(41)
    pks, is_bad = [], []
    for i, b in enumerate(bad):
        pks += [key_pool[2 * i], b, key_pool[2 * i + 1]]
        is_bad += [False, True, False]
    n = len(pks)
    rs = [rng.randrange(1, R) for _ in range(n)]
    msgs = [bytes(rng.randrange(256) for _ in range(LENGTHS[(i + 4) % len(LENGTHS)])) for i in range(n)]
    got, st = ctx.encrypt(pks, rs, msgs)
    _, mst = ctx.g1_mul(pks, rs)
    assert list(st) == list(mst)
    assert [s == N.DECODE_ERR for s in st] == is_bad
    good = [i for i in range(n) if not is_bad[i]]
    ref, rst = ctx.encrypt([pks[i] for i in good], [rs[i] for i in good], [msgs[i] for i in good])
    assert not rst.any()
    assert [got[i] for i in good] == ref
    for i in range(n):
        if is_bad[i]:
            assert got[i] == (bytes(48), bytes(len(msgs[i])), bytes(96)), i
    # a bad shared key rejects every item
    _, sst = ctx.encrypt(bad[0], rs[:3], msgs[:3])
    assert (sst == N.DECODE_ERR).all()


# ------------------------------------------------------------------ 5. the lazily built table
def test_calling_twice_is_bit_equal(cases):
    pks, rs, msgs, ref = cases[1]
    c = N.Context(0)  # a fresh context: the first call builds the generator's table
    try:
        first, st1 = c.encrypt(pks, rs, msgs)
        second, st2 = c.encrypt(pks, rs, msgs)
    finally:
        c.close()
    assert not st1.any() and not st2.any()
    assert first == second == ref


def test_argument_checks(ctx):
    lib, null = ctx.lib, N._ptr(None)
    pk = np.frombuffer(G1, np.uint8).copy()
    r = np.zeros(32, np.uint8)
    u, w, st = np.zeros(48, np.uint8), np.zeros(96, np.uint8), np.zeros(1, np.int32)
    bad_off = np.array([1, 1], np.uint32)
    assert lib.hbtc_encrypt(ctx.h, 0, null, 0, null, null, null, null, null, null, null) == 0
    assert lib.hbtc_encrypt(ctx.h, 1, N._ptr(pk), 0, N._ptr(r), null, N._ptr(bad_off), N._ptr(u), null,
                            N._ptr(w), N._ptr(st)) == -1
    assert lib.hbtc_encrypt(ctx.h, 1, N._ptr(pk), 2, N._ptr(r), null, N._ptr(np.zeros(2, np.uint32)),
                            N._ptr(u), null, N._ptr(w), N._ptr(st)) == -1


# ------------------------------------------------------------------ 6. Fr polynomials
def _draw(rng):
    pool = [0, 1, R - 1, R, (1 << 256) - 1]
    return rng.choice(pool) if rng.random() < 0.4 else rng.randrange(1 << 256)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 0, 3), (3, 5, 65), (67, 4, 67), (1, 334, 70)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_fr_poly_eval_against_python_integers(ctx, shape):
    n_poly, n_coeff, n_x = shape
    rng = random.Random(sum(shape))
    coeffs = [[_draw(rng) for _ in range(n_coeff)] for _ in range(n_poly)]
    xs = [_draw(rng) for _ in range(n_x)]
    out = ctx.fr_poly_eval(coeffs, xs)
    assert out.shape == (n_poly, n_x, 32)
    for p in range(n_poly):
        for j in range(n_x):
            want = sum(c * pow(xs[j], k, R) for k, c in enumerate(coeffs[p])) % R
            assert int.from_bytes(out[p, j].tobytes(), "little") == want, (p, j)


# ------------------------------------------------------------------ 7. the skg layer
def test_skg_encrypt_batch_equals_restatement(ctx, cases):
    pks, rs, msgs, ref = cases[1]
    keep = [i for i in range(len(rs)) if pks[i] != G1_INF][:12]
    cts = skg.encrypt_batch(ctx, [pks[i] for i in keep], [msgs[i] for i in keep], [rs[i] for i in keep])
    assert [tuple(c) for c in cts] == [ref[i] for i in keep]
    assert all(isinstance(c, skg.Ciphertext) for c in cts)


def test_sync_key_gen_parts_and_acks_decrypt_to_the_polynomials(ctx, monkeypatch):
    """N = 4, t = 1: every row of every Part decrypts to _bivar_row of the proposer's polynomial,
    every Ack value to _poly_eval of the acked row."""
    n, t = 4, 1
    rng = random.Random(404)
    sks = [rng.randrange(1, R) for _ in range(n)]
    out, st = ctx.g1_mul(G1, sks)
    assert not st.any()
    pub = {i: bytes(out[48 * i:48 * i + 48]) for i in range(n)}
    polys = {}
    real_randbelow = skg.secrets.randbelow

    nodes, parts = [], []
    for i in range(n):
        drawn = []

        def rb(bound, drawn=drawn):
            v = real_randbelow(bound)
            drawn.append((bound, v))
            return v
        monkeypatch.setattr(skg.secrets, "randbelow", rb)
        kg, part = skg.SyncKeyGen.new(ctx, i, sks[i], pub, t)
        monkeypatch.setattr(skg.secrets, "randbelow", real_randbelow)
        polys[i] = [v for bound, v in drawn if bound == R][:(t + 1) * (t + 2) // 2]
        nodes.append(kg)
        parts.append(part)
    for p, part in enumerate(parts):
        assert len(part.rows) == n
        for j in range(n):
            row = skg.decrypt_batch(ctx, sks[j], [part.rows[j]])[0]
            assert row is not None
            assert wire.poly_from_wire(row) == skg._bivar_row(polys[p], t, j + 1), (p, j)
    # node 0 handles every Part and acks it
    for p, part in enumerate(parts):
        nodes[0].handle_part(p, part)
    res = nodes[0].flush()
    assert [r[0] for r in res] == ["valid"] * n
    for p, (_, ack) in enumerate(res):
        assert ack.proposer == p and len(ack.values) == n
        our_row = skg._bivar_row(polys[p], t, 1)
        for j in range(n):
            val = skg.decrypt_batch(ctx, sks[j], [ack.values[j]])[0]
            assert val is not None
            assert wire.fr_value_from_wire(val) == skg._poly_eval(our_row, j + 1), (p, j)
