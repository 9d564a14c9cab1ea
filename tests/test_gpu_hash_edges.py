"""The GPU hash-to-G2 path (hbtc_hash.hip: k_hash_cand, k_g2_clear_cofactor) on the cases of
tests/hash_cases.py: every draw class of G2::rand's loop, the SHA3 rate edges of the message and of
hash_g1_g2's inner digest, and batch sizes on both sides of the 32-candidate (k_g2_clear_cofactor)
and 64-message (k_hash_cand) workgroup edges with the heaviest draw beside first-draw lanes.
Every expected byte comes from the oracle (oracle/threshold_crypto.py), computed once per module;
the host C path is not consulted (tests/test_hash_cases.py pins it on the same cases).  The
consumers that launch the kernels themselves (hbtc_sign_shares, hbtc_verify_signed_msgs,
hbtc_decrypt_shares / hbtc_decrypt, hbtc_encrypt) run one small batch each against oracle-made
signatures and ciphertexts.  Bar: identical bytes and decisions.

Not reached here: the [h2] P = O redraw (st[i] = 1 in k_g2_clear_cofactor) -- no message is known
to hash to a candidate in the cofactor's kernel; g2p_clear_cofactor's own cases in
tests/devarith_cases.py cover that result.  Parity with real threshold_crypto bytes stays
unpinned."""
import numpy as np
import pytest

import hash_cases as HC
from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # HBTC_ERR_ARG (include/hbtc.h)
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g2():
    """(cases [(name, msg)], oracle hashes, layouts)"""
    cases = HC.g2_cases()
    profs = [HC.trace(m, with_hash=False)[1] for _, m in cases]
    empty = [m for _, m in cases].index(b"")
    return cases, [HC.want_g2(m) for _, m in cases], HC.layouts(profs, empty)


@pytest.fixture(scope="module")
def g1g2():
    """(cases [(name, u, v)], oracle hashes, layouts)"""
    cases = HC.g1g2_cases()
    profs = [HC.trace(HC.g1g2_seed_msg(u, v), with_hash=False)[1] for _, u, v in cases]
    empty = [v for _, _, v in cases].index(b"")
    return cases, [HC.want_g1g2(u, v) for _, u, v in cases], HC.layouts(profs, empty)


def _wrong(idx, got, want, cases):
    return [(i, cases[c][0]) for i, c in enumerate(idx) if got[i] != want[c]]


# ------------------------------------------------------------------ the batches
def test_hash_g2_batches_equal_the_oracle(ctx, g2):
    cases, want, lay = g2
    seen = [set() for _ in cases]
    for name, idx in lay.items():
        got = ctx.hash_g2_batch([cases[c][1] for c in idx])
        assert _wrong(idx, got, want, cases) == [], name
        for i, c in enumerate(idx):
            seen[c].add(got[i])
    assert all(len(s) == 1 for s in seen)  # every case ran, with one answer wherever it sat


def test_hash_g1_g2_batches_equal_the_oracle(ctx, g1g2):
    cases, want, lay = g1g2
    seen = [set() for _ in cases]
    for name, idx in lay.items():
        got = ctx.hash_g1_g2_batch([cases[c][1] for c in idx], [cases[c][2] for c in idx])
        assert _wrong(idx, got, want, cases) == [], name
        for i, c in enumerate(idx):
            seen[c].add(got[i])
    assert all(len(s) == 1 for s in seen)


# ------------------------------------------------------------------ the C ABI's buffer rules
def _u_batch(n):
    return [B.g1_compress(B.g1_mul(B.G1_GEN, 1 + i % HC.U_MULTIPLES)) for i in range(n)]


@pytest.mark.parametrize("n", [1, 33])
def test_null_msgs_is_a_batch_of_empty_messages(ctx, n):
    off = np.zeros(n + 1, np.uint32)
    out = np.full(96 * n, GUARD, np.uint8)
    assert ctx.lib.hbtc_hash_g2_batch_gpu(ctx.h, n, None, N._ptr(off), N._ptr(out)) == 0
    assert out.tobytes() == HC.want_g2(b"") * n
    us = _u_batch(n)
    u = N._join(us, 48)
    out[:] = GUARD
    assert ctx.lib.hbtc_hash_g1_g2_batch_gpu(ctx.h, n, N._ptr(u), None, N._ptr(off), N._ptr(out)) == 0
    assert out.tobytes() == b"".join(HC.want_g1g2(x, b"") for x in us)


def test_n_zero_touches_nothing(ctx):
    off = np.zeros(1, np.uint32)
    out = np.full(96, GUARD, np.uint8)
    u = N._join(_u_batch(1), 48)
    assert ctx.lib.hbtc_hash_g2_batch_gpu(ctx.h, 0, None, N._ptr(off), N._ptr(out)) == 0
    assert ctx.lib.hbtc_hash_g1_g2_batch_gpu(ctx.h, 0, N._ptr(u), None, N._ptr(off), N._ptr(out)) == 0
    assert ctx.lib.hbtc_hash_g2_batch_gpu(ctx.h, 0, None, None, None) == 0
    assert ctx.lib.hbtc_hash_g1_g2_batch_gpu(ctx.h, 0, None, None, None, None) == 0
    assert (out == GUARD).all()


@pytest.mark.parametrize("offsets", [[1, 1, 2, 3], [0, 2, 1, 3], [0, 3, 3, 2]])
def test_bad_offsets_are_argument_errors(ctx, offsets):
    off = np.array(offsets, np.uint32)
    msgs = np.zeros(8, np.uint8)
    out = np.full(96 * 3, GUARD, np.uint8)
    u = N._join(_u_batch(3), 48)
    assert ctx.lib.hbtc_hash_g2_batch_gpu(ctx.h, 3, N._ptr(msgs), N._ptr(off), N._ptr(out)) == ERR_ARG
    assert ctx.lib.hbtc_hash_g1_g2_batch_gpu(ctx.h, 3, N._ptr(u), N._ptr(msgs), N._ptr(off),
                                             N._ptr(out)) == ERR_ARG
    assert (out == GUARD).all()
    # a NULL buffer with bytes to read is one too
    good = np.array([0, 1, 2, 3], np.uint32)
    assert ctx.lib.hbtc_hash_g2_batch_gpu(ctx.h, 3, None, N._ptr(good), N._ptr(out)) == ERR_ARG


# ------------------------------------------------------------------ the consumers
SKS = [0x1D2C3B4A5968778695A4B3C2D1E0F00112233445566778899AABBCCDDEEFF013 % B.R, 5, B.R - 2]


@pytest.fixture(scope="module")
def signed_set(g2):
    """The mined messages and the rate-edge ones, signed by the oracle under three keys."""
    cases, _, _ = g2
    keep = [(name, m) for name, m in cases if name.startswith("hc") or len(m) in (0, 135, 136, 137, 272)]
    signer = [i % len(SKS) for i in range(len(keep))]
    sigs = [B.g2_compress(TC.sign(SKS[j], m)) for j, (_, m) in zip(signer, keep)]
    return keep, signer, sigs


def test_sign_shares_hash_and_signature_equal_the_oracle(ctx, g2):
    cases, want, _ = g2
    msgs = [m for _, m in cases]
    assert len(msgs) <= 40
    sk = SKS[0]
    sigs, H = ctx.sign_shares(sk, msgs)
    assert [cases[i][0] for i in range(len(msgs)) if H[i] != want[i]] == []
    for i, (name, m) in enumerate(cases):
        assert sigs[i] == B.g2_compress(B.g2_mul(HC.g2_point(m), sk)), name


@pytest.mark.parametrize("exact_below", [0, None])
def test_signed_message_verify_accepts_oracle_signatures(signed_set, exact_below):
    """exact_below 0: the grouped route; None: the library's default choice at this size."""
    keep, signer, sigs = signed_set
    assert len(keep) <= 40
    c = N.Context(0)
    try:
        if exact_below is not None:
            c.set_exact_below(exact_below)
        ks, bad = c.keyset_load([B.g1_compress(B.g1_mul(B.G1_GEN, sk)) for sk in SKS])
        assert bad == 0
        msgs = [m for _, m in keep]
        st = c.verify_signed_msgs(ks, signer, msgs, sigs)
        assert [keep[i][0] for i in range(len(keep)) if st[i] != N.ACCEPT] == []
        # one byte of every message changed: another hash, the signature no longer fits
        flip = [i for i, m in enumerate(msgs) if m]
        bent = [msgs[i][:len(msgs[i]) // 2] + bytes([msgs[i][len(msgs[i]) // 2] ^ 0x01]) +
                msgs[i][len(msgs[i]) // 2 + 1:] for i in flip]
        st = c.verify_signed_msgs(ks, [signer[i] for i in flip], bent, [sigs[i] for i in flip])
        assert [keep[i][0] for k, i in enumerate(flip) if st[k] != N.REJECT] == []
    finally:
        c.close()


CT_LENGTHS = [0, 64, 65, 136, 137]


@pytest.fixture(scope="module")
def ciphertexts():
    """Oracle ciphertexts under sk's public key at the |v| where hash_g1_g2 changes its input."""
    sk = SKS[0]
    pk = B.g1_mul(B.G1_GEN, sk)
    rng = np.random.default_rng(0x6374)
    out = []
    for k, n in enumerate(CT_LENGTHS):
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        r = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % B.R
        u, v, w = TC.encrypt_with_rng(pk, r, msg)
        out.append({"msg": msg, "r": r, "u": B.g1_compress(u), "v": v, "w": B.g2_compress(w),
                    "H": B.g2_compress(TC.hash_g1_g2(u, v)), "share": B.g1_compress(B.g1_mul(u, sk))})
    return sk, B.g1_compress(pk), out


def _flip_v(ct):
    v = ct["v"]
    return v[:-1] + bytes([v[-1] ^ 0x80])


def test_decrypt_shares_accepts_oracle_ciphertexts(ctx, ciphertexts):
    sk, _, cts = ciphertexts
    us, vs, ws = [c["u"] for c in cts], [c["v"] for c in cts], [c["w"] for c in cts]
    shares, H, st = ctx.decrypt_shares(sk, us, vs, ws)
    assert list(st) == [N.ACCEPT] * len(cts)
    assert H == [c["H"] for c in cts] and shares == [c["share"] for c in cts]
    bent = [c for c in cts if c["v"]]
    assert len(bent) == len(cts) - 1  # the empty v has no byte to flip
    shares, H, st = ctx.decrypt_shares(sk, [c["u"] for c in bent], [_flip_v(c) for c in bent],
                                       [c["w"] for c in bent])
    assert list(st) == [N.REJECT] * len(bent) and shares == [None] * len(bent)
    for c, h in zip(bent, H):
        assert h == HC.want_g1g2(c["u"], _flip_v(c)) and h != c["H"]


def test_decrypt_accepts_oracle_ciphertexts(ctx, ciphertexts):
    sk, _, cts = ciphertexts
    plain, st = ctx.decrypt(sk, [c["u"] for c in cts], [c["w"] for c in cts], [c["v"] for c in cts])
    assert list(st) == [N.ACCEPT] * len(cts) and plain == [c["msg"] for c in cts]
    bent = [c for c in cts if c["v"]]
    plain, st = ctx.decrypt(sk, [c["u"] for c in bent], [c["w"] for c in bent], [_flip_v(c) for c in bent])
    assert list(st) == [N.REJECT] * len(bent) and plain == [None] * len(bent)


def test_encrypt_with_fixed_r_equals_the_oracle(ctx, ciphertexts):
    _, pk, cts = ciphertexts
    got, st = ctx.encrypt(pk, [c["r"] for c in cts], [c["msg"] for c in cts])
    assert list(st) == [N.ACCEPT] * len(cts)
    for c, (u, v, w) in zip(cts, got):
        assert (u, v, w) == (c["u"], c["v"], c["w"]), len(c["msg"])
