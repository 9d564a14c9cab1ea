"""hbtc_skg_part and hbtc_skg_acks (SyncKeyGen::new's Part and the Acks of verified Parts, one
device call each) on gfx950.

References: oracle/threshold_crypto.py (commitment, bivar_poly_row, encrypt_with_rng: the
pure-Python restatement, at most ~25 encryptions per case), hbbft_amd/wire.py's frames, and at the
larger shapes the composed calls the one-call path replaces (g1_mul, fr_poly_eval, wire.*,
hbtc_encrypt).  Bar: every commitment point, u, v, w and status bit-equal."""
import random

import numpy as np
import pytest

import keyset_cases as KC
from hbbft_amd import _native as N
from hbbft_amd import skg, wire
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
G1_INF = bytes([0xC0]) + bytes(47)
G2_INF = bytes([0xC0]) + bytes(95)
EDGE = [0, 1, R - 1, R, R + 1, (1 << 256) - 1]


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(ctx):
    """65 secret keys and their public keys (hbtc_g1_mul, pinned by tests/test_gpu_parity.py)."""
    rng = random.Random(6667)
    sks = [rng.randrange(1, R) for _ in range(65)]
    out, st = ctx.g1_mul(G1, sks)
    assert not st.any()
    return sks, [bytes(out[48 * i:48 * i + 48]) for i in range(65)]


class _Loaded:
    """A key set loaded for the length of a with block."""

    def __init__(self, ctx, keys, n_bad=0):
        self.ctx, self.keys, self.n_bad = ctx, keys, n_bad

    def __enter__(self):
        self.kid, bad = self.ctx.keyset_load(self.keys)
        assert bad == self.n_bad
        return self.kid

    def __exit__(self, *exc):
        self.ctx.keyset_free(self.kid)


def _draw(rng, n):
    return [rng.randrange(1, R) for _ in range(n)]


def _composed_part(ctx, keys, t, b, rs):
    """The Part by the calls SyncKeyGen.new composes: (commit, [(u, v, w)], status)."""
    cm, st = ctx.g1_mul(G1, skg._fr_le(b))
    assert not st.any()
    rows = skg.bivar_rows(ctx, b, t, len(keys))
    cts, est = ctx.encrypt(keys, rs, rows)
    return [bytes(cm[48 * k:48 * k + 48]) for k in range(len(b))], cts, est


def _composed_acks(ctx, keys, rows, rs):
    """The Acks by the calls _emit_acks composes: ([(u, v, w)], status)."""
    n = len(keys)
    msgs = [m for vals in skg.ack_values(ctx, rows, n) for m in vals]
    return ctx.encrypt(list(keys) * len(rows), rs, msgs)


def _restated(pk_bytes, r, msg):
    pk = None if pk_bytes == G1_INF else B.g1_decompress(pk_bytes)
    u, v, w = TC.encrypt_with_rng(pk, r % R, msg)
    return (B.g1_compress(u), v, B.g2_compress(w) if w is not None else G2_INF)


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("n,t", [(1, 0), (4, 1), (7, 2)])
def test_part_parity_with_restatement(ctx, pool, n, t):
    rng = random.Random(100 * n + t)
    keys = pool[1][:n]
    b, rs = _draw(rng, (t + 1) * (t + 2) // 2), _draw(rng, n)
    with _Loaded(ctx, keys) as kid:
        commit, cts, st = ctx.skg_part(kid, n, t, b, rs)
    assert not st.any()
    assert commit == [B.g1_compress(p) for p in TC.commitment(b)]
    for x in range(1, n + 1):
        row = wire.poly_to_wire(TC.bivar_poly_row(b, t, x))
        assert len(row) == 8 + 40 * (t + 1)
        assert cts[x - 1] == _restated(keys[x - 1], rs[x - 1], row), x


@pytest.mark.parametrize("n_rows,n,n_coeff", [(1, 4, 2), (3, 7, 3)])
def test_acks_parity_with_restatement(ctx, pool, n_rows, n, n_coeff):
    rng = random.Random(1000 * n_rows + n)
    keys = pool[1][:n]
    rows = [_draw(rng, n_coeff) for _ in range(n_rows)]
    rs = _draw(rng, n_rows * n)
    with _Loaded(ctx, keys) as kid:
        cts, st = ctx.skg_acks(kid, n, rows, rs)
    assert not st.any() and len(cts) == n_rows * n
    for a in range(n_rows):
        for i in range(n):
            val = wire.fr_to_wire(TC.poly_evaluate(rows[a], i + 1))
            assert cts[a * n + i] == _restated(keys[i], rs[a * n + i], val), (a, i)


# ------------------------------------------------------------------ 2. the composed path
# (33, 10): 66 coefficients straddle a wave of k_skgp_commit's pairs and of its items, 33 items the
# 32-item wave of k_enc_w, a 448-byte row the 64-byte inner hash switch and the SHA3 rate;
# (65, 2): 65 items straddle a wave of the G1 stage; (5, 3) and (4, 1): 10 and 3 coefficients
@pytest.mark.parametrize("n,t", [(33, 10), (65, 2), (5, 3), (4, 1)])
def test_part_parity_with_composed_path(ctx, pool, n, t):
    rng = random.Random(7 * n + t)
    keys = pool[1][:n]
    b, rs = _draw(rng, (t + 1) * (t + 2) // 2), _draw(rng, n)
    with _Loaded(ctx, keys) as kid:
        commit, cts, st = ctx.skg_part(kid, n, t, b, rs)
    want_commit, want_cts, want_st = _composed_part(ctx, keys, t, b, rs)
    assert not st.any() and not want_st.any()
    assert commit == want_commit
    assert cts == want_cts


def test_packed_coefficients_give_the_same_part_and_stay_intact(ctx, pool):
    """bcoef as a packed uint8 array: the wrapper clears its own copy, never the caller's array."""
    rng = random.Random(4100)
    keys = pool[1][:4]
    b, rs = _draw(rng, 3), _draw(rng, 4)
    packed = skg._fr_le(b)
    keep = packed.copy()
    with _Loaded(ctx, keys) as kid:
        from_ints = ctx.skg_part(kid, 4, 1, b, rs)
        from_array = ctx.skg_part(kid, 4, 1, packed, rs)
        with pytest.raises(ValueError):
            ctx.skg_part(kid, 4, 1, packed[:64], rs)
    assert (packed == keep).all()
    assert from_array[0] == from_ints[0] and from_array[1] == from_ints[1]


# 66 and 130 items; constant rows; rows without coefficients (every value is 0)
@pytest.mark.parametrize("n_rows,n,n_coeff", [(3, 22, 4), (2, 65, 3), (2, 5, 1), (2, 5, 0)])
def test_acks_parity_with_composed_path(ctx, pool, n_rows, n, n_coeff):
    rng = random.Random(31 * n_rows + n)
    keys = pool[1][:n]
    rows = [_draw(rng, n_coeff) for _ in range(n_rows)]
    rs = _draw(rng, n_rows * n)
    with _Loaded(ctx, keys) as kid:
        cts, st = ctx.skg_acks(kid, n, rows, rs)
    want, want_st = _composed_acks(ctx, keys, rows, rs)
    assert not st.any() and not want_st.any()
    assert cts == want
    if n_coeff == 0:
        sks = pool[0]
        plain, dst = ctx.decrypt(sks[0], [cts[0][0]], [cts[0][2]], [cts[0][1]])
        assert dst[0] == N.ACCEPT and plain[0] == wire.fr_to_wire(0)


# ------------------------------------------------------------------ 3. edge scalars
def test_edge_scalars_in_every_place(ctx, pool):
    keys = pool[1][:6]
    with _Loaded(ctx, keys) as kid:
        commit, cts, st = ctx.skg_part(kid, 6, 2, EDGE, EDGE)            # t = 2: six coefficients
        acts, ast = ctx.skg_acks(kid, 6, [EDGE, EDGE[::-1]], EDGE + EDGE[::-1])
    want_commit, want_cts, want_st = _composed_part(ctx, keys, 2, EDGE, EDGE)
    assert not st.any() and not want_st.any()
    assert commit == want_commit and cts == want_cts
    assert [c == G1_INF for c in commit] == [v % R == 0 for v in EDGE]
    assert commit[1] == commit[4] == G1
    for i, r in enumerate(EDGE):
        assert (cts[i][0] == G1_INF and cts[i][2] == G2_INF) == (r % R == 0), i
    want, want_st = _composed_acks(ctx, keys, [EDGE, EDGE[::-1]], EDGE + EDGE[::-1])
    assert not ast.any() and not want_st.any()
    assert acts == want
    assert acts[0][0] == G1_INF and acts[0][2] == G2_INF


# ------------------------------------------------------------------ 4. key-set edges
def test_infinity_key_and_key_that_did_not_load(ctx):
    ks = KC.build("skg_producer", 5, 2, (1,), ((3, "not_on_curve"),))
    out, st = ctx.g1_mul(G1, [sk or 1 for sk in ks.sks])
    assert not st.any()
    keys = KC.key_bytes(ks, [bytes(out[48 * i:48 * i + 48]) for i in range(5)])
    assert keys[1] == G1_INF
    rng = random.Random(53)
    t = 1
    b, rs = _draw(rng, 3), _draw(rng, 5)
    rows, ars = [_draw(rng, 2), _draw(rng, 2)], _draw(rng, 10)
    with _Loaded(ctx, keys, n_bad=1) as kid:
        commit, cts, st = ctx.skg_part(kid, 5, t, b, rs)
        acts, ast = ctx.skg_acks(kid, 5, rows, ars)
    cm, cst = ctx.g1_mul(G1, skg._fr_le(b))
    assert not cst.any() and b"".join(commit) == bytes(cm)               # the commitment is unaffected
    msgs = skg.bivar_rows(ctx, b, t, 5)
    want, want_st = ctx.encrypt(keys, rs, msgs)
    assert list(st) == list(want_st) == [N.ACCEPT, N.ACCEPT, N.ACCEPT, N.DECODE_ERR, N.ACCEPT]
    assert cts == want
    assert cts[3] == (bytes(48), bytes(8 + 40 * (t + 1)), bytes(96))
    vals = [m for v in skg.ack_values(ctx, rows, 5) for m in v]
    want, want_st = ctx.encrypt(keys * 2, ars, vals)
    assert list(ast) == list(want_st) == [N.ACCEPT, N.ACCEPT, N.ACCEPT, N.DECODE_ERR, N.ACCEPT] * 2
    assert acts == want
    assert acts[3] == acts[8] == (bytes(48), bytes(40), bytes(96))


# ------------------------------------------------------------------ 5. round trip
def test_round_trip_through_decrypt_and_the_checks(ctx, pool):
    n, t = 7, 2
    sks, keys = pool[0][:n], pool[1][:n]
    rng = random.Random(72)
    b, rs = _draw(rng, 6), _draw(rng, n)
    with _Loaded(ctx, keys) as kid:
        commit, cts, st = ctx.skg_part(kid, n, t, b, rs)
        assert not st.any()
        got_rows = []
        for j in range(n):
            plain, dst = ctx.decrypt(sks[j], [cts[j][0]], [cts[j][2]], [cts[j][1]])
            assert dst[0] == N.ACCEPT
            row = wire.poly_from_wire(plain[0])
            assert row == skg._bivar_row(b, t, j + 1)
            assert int(ctx.skg_check_parts(t, j, commit, [row])[0]) == N.ACCEPT
            got_rows.append(row)
        ars = _draw(rng, 2 * n)
        acts, ast = ctx.skg_acks(kid, n, got_rows[:2], ars)
    assert not ast.any()
    for a in range(2):
        for j in range(n):
            u, v, w = acts[a * n + j]
            plain, dst = ctx.decrypt(sks[j], [u], [w], [v])
            assert dst[0] == N.ACCEPT
            assert wire.fr_value_from_wire(plain[0]) == skg._poly_eval(got_rows[a], j + 1), (a, j)


# ------------------------------------------------------------------ 6. the protocol
def test_one_call_era(ctx, pool, monkeypatch):
    n, t = 4, 1
    sks, keys = pool[0][:n], pool[1][:n]
    pub = {i: keys[i] for i in range(n)}
    nodes, parts = [], []
    for i in range(n):
        kg, part = skg.SyncKeyGen.new(ctx, i, sks[i], pub, t, one_call=True)
        assert kg.one_call and kg.rcpt_keyset is not None and len(part.rows) == n
        nodes.append(kg)
        parts.append(part)
    acks = []
    for node in nodes:
        for p, part in enumerate(parts):
            node.handle_part(p, part)
    for i, node in enumerate(nodes):
        outs = node.flush()
        assert [o[0] for o in outs] == ["valid"] * n, outs
        acks += [(i, o[1]) for o in outs]
    for node in nodes:
        for sender, ack in acks:
            node.handle_ack(sender, ack)
        assert all(f == [] for f in node.flush())
        assert node.is_ready()
    gen = [node.generate_keys() for node in nodes]
    assert all(g[0] == gen[0][0] and g[1] is not None and g[3] is not None for g in gen)
    own, st = ctx.g1_mul(G1, [g[1] for g in gen])
    assert not st.any() and b"".join(gen[0][2]) == bytes(own)
    for g in gen:
        ctx.keyset_free(g[3])
    for node in nodes:
        node.close()
        assert node.rcpt_keyset is None
    # an observer makes no Part and loads nothing

    def no_load(*a):
        raise AssertionError("an observer loaded a key set")
    monkeypatch.setattr(ctx, "keyset_load", no_load)
    obs, part = skg.SyncKeyGen.new(ctx, "observer", 1, pub, t, one_call=True)
    assert part is None and obs.rcpt_keyset is None and not obs.one_call
    # the default is the composed path: nothing is loaded either
    kg, part = skg.SyncKeyGen.new(ctx, 0, sks[0], pub, t)
    assert not kg.one_call and kg.rcpt_keyset is None and len(part.rows) == n


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors(ctx, pool):
    lib, null = ctx.lib, N._ptr(None)
    keys = pool[1][:4]
    b, r = np.zeros(32 * 3, np.uint8), np.zeros(32 * 4, np.uint8)
    cm, u, v, w = np.zeros(48 * 3, np.uint8), np.zeros(48 * 4, np.uint8), np.zeros(88 * 4, np.uint8), \
        np.zeros(96 * 4, np.uint8)
    st = np.zeros(4, np.int32)
    ERR_ARG = -1
    with _Loaded(ctx, keys) as kid:
        def part(k=kid, b_=N._ptr(b), r_=N._ptr(r), cm_=N._ptr(cm), u_=N._ptr(u), v_=N._ptr(v), w_=N._ptr(w),
                 st_=N._ptr(st), t=1):
            return lib.hbtc_skg_part(ctx.h, k, t, b_, r_, cm_, u_, v_, w_, st_)

        def acks(k=kid, n_rows=1, n_coeff=2, rows_=N._ptr(b), r_=N._ptr(r), u_=N._ptr(u), v_=N._ptr(v),
                 w_=N._ptr(w), st_=N._ptr(st)):
            return lib.hbtc_skg_acks(ctx.h, k, n_rows, n_coeff, rows_, r_, u_, v_, w_, st_)
        assert part() == 0 and acks() == 0
        assert part(k=kid + 1000) == ERR_ARG and acks(k=kid + 1000) == ERR_ARG    # an unknown key set
        for name in ("b_", "r_", "cm_", "u_", "v_", "w_", "st_"):
            assert part(**{name: null}) == ERR_ARG, name
        for name in ("rows_", "r_", "u_", "v_", "w_", "st_"):
            assert acks(**{name: null}) == ERR_ARG, name
        assert acks(n_rows=0) == ERR_ARG                                          # no items
        assert acks(n_coeff=0, rows_=null) == 0                                   # rows may be NULL then
        assert acks(n_rows=(1 << 20) // 4 + 1) == ERR_ARG                         # more than 2^20 items
        assert part(t=0xFFFFFFFF) == ERR_ARG and part(t=1 << 20) == ERR_ARG       # 2^32 bytes of rows and more
    assert part(k=kid) == ERR_ARG                                                 # the freed key set


def test_wrapper_splits_a_large_batch_by_rows(ctx, pool, monkeypatch):
    n = 4
    keys = pool[1][:n]
    rng = random.Random(90)
    rows, rs = [_draw(rng, 2) for _ in range(5)], _draw(rng, 5 * n)
    with _Loaded(ctx, keys) as kid:
        whole, st = ctx.skg_acks(kid, n, rows, rs)
        calls = []
        real = ctx.lib.hbtc_skg_acks

        class Lib:
            def __getattr__(self, name):
                return getattr(ctx.lib, name)

            def hbtc_skg_acks(self, h, k, n_rows, *rest):
                calls.append(n_rows)
                return real(h, k, n_rows, *rest)
        monkeypatch.setattr(N, "SKG_ACKS_MAX_ITEMS", 10)     # two rows of four items per call
        monkeypatch.setattr(ctx, "lib", Lib())
        split, sst = ctx.skg_acks(kid, n, rows, rs)
        monkeypatch.undo()
        chunks = [ctx.skg_acks(kid, n, rows[a:a + 2], rs[a * n:(a + 2) * n])[0] for a in (0, 2, 4)]
    assert calls == [2, 2, 1]
    assert not st.any() and not sst.any()
    assert split == whole == [c for ch in chunks for c in ch]
