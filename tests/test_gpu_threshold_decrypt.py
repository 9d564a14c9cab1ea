"""ThresholdDecryption to the plaintext on the GPU: hbtc_threshold_decrypt (shares -> statuses -> g
-> plaintext in one call), hbtc_pad_xor_dev, hbtc_dec_epoch_submit_plain, and hbtc_decrypt with g
and H kept on the device.

Restated with the C oracle (pairing checks, the G1 combine, hash_g1_g2) and
oracle.threshold_crypto (hash_bytes, decrypt).  Bar: bit-equal statuses, g and plaintexts; the
ranges of ciphertexts that do not combine are all zero."""
import json
import os
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import cbaseline as C
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
G2 = B.g2_compress(B.G2_GEN)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = [0, 1, 15, 16, 17, 40, 64, 65, 136, 137, 1000]
LONG = 70001  # 4,376 pad blocks: many workgroups of the pad and an odd tail


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def _pad(g48, n):
    return TC.hash_bytes(B.g1_decompress(bytes(g48)), n)


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def _keys(ctx, rng, n, t):
    """n key shares of a random degree t - 1 polynomial: (secret shares, compressed pk shares)."""
    coeffs = [rng.randrange(1, R) for _ in range(t)]
    sks = []
    for i in range(n):
        acc = 0
        for c in reversed(coeffs):
            acc = (acc * (i + 1) + c) % R
        sks.append(acc)
    pk, st = ctx.g1_mul(G1, sks)
    assert not st.any()
    return sks, pk


def _round(ctx, rng, sks, senders, bad=()):
    """One ciphertext's (H, w) and the shares of `senders`: H = h G2, w = r h G2, share_i = sk_i r G1
    (so e(share, H) == e(pk, w)); positions in `bad` get a wrong scalar."""
    r, h = rng.randrange(1, R), rng.randrange(1, R)
    scal = [(sks[i] * r + (1 + j if j in bad else 0)) % R for j, i in enumerate(senders)]
    return C.g2_mul(G2, h), C.g2_mul(G2, r * h % R), scal


def _restate(pk, H, w, off, idx, shares, t, vs):
    """(statuses, g, inst_status, plaintexts) by the reference's rules: each share by the pairing
    check of verify_decryption_share, the first t verified shares interpolated, v XOR hash_bytes."""
    n_keys = len(pk) // 48
    sh = bytes(shares)
    st, gs, cst, plain = [], [], [], []
    for k in range(len(off) - 1):
        kept = []
        w_ok = C.g2_mul(w[k], 1) is not None and C.g2_mul(H[k], 1) is not None
        for j in range(off[k], off[k + 1]):
            s = sh[48 * j:48 * j + 48]
            if not w_ok:
                st.append(N.INSTANCE_ERR)
            elif idx[j] >= n_keys:
                st.append(N.UNKNOWN_SENDER)
            else:
                ok = C.pairing_eq(s, H[k], bytes(pk[48 * idx[j]:48 * idx[j] + 48]), w[k])
                st.append(N.DECODE_ERR if ok is None else (N.ACCEPT if ok else N.REJECT))
            if st[-1] == N.ACCEPT:
                kept.append((idx[j], s))
        c, g = C.combine(1, [i for i, _ in kept[:t]], [s for _, s in kept[:t]], t)
        cst.append(c)
        gs.append(g if c == 0 else bytes(48))
        plain.append(_xor(vs[k], _pad(g, len(vs[k]))) if c == 0 else None)
    return np.asarray(st, np.int32), gs, np.asarray(cst, np.int32), plain


def _check(got, want, tag=""):
    st, plain, g, cst = got
    wst, wg, wcst, wplain = want
    assert (np.asarray(st) == wst).all(), tag
    assert (np.asarray(cst) == wcst).all(), tag
    assert [bytes(x) for x in g] == wg, tag
    assert plain == wplain, tag


# ------------------------------------------------------------------------------------ 1. golden
def test_golden_c1(ctx):
    with open(os.path.join(GOLDEN, "c1_dec.json")) as fh:
        d = json.load(fh)
    b = bytes.fromhex
    ks, bad = ctx.keyset_load([b(p) for p in d["pk_shares"]])
    assert bad == 0
    names = {v: k for k, v in N.STATUS_NAMES.items()}
    idx = [it["idx"] for it in d["items"]]
    shares = [b(it["share"]) for it in d["items"]]
    want_st = [names[it["expected"]] for it in d["items"]]
    first = next(c for c in d["combines"] if c["name"] == "first_t")
    v = b(d["v"])
    args = (ks, [b(d["H"])], [b(d["w"])])
    st, plain, g, cst = ctx.threshold_decrypt(*args, [len(idx)], idx, shares, d["t"], [v])
    assert list(st) == want_st
    assert list(cst) == [N.ACCEPT]  # the first t ACCEPTed items are the golden first_t shares
    assert g[0] == b(first["g"])
    assert plain[0] == b(d["plaintext"])
    assert plain[0] == TC.decrypt(d["t"], [(i, B.g1_decompress(b(s))) for i, s in zip(first["idx"], first["shares"])],
                                  (None, v, None))[0]
    off = np.asarray([0, len(idx)], np.uint32)
    st2, g2, cst2, p2, voff = ctx.dec_epoch_submit_plain(*args, off, idx, b"".join(shares), d["t"], [v]).wait()
    assert list(st2[:len(idx)]) == want_st and cst2[0] == N.ACCEPT
    assert g2[0].tobytes() == b(first["g"])
    assert p2[voff[0]:voff[1]].tobytes() == b(d["plaintext"])


# ------------------------------------------------------------------------- 2. small combine path
@pytest.fixture(scope="module")
def small(ctx):
    """t = 2, N = 4, 15 ciphertexts: every length of LENGTHS, the long one between short ones, and
    the failure cases; the restatement is computed once."""
    rng = random.Random(4242)
    sks, pk = _keys(ctx, rng, 4, 2)
    lens = LENGTHS + [LONG, 33, 5, 48]
    special = {
        2: dict(bad=(0,)),                  # a corrupted share inside the first t: skipped
        4: dict(bad=(0, 2)),                # one valid share: NOT_ENOUGH_SHARES
        6: dict(senders=[1, 1, 2]),         # a repeated index among the first t: DUPLICATE_ENTRY
        8: dict(break_w=True),              # w does not decode: INSTANCE_ERR, then NOT_ENOUGH_SHARES
        10: dict(senders=[7, 0, 3]),        # an unknown sender first
        12: dict(bad=(0, 1, 2)),            # the short neighbour behind the long item: gated out
        14: dict(senders=[]),               # no shares at all
    }
    H, w, idx, scal, counts, vs = [], [], [], [], [], []
    for k, n in enumerate(lens):
        sp = special.get(k, {})
        senders = sp.get("senders", [0, 1, 2])
        known = [i if i < 4 else 0 for i in senders]
        Hk, wk, sc = _round(ctx, rng, sks, known, sp.get("bad", ()))
        if sp.get("break_w"):
            wk = bytes([wk[0] & 0x7F]) + wk[1:]  # compression flag cleared
        H.append(Hk)
        w.append(wk)
        idx += senders
        scal += sc
        counts.append(len(senders))
        vs.append(bytes(rng.randrange(256) for _ in range(n)))
    shares, st = ctx.g1_mul(G1, scal)
    assert not st.any()
    off = np.zeros(len(counts) + 1, np.uint32)
    off[1:] = np.cumsum(counts)
    want = _restate(bytes(pk), H, w, off, idx, shares, 2, vs)
    ks, _ = ctx.keyset_load(pk)
    return dict(ks=ks, H=H, w=w, off=off, idx=idx, shares=shares, vs=vs, want=want)


def test_small_combine_path(ctx, small):
    s = small
    wst, wg, wcst, wplain = s["want"]
    # the cases are what they were built to be
    assert list(wcst[[2, 4, 6, 8, 10, 12, 14]]) == [N.ACCEPT, N.NOT_ENOUGH_SHARES, N.DUPLICATE_ENTRY,
                                                    N.NOT_ENOUGH_SHARES, N.ACCEPT, N.NOT_ENOUGH_SHARES,
                                                    N.NOT_ENOUGH_SHARES]
    assert wst[s["off"][2]] == N.REJECT and wst[s["off"][10]] == N.UNKNOWN_SENDER
    assert (wst[s["off"][8]:s["off"][9]] == N.INSTANCE_ERR).all()
    got = ctx.threshold_decrypt(s["ks"], s["H"], s["w"], None, s["idx"], s["shares"], 2, s["vs"],
                                offsets=s["off"])
    _check(got, s["want"])
    # the raw buffer: ranges of ciphertexts that do not combine are zero, their neighbours intact
    st, g, cst, plain, voff = ctx.dec_epoch_submit_plain(s["ks"], s["H"], s["w"], s["off"], s["idx"],
                                                         s["shares"], 2, s["vs"]).wait()
    assert (st[:len(wst)] == wst).all() and (cst[:len(wcst)] == wcst).all()
    for k, p in enumerate(wplain):
        rng_k = plain[voff[k]:voff[k + 1]].tobytes()
        assert rng_k == (p if p is not None else bytes(len(s["vs"][k]))), k
        assert g[k].tobytes() == wg[k], k
    assert int(voff[-1]) == sum(len(v) for v in s["vs"])


# ----------------------------------------------------- 3. Pippenger combine and RLC verification
def test_pippenger_path_and_rlc(ctx):
    """t = 65 (above the one-launch combine's 64), 4 x 66 = 264 shares (above the 256-share
    exact-only limit), one corrupted share among the first t."""
    rng = random.Random(6565)
    n, t = 66, 65
    sks, pk = _keys(ctx, rng, n, t)
    H, w, scal, vs = [], [], [], []
    for k, ln in enumerate([40, 1000, 40, 1000]):
        Hk, wk, sc = _round(ctx, rng, sks, list(range(n)), bad=(7,) if k == 1 else ())
        H.append(Hk)
        w.append(wk)
        scal += sc
        vs.append(bytes(rng.randrange(256) for _ in range(ln)))
    shares, st = ctx.g1_mul(G1, scal)
    assert not st.any()
    idx = np.tile(np.arange(n, dtype=np.uint32), 4)
    off = np.arange(5, dtype=np.uint32) * n
    ks, _ = ctx.keyset_load(pk)
    got = ctx.threshold_decrypt(ks, H, w, None, idx, shares, t, vs, offsets=off)
    st, plain, g, cst = got
    # (b): the composed path
    st_b = ctx.verify_dec_shares(ks, H, w, None, idx, shares, offsets=off)
    assert (st == st_b).all() and st[n + 7] == N.REJECT and (np.delete(st, n + 7) == N.ACCEPT).all()
    sh = np.asarray(shares, np.uint8).reshape(-1, 48)
    sel = [[i for i in range(off[k], off[k + 1]) if st_b[i] == N.ACCEPT][:t] for k in range(4)]
    flat = [i for s in sel for i in s]
    g_b, cst_b = ctx.combine_dec([len(s) for s in sel], idx[flat], sh[flat].reshape(-1), t)
    assert (cst == cst_b).all() and (cst == N.ACCEPT).all() and g == g_b
    assert plain == N.xor_hash_bytes_batch(g_b, vs)
    # the C oracle's combine and hash_bytes
    for k in range(4):
        c, gk = C.combine(1, [int(idx[i]) for i in sel[k]], [sh[i].tobytes() for i in sel[k]], t)
        assert c == 0 and gk == g[k]
        assert plain[k] == _xor(vs[k], _pad(gk, len(vs[k])))


# ------------------------------------------------------------------------ 4. composed equality
@pytest.mark.parametrize("n_ct", [1, 63, 64, 65])
def test_equals_composed_calls_and_pad_xor(ctx, n_ct):
    rng = random.Random(900 + n_ct)
    sks, pk = _keys(ctx, rng, 4, 2)
    ks, _ = ctx.keyset_load(pk)
    H, w, scal, vs = [], [], [], []
    for k in range(n_ct):
        bad = {0: (), 1: (1,), 2: (0, 1), 3: (0, 1, 2)}[k % 7] if k % 7 < 4 else ()
        Hk, wk, sc = _round(ctx, rng, sks, [0, 1, 2], bad)
        H.append(Hk)
        w.append(wk)
        scal += sc
        vs.append(bytes(rng.randrange(256) for _ in range(LENGTHS[k % len(LENGTHS)])))
    shares, _ = ctx.g1_mul(G1, scal)
    idx = np.tile(np.arange(3, dtype=np.uint32), n_ct)
    off = np.arange(n_ct + 1, dtype=np.uint32) * 3
    st, plain, g, cst = ctx.threshold_decrypt(ks, H, w, None, idx, shares, 2, vs, offsets=off)
    st_b = ctx.verify_dec_shares(ks, H, w, None, idx, shares, offsets=off)
    sh = np.asarray(shares, np.uint8).reshape(-1, 48)
    sel = [[i for i in range(off[k], off[k + 1]) if st_b[i] == N.ACCEPT][:2] for k in range(n_ct)]
    flat = [i for s in sel for i in s]
    g_b, cst_b = ctx.combine_dec([len(s) for s in sel], idx[flat], sh[flat].reshape(-1), 2)
    assert (st == st_b).all() and (cst == cst_b).all()
    if n_ct > 3:
        assert cst[3] == N.NOT_ENOUGH_SHARES and cst[2] == N.NOT_ENOUGH_SHARES and cst[1] == N.ACCEPT
    p_b = N.xor_hash_bytes_batch(g_b, vs)
    for k in range(n_ct):
        if cst[k] == N.ACCEPT:
            assert g[k] == g_b[k] and plain[k] == p_b[k], k
        else:
            assert g[k] == bytes(48) and plain[k] is None, k
    # pad_xor on the downloaded and re-uploaded g, gated on the combine's statuses
    vbuf, voff = N._msg_batch(vs)
    gbuf = np.frombuffer(b"".join(g_b), np.uint8).copy()
    gate = np.ascontiguousarray(cst_b, np.int32)
    total = max(int(voff[-1]), 1)
    d_g, d_gate = ctx.dev_alloc(gbuf.size), ctx.dev_alloc(gate.nbytes)
    d_v, d_out = ctx.dev_alloc(total), ctx.dev_alloc(total)
    try:
        ctx.dev_upload(d_g, gbuf)
        ctx.dev_upload(d_gate, gate)
        ctx.dev_upload(d_v, vbuf)
        ctx.pad_xor(d_g, d_gate, voff, d_v, d_out)
        out = np.zeros(total, np.uint8)
        ctx.dev_download(out, d_out)
    finally:
        for p in (d_g, d_gate, d_v, d_out):
            ctx.dev_free(p)
    for k in range(n_ct):
        want = p_b[k] if cst_b[k] == N.ACCEPT else bytes(len(vs[k]))
        assert out[voff[k]:voff[k + 1]].tobytes() == want, k


# ---------------------------------------------------------------------------------- 5. pipelining
def test_five_epochs_in_flight(ctx, small):
    """Five submissions with different v (the fifth completes the oldest), waited out of order."""
    s = small
    wst, wg, wcst, wplain = s["want"]
    rng = random.Random(55)
    pend, vss = [], []
    for e in range(5):
        vs = [bytes(rng.randrange(256) for _ in range(len(v))) for v in s["vs"]]
        vss.append(vs)
        pend.append(ctx.dec_epoch_submit_plain(s["ks"], s["H"], s["w"], s["off"], s["idx"], s["shares"], 2, vs))
    for e in (3, 0, 4, 1, 2):
        st, g, cst, plain, voff = pend[e].wait()
        assert (st[:len(wst)] == wst).all() and (cst[:len(wcst)] == wcst).all(), e
        for k, p in enumerate(wplain):
            # the pad depends on g alone: this epoch's plaintext = its v XOR (small's v XOR plaintext)
            want = bytes(len(vss[e][k])) if p is None else _xor(vss[e][k], _xor(s["vs"][k], p))
            assert plain[voff[k]:voff[k + 1]].tobytes() == want, (e, k)
    with pytest.raises(N.HbtcError):  # t == 0 is an argument error
        ctx.dec_epoch_submit_plain(s["ks"], s["H"], s["w"], s["off"], s["idx"], s["shares"], 0, s["vs"])


# ------------------------------------------------------------------- 6. hbtc_decrypt (SecretKey)
@pytest.fixture(scope="module")
def sk_cases(ctx):
    """encrypt -> (us, ws, vs) over the length list, one tampered w and one u that does not decode,
    with the restated (status, plaintext) of every item."""
    rng = random.Random(777)
    sk = rng.randrange(1, R)
    pk = C.g1_mul(G1, sk)
    lens = LENGTHS + [LONG, 33, 5]
    msgs = [bytes(rng.randrange(256) for _ in range(n)) for n in lens]
    cts, st = ctx.encrypt(pk, [rng.randrange(1, R) for _ in lens], msgs)
    assert not st.any()
    us, vs, ws = [c[0] for c in cts], [c[1] for c in cts], [c[2] for c in cts]
    ws[5] = ws[6]                                # a valid point, the wrong one: REJECT
    us[9] = bytes([us[9][0] & 0x7F]) + us[9][1:]  # compression flag cleared: DECODE_ERR
    want = []
    for u, v, w in zip(us, vs, ws):
        ok = C.pairing_eq(G1, w, u, C.hash_g1_g2(u, v))  # Ciphertext::verify
        if ok is None:
            want.append((N.DECODE_ERR, None))
        elif not ok:
            want.append((N.REJECT, None))
        else:
            want.append((N.ACCEPT, _xor(v, _pad(C.g1_mul(u, sk), len(v)))))
    assert [s for s, _ in want].count(N.ACCEPT) == len(lens) - 2
    assert all(p == m for (s, p), m in zip(want, msgs) if s == N.ACCEPT)  # the round trip
    return sk, us, ws, vs, want


@pytest.mark.parametrize("mode,exact_below", [(N.MODE_RLC, 0), (N.MODE_RLC, 256), (N.MODE_PER_SHARE, 256)])
def test_secret_key_decrypt_on_device(ctx, sk_cases, mode, exact_below):
    sk, us, ws, vs, want = sk_cases
    ctx.set_verify_mode(mode)
    ctx.set_exact_below(exact_below)
    ctx.timing_reset()
    ctx.timing_enable(True)
    try:
        plain, st = ctx.decrypt(sk, us, ws, vs)
        # the pad ran on the device, behind the multiplication: one seed + pad span per call
        assert ctx.timing_read("dec_pad")[1] == 1
        ctx.timing_enable(False)
        # the raw output: rejected ranges are zero
        buf, off = N._msg_batch(vs)
        out = np.full(int(off[-1]), 0xAA, np.uint8)
        st2 = np.zeros(len(vs), np.int32)
        k = np.frombuffer(int(sk).to_bytes(32, "little"), np.uint8).copy()
        ub, wb = N._join(us, 48), N._join(ws, 96)  # held: the call reads them through raw pointers
        rc = ctx.lib.hbtc_decrypt(ctx.h, len(vs), N._ptr(k), N._ptr(ub), N._ptr(wb), N._ptr(buf), N._ptr(off),
                                  N._ptr(out), N._ptr(st2))
        assert rc == 0
    finally:
        ctx.timing_enable(False)
        ctx.set_verify_mode(N.MODE_RLC)
        ctx.set_exact_below(256)
    assert list(st) == [s for s, _ in want] and list(st2) == list(st)
    assert plain == [p for _, p in want]
    for i, (s, p) in enumerate(want):
        assert out[off[i]:off[i + 1]].tobytes() == (p if p is not None else bytes(len(vs[i]))), i
