"""Every consumer of a loaded key set on key sets that hold keys at infinity (the share of node i
when the era's polynomial has a root at i + 1) and keys that did not load (hbtc_keyset_load's
n_bad): the share checks on every route, both combine routes of hbtc_coin_decide with and without
the speculation, hbtc_coin_epoch_submit, hbtc_threshold_decrypt and hbtc_dec_epoch_submit_plain,
both routes of hbtc_verify_signed_msgs, the set hbtc_skg_generate leaves loaded and the
multi-device node.

Reference: the construction of tests/keyset_cases.py (Python integers; tests/test_keyset_cases.py
holds it against the oracle's pairing).  Points are made with hbtc_g1_mul / hbtc_g2_mul, pinned
against the oracle by tests/test_gpu_parity.py; parity bits and hash_bytes come from the oracle.
Every key set is loaded in the place of a freed one (_load), so that the table rows the library
never writes for such keys hold stale points instead of zeros.
Bar: identical statuses, bytes and parity bits, every array compared whole."""
import os
import random

import numpy as np
import pytest

import keyset_cases as KC
from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
G2 = B.g2_compress(B.G2_GEN)
SCHEDULES = (N.CHECK_AUTO, N.CHECK_PLAIN_FIRST, N.CHECK_PAIR_SUBS, N.CHECK_PAIR_LEAVES)
EXACT_BELOW = 256  # the context's default


def _context(spec):
    old = os.environ.get("HBTC_COIN_SPEC")
    os.environ["HBTC_COIN_SPEC"] = spec
    try:
        return N.Context(0)
    finally:
        if old is None:
            os.environ.pop("HBTC_COIN_SPEC", None)
        else:
            os.environ["HBTC_COIN_SPEC"] = old


@pytest.fixture(scope="module")
def ctx():
    c = _context("1")
    yield c
    c.close()


@pytest.fixture(scope="module")
def nospec():
    """A second context for the coin rounds without speculation: the switch is read at creation."""
    c = _context("0")
    yield c
    c.close()


def _split(buf, size):
    raw = bytes(buf)
    return [raw[p:p + size] for p in range(0, len(raw), size)]


def _keys(ctx, ks):
    """The key set's encodings and its master key."""
    out, st = ctx.g1_mul(G1, [sk or 1 for sk in ks.sks] + [KC.master(ks)])
    assert not st.any()
    enc = _split(out, 48)
    return KC.key_bytes(ks, enc[:ks.N]), enc[ks.N]


def _load(ctx, ks):
    """The key set loaded where a freed set of N ordinary keys has just been: an allocation of the
    same size usually comes back at the same place, so the table rows that are never written for
    this set hold another set's points rather than a fresh allocation's zeros.  (A row of zeros
    hides a read: adding (0, 0) to itself doubles a point with y = 0, the point at infinity.)"""
    keys, mpk = _keys(ctx, ks)
    ghost, st = ctx.g1_mul(G1, [i + 2 for i in range(ks.N)])
    assert not st.any()
    gid, bad = ctx.keyset_load(ghost)
    assert bad == 0
    ctx.keyset_free(gid)
    kid, bad = ctx.keyset_load(keys)
    assert bad == len(ks.B)
    ctx.keyset_set_master(kid, mpk)
    return kid


def _encode(ctx, group, insts, mults):
    """The items' encodings: [s m_k] G of item (idx, s) of instance k; s = 0 is the point at
    infinity, s = None a point without its compression flag."""
    mul, gen, size, inf = (ctx.g1_mul, G1, 48, KC.G1_INF) if group == 1 else (ctx.g2_mul, G2, 96, KC.G2_INF)
    flat = [(s, m) for inst, m in zip(insts, mults) for _, s in inst]
    out, st = mul(gen, [s * m % R if s else 1 for s, m in flat])
    assert not st.any()
    pts = _split(out, size)
    for p, (s, _) in enumerate(flat):
        if s is None:
            pts[p] = bytes([pts[p][0] & 0x7F]) + pts[p][1:]
        elif s % R == 0:
            pts[p] = inf
    return pts


class Round:
    """Instances as one call's arguments.  SignatureShares: H_k = [h_k] G2, item [s h_k] G2.
    DecryptionShares: u_k = [r_k] G1, H_k = [h_k] G2, w_k = [r_k h_k] G2, item [s r_k] G1."""

    def __init__(self, ctx, ks, insts, seed):
        rng = random.Random(seed)
        self.ks, self.insts = ks, list(insts)
        n = len(self.insts)
        self.hs = [rng.randrange(1, R) for _ in range(n)]
        self.rs = [rng.randrange(1, R) for _ in range(n)]
        out, st = ctx.g2_mul(G2, self.hs + [r * h % R for r, h in zip(self.rs, self.hs)])
        assert not st.any()
        pts = _split(out, 96)
        self.H, self.w = pts[:n], pts[n:]
        self.counts = [len(i) for i in self.insts]
        self.off = [0] + list(np.cumsum(self.counts))
        self.idx = [i for inst in self.insts for i, _ in inst]
        self.sigs = _encode(ctx, 2, self.insts, self.hs)
        self.shares = _encode(ctx, 1, self.insts, self.rs)
        self.want = [s for inst in self.insts for s in KC.statuses(ks, inst)]
        self.comb = [KC.combine(ks, inst) for inst in self.insts]
        self.want_coin = [st for st, _ in self.comb]

    def want_points(self, ctx, group):
        """The combined points [f(0) m_k] G of the ACCEPTed instances, zeros for the others."""
        mul, gen, size, mults = (ctx.g1_mul, G1, 48, self.rs) if group == 1 else (ctx.g2_mul, G2, 96, self.hs)
        out, st = mul(gen, [k * m % R if k is not None else 1 for (_, k), m in zip(self.comb, mults)])
        assert not st.any()
        return [p if k is not None else bytes(size) for p, (_, k) in zip(_split(out, size), self.comb)]


def _parity(sig, status):
    if status != N.ACCEPT:
        return 0
    return int(TC.signature_parity(B.g2_decompress(sig, check_subgroup=False)))


def _defaults(ctx):
    ctx.set_verify_mode(N.MODE_RLC)
    ctx.set_check_schedule(N.CHECK_AUTO)
    ctx.set_rlc_bits(128)
    ctx.set_exact_below(EXACT_BELOW)
    ctx.set_sender_tracking(True)


def _routes(ctx, call, want):
    """call() on every route of the share checks: per-share mode; the RLC mode without the exact
    small-call path at both scalar widths under every schedule; with sender tracking on, twice (a Z
    sender lies in the batch: in the second call its shares go straight to the leaf checks); with
    the default exact-below value (these calls are below it: exact checks only)."""
    def check(tag):
        st = np.asarray(call()).tolist()
        assert st == want, (tag, [(p, a, b) for p, (a, b) in enumerate(zip(st, want)) if a != b])

    try:
        ctx.set_sender_tracking(False)
        ctx.set_exact_below(0)
        ctx.set_verify_mode(N.MODE_PER_SHARE)
        check("per-share")
        ctx.set_verify_mode(N.MODE_RLC)
        for bits in (128, 64):
            ctx.set_rlc_bits(bits)
            for sched in SCHEDULES:
                ctx.set_check_schedule(sched)
                check((bits, sched))
        ctx.set_rlc_bits(128)
        ctx.set_check_schedule(N.CHECK_AUTO)
        ctx.set_sender_tracking(True)
        check("tracking, the call with the lie")
        check("tracking, the call after the lie")
        ctx.set_exact_below(EXACT_BELOW)
        check("default exact-below")
    finally:
        _defaults(ctx)


@pytest.fixture(scope="module")
def big(ctx):
    """The large set loaded, and batch (A, B, C) on it."""
    ks = KC.large()
    kid = _load(ctx, ks)
    rd = Round(ctx, ks, KC.share_batch(ks).values(), "big")
    assert rd.counts == [70, 8, 64] and sum(rd.counts) < EXACT_BELOW
    assert sorted(set(rd.want)) == [N.ACCEPT, N.REJECT, N.DECODE_ERR, N.UNKNOWN_SENDER]
    yield ks, kid, rd
    ctx.keyset_free(kid)


# ------------------------------------------------------------------------- a, b: the share checks
def test_signature_shares_on_every_route(ctx, big):
    ks, kid, rd = big
    _routes(ctx, lambda: ctx.verify_sig_shares(kid, rd.H, rd.counts, rd.idx, rd.sigs), rd.want)


def test_decryption_shares_on_every_route(ctx, big):
    ks, kid, rd = big
    _routes(ctx, lambda: ctx.verify_dec_shares(kid, rd.H, rd.w, rd.counts, rd.idx, rd.shares), rd.want)


def test_only_later_copies_take_the_exact_path(ctx, big):
    """Instances B and C as a call of their own, every share valid.  A key at infinity adds nothing
    to the G1 side of a tile's sums and its share at infinity nothing to the G2 side, so both tiles
    pass their group checks.  SignatureShares carry a scalar per item: no share reaches the exact
    leaf checks.  DecryptionShares carry one per sender, and the duplicate guard sends the later
    copies of a sender there (five in B, one in C), under a key at infinity.  A term read from
    the never-written table rows of such a key would fail its tile and send all of it there."""
    ks, kid, rd = big
    insts = rd.insts[1:]
    later = sum(sum(1 for p, (i, _) in enumerate(inst) if i in [j for j, _ in inst[:p]]) for inst in insts)
    assert later == 6 and all(len(inst) <= 64 for inst in insts)
    a, b = rd.off[1], rd.off[3]
    H, w, counts, idx = rd.H[1:], rd.w[1:], rd.counts[1:], rd.idx[a:b]
    try:
        ctx.set_sender_tracking(False)
        ctx.set_exact_below(0)
        for bits in (128, 64):
            ctx.set_rlc_bits(bits)
            st = ctx.verify_sig_shares(kid, H, counts, idx, rd.sigs[a:b])
            assert st.tolist() == rd.want[a:b] == [N.ACCEPT] * (b - a), bits
            assert ctx.rlc_last_leaves() == 0, ("sig", bits, ctx.rlc_last_leaves())
            st = ctx.verify_dec_shares(kid, H, w, counts, idx, rd.shares[a:b])
            assert st.tolist() == rd.want[a:b], bits
            assert ctx.rlc_last_leaves() == later, ("dec", bits, ctx.rlc_last_leaves())
    finally:
        _defaults(ctx)


# -------------------------------------------------------------------------- c, d: coins, t <= 64
def _check_coin(got, rd, want_sig, tag):
    st, sig, par, cst = got
    n = len(rd.insts)
    assert np.asarray(st)[:len(rd.want)].tolist() == rd.want, tag
    assert [int(c) for c in np.asarray(cst)[:n]] == rd.want_coin, tag
    assert [bytes(sig[k]) for k in range(n)] == want_sig, tag
    want_par = [_parity(s, c) for s, c in zip(want_sig, rd.want_coin)]
    assert [int(p) for p in np.asarray(par)[:n]] == want_par, tag


@pytest.mark.parametrize("reps", [1, 11], ids=["speculative", "too_large_to_speculate"])
@pytest.mark.parametrize("kind", KC.BAD_KINDS)
def test_coin_decide_small(ctx, nospec, kind, reps):
    """Instances i .. v once (25 subsets: speculated on `ctx`, not on `nospec`) and eleven times
    (275 subsets: no speculation on either).  In the speculated call the subsets that hold the
    bad key's item are combined from its never-written table rows; none of them may be committed."""
    ks = KC.small(kind)
    insts = list(KC.coin_small(ks).values()) * reps
    t = ks.t
    assert (len(insts) * (t + 1) <= 256) == (reps == 1)
    for c, tag in ((ctx, "spec"), (nospec, "nospec")):
        kid = _load(c, ks)
        try:
            rd = Round(c, ks, insts, "coin_small:%s:%d" % (kind, reps))
            assert rd.want_coin[:5] == [N.ACCEPT] * 4 + [N.NOT_ENOUGH_SHARES]
            want_sig = rd.want_points(c, 2)
            _check_coin(c.coin_decide(kid, rd.H, rd.counts, rd.idx, rd.sigs, t), rd, want_sig, (tag, "decide"))
            _check_coin(c.coin_epoch_submit(kid, rd.H, rd.off, rd.idx, rd.sigs, t).wait(), rd, want_sig,
                        (tag, "ticket"))
        finally:
            c.keyset_free(kid)


# ------------------------------------------------------------------------------- e: coins, t = 65
def _composed(ctx, kid, rd, t, mpk):
    """hbtc_verify_sig_shares, hbtc_combine_sigs over the first t ACCEPTed, hbtc_verify_sigs."""
    st = ctx.verify_sig_shares(kid, rd.H, rd.counts, rd.idx, rd.sigs)
    sel_counts, sel_idx, sel_sigs = [], [], []
    for k in range(len(rd.insts)):
        acc = [j for j in range(rd.off[k], rd.off[k + 1]) if st[j] == N.ACCEPT][:t]
        sel_counts.append(len(acc))
        sel_idx += [rd.idx[j] for j in acc]
        sel_sigs += [rd.sigs[j] for j in acc]
    out, par, cst = ctx.combine_sigs(sel_counts, sel_idx, sel_sigs, t)
    coin = [int(c) for c in cst]
    ok = [k for k, c in enumerate(coin) if c == N.ACCEPT]
    if ok:
        v = ctx.verify_sigs([mpk] * len(ok), [rd.H[k] for k in ok], [out[k] for k in ok])
        for k, r in zip(ok, v):
            coin[k] = int(r)
    return st.tolist(), out, [int(p) for p in par], coin


def test_coin_large(ctx, big):
    """t = 65: the selection holds the three shares at infinity and steps over every bad key; the
    second instance has 64 acceptable shares.  Blocking and ticketed, on the exact route (the call
    is below the default exact-below) and on the batch route, and the composed calls."""
    ks, kid, _ = big
    t = ks.t
    rd = Round(ctx, ks, KC.coin_large(ks).values(), "coin_large")
    assert rd.want_coin == [N.ACCEPT, N.NOT_ENOUGH_SHARES] and sum(rd.counts) < EXACT_BELOW
    want_sig = rd.want_points(ctx, 2)
    _, mpk = _keys(ctx, ks)
    try:
        for below in (EXACT_BELOW, 0):
            ctx.set_exact_below(below)
            _check_coin(ctx.coin_decide(kid, rd.H, rd.counts, rd.idx, rd.sigs, t), rd, want_sig, (below, "decide"))
            _check_coin(ctx.coin_epoch_submit(kid, rd.H, rd.off, rd.idx, rd.sigs, t).wait(), rd, want_sig,
                        (below, "ticket"))
            st, out, par, coin = _composed(ctx, kid, rd, t, mpk)
            assert st == rd.want and coin == rd.want_coin and out == want_sig, below
            assert par == [_parity(s, c) for s, c in zip(want_sig, rd.want_coin)], below
    finally:
        _defaults(ctx)


# ----------------------------------------------------------------------------------- f: plaintext
def _check_plain(ctx, kid, rd, t, tag):
    rng = random.Random("plain:%s" % (tag,))
    vs = [bytes(rng.randrange(256) for _ in range(n)) for n in (33, 1, 64, 7)[:len(rd.insts)]]
    want_g = rd.want_points(ctx, 1)
    want_plain = []
    for v, g, c in zip(vs, want_g, rd.want_coin):
        pad = TC.hash_bytes(B.g1_decompress(g, check_subgroup=False), len(v)) if c == N.ACCEPT else None
        want_plain.append(bytes(a ^ b for a, b in zip(v, pad)) if pad is not None else None)
    st, plain, g, cst = ctx.threshold_decrypt(kid, rd.H, rd.w, rd.counts, rd.idx, rd.shares, t, vs)
    assert st.tolist() == rd.want and cst.tolist() == rd.want_coin, tag
    assert g == want_g and plain == want_plain, tag
    st, g, cst, flat, voff = ctx.dec_epoch_submit_plain(kid, rd.H, rd.w, rd.off, rd.idx, rd.shares, t, vs).wait()
    n = len(rd.insts)
    assert st[:len(rd.want)].tolist() == rd.want and cst[:n].tolist() == rd.want_coin, tag
    # a failed combine's g is not part of the ticket's contract; its plaintext is zeros
    assert [bytes(g[k]) for k in range(n) if rd.want_coin[k] == N.ACCEPT] == \
        [p for p, c in zip(want_g, rd.want_coin) if c == N.ACCEPT], tag
    assert [bytes(flat[voff[k]:voff[k + 1]]) for k in range(n)] == \
        [p if p is not None else bytes(len(v)) for p, v in zip(want_plain, vs)], tag


@pytest.mark.parametrize("kind", KC.BAD_KINDS)
def test_plaintext_small(ctx, kind):
    ks = KC.small(kind)
    coin = KC.coin_small(ks)
    kid = _load(ctx, ks)
    try:
        rd = Round(ctx, ks, [coin["i"], coin["ii"], coin["v"]], "plain_small:" + kind)
        assert rd.want_coin == [N.ACCEPT, N.ACCEPT, N.NOT_ENOUGH_SHARES]
        _check_plain(ctx, kid, rd, ks.t, kind)
    finally:
        ctx.keyset_free(kid)


def test_plaintext_large(ctx, big):
    ks, kid, _ = big
    rd = Round(ctx, ks, [KC.coin_large(ks)["all_z"]], "plain_large")
    assert rd.want_coin == [N.ACCEPT]
    _check_plain(ctx, kid, rd, ks.t, "large")


# ------------------------------------------------------------------------------ g: signed messages
def test_signed_messages(ctx):
    ks = KC.signed()
    items = KC.signed_items(ks)
    rng = random.Random("signed msgs")
    msgs = [bytes(rng.randrange(256) for _ in range(n)) for _, _, n in items]
    signer = [j for j, _, _ in items]
    sigs = [KC.G2_INF] * len(items)
    for s in sorted({s for _, s, _ in items if s}):  # one hbtc_sign_shares call per secret
        pos = [p for p, it in enumerate(items) if it[1] == s]
        made = ctx.sign_shares(s, [msgs[p] for p in pos], want_H=False)[0]
        for p, sg in zip(pos, made):
            sigs[p] = sg
    want = [KC.item_status(ks, j, s) for j, s, _ in items]
    assert sigs.count(KC.G2_INF) == 5 and len(items) < EXACT_BELOW
    keys, _ = _keys(ctx, ks)
    kid = _load(ctx, ks)
    assert len(ks.B) == 2
    try:
        assert ctx.verify_signed_msgs(kid, signer, msgs, sigs).tolist() == want  # the exact route
        ctx.set_exact_below(0)
        assert ctx.verify_signed_msgs(kid, signer, msgs, sigs).tolist() == want  # grouped by signer
        # the composed calls, item by item (the stranger has no key to pass them)
        known = [p for p, j in enumerate(signer) if j < ks.N]
        H = ctx.hash_g2_batch([msgs[p] for p in known])
        ref = ctx.verify_sigs([keys[signer[p]] for p in known], H, [sigs[p] for p in known])
        assert ref.tolist() == [want[p] for p in known]
    finally:
        _defaults(ctx)
        ctx.keyset_free(kid)


# ------------------------------------------------------------------------ h: the generated key set
def test_generated_key_set(ctx):
    """hbtc_skg_generate from the commitment to the small set's f: the key bytes are the
    construction's (C0 00.. at 2 and 7), and the set it leaves loaded -- statuses, infinity flags
    and tables written by other kernels than hbtc_keyset_load's -- decides the share batch and
    coin instances i and iv as the construction says, like the set loaded from the bytes."""
    ks = KC.small()
    row, st = ctx.g1_mul(G1, list(ks.coeffs))
    assert not st.any()
    commit, _, pks, gen, status = ctx.skg_generate(ks.t - 1, bytes(row), None, ks.N, load_keyset=True)
    assert status == N.ACCEPT and gen is not None
    loaded = _load(ctx, ks)
    try:
        keys, mpk = _keys(ctx, ks)
        assert pks == keys and [pks[z] for z in ks.Z] == [KC.G1_INF] * 2 and commit[0] == mpk
        rd = Round(ctx, ks, KC.share_batch(ks, trio=5).values(), "generated")
        coin = Round(ctx, ks, KC.coin_small(ks).values(), "generated coin")
        assert coin.want_coin == [N.ACCEPT] * 2
        want_sig = coin.want_points(ctx, 2)
        for kid in (gen, loaded):
            _routes(ctx, lambda: ctx.verify_sig_shares(kid, rd.H, rd.counts, rd.idx, rd.sigs), rd.want)
            _routes(ctx, lambda: ctx.verify_dec_shares(kid, rd.H, rd.w, rd.counts, rd.idx, rd.shares), rd.want)
            _check_coin(ctx.coin_decide(kid, coin.H, coin.counts, coin.idx, coin.sigs, ks.t), coin, want_sig, kid)
    finally:
        ctx.keyset_free(gen)
        ctx.keyset_free(loaded)


# ---------------------------------------------------------------------------------------- i: node
def test_node(ctx, big):
    ks, kid, rd = big
    keys, _ = _keys(ctx, ks)
    node = N.Node([0, 0])
    try:
        nks, bad = node.keyset_load(keys)
        assert bad == 5
        for mode in (N.MODE_RLC, N.MODE_PER_SHARE):
            ctx.set_verify_mode(mode)
            node.set_verify_mode(mode)
            one = ctx.verify_sig_shares(kid, rd.H, rd.counts, rd.idx, rd.sigs).tolist()
            assert node.verify_sig_shares(nks, rd.H, rd.counts, rd.idx, rd.sigs).tolist() == one == rd.want, mode
            one = ctx.verify_dec_shares(kid, rd.H, rd.w, rd.counts, rd.idx, rd.shares).tolist()
            assert node.verify_dec_shares(nks, rd.H, rd.w, rd.counts, rd.idx, rd.shares).tolist() == one == rd.want, \
                mode
        node.keyset_free(nks)
    finally:
        _defaults(ctx)
        node.close()
