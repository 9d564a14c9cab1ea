"""Per-sender RLC scalars of the DecryptionShare path (hbtc_rlc.hip): the scalar of a share is a
function of (call key, sender id), so [r_id] pk_id is computed once per call into a sender table
(tail workgroups of k_rlc_decode) and k_rlc_items loads it.  Two entries of one sender inside one
tile would share a scalar; the duplicate guard sends every later copy to the exact leaf checks.
Decisions must equal the construction's and the per-share mode's under every check schedule, at
128- and 64-bit scalars.
Reference: threshold_crypto's PublicKeyShare::verify_decryption_share, once per share."""
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from tests.test_gpu_parity import R, _keyset, b, load

pytestmark = pytest.mark.gpu

N_KEYS = 70
BAD_KEY = 21  # the sender whose key fails to load in the second key set
SCHEDULES = (N.CHECK_AUTO, N.CHECK_PLAIN_FIRST, N.CHECK_PAIR_SUBS, N.CHECK_PAIR_LEAVES)


def _senders(rng, count, exclude=()):
    """`count` distinct senders, none of `exclude`."""
    return rng.sample([s for s in range(N_KEYS) if s not in exclude], count)


class Batch:
    """Instances appended one by one: sender list, per-position scalar offsets (a wrong share is
    sk r + delta), positions whose encoding is broken, and the expected statuses."""

    def __init__(self, rng, sks):
        self.rng, self.sks = rng, sks
        self.counts, self.idx, self.scal, self.exp, self.broken, self.rh = [], [], [], [], [], []
        self.first = {}

    def add(self, name, senders, delta=None, broken=(), expect=None):
        delta, expect = delta or {}, expect or {}
        r, h = self.rng.randrange(1, R), self.rng.randrange(1, R)
        base = len(self.idx)
        self.first[name] = base
        self.rh.append((r, h))
        self.counts.append(len(senders))
        for j, s in enumerate(senders):
            self.idx.append(s)
            sk = self.sks[s] if s < N_KEYS else 1
            self.scal.append((sk * r + delta.get(j, 0)) % R)
            self.exp.append(expect.get(j, N.REJECT if j in delta else N.ACCEPT))
        self.broken += [base + j for j in broken]

    def build(self, ctx):
        codec = load("codec.json")
        g1, g2 = b(codec["g1_generator"]), b(codec["g2_generator"])
        H, _ = ctx.g2_mul(g2, [h for _, h in self.rh])
        w, _ = ctx.g2_mul(g2, [r * h % R for r, h in self.rh])
        shares, st = ctx.g1_mul(g1, self.scal)
        assert not st.any()
        shares = shares.reshape(len(self.scal), 48).copy()
        for p in self.broken:
            shares[p, 0] &= 0x7F  # no compression flag: an invalid encoding
        return H, w, self.counts, self.idx, shares.reshape(-1), np.asarray(self.exp, np.int32)


@pytest.fixture(scope="module")
def env():
    ctx = N.Context(0)
    ctx.set_exact_below(0)
    ctx.set_sender_tracking(False)
    rng = random.Random(707)
    f, coeffs, sks, pk = _keyset(ctx, rng, N_KEYS)
    ks, bad = ctx.keyset_load(pk)
    assert bad == 0
    yield ctx, rng, sks, pk, ks
    ctx.set_rlc_bits(128)
    ctx.close()


def _dup_instance(rng):
    """Instance C: 64 valid entries, sender 7 at positions 3 and 12, sender 9 at 20, 21 and 22."""
    senders = _senders(rng, 64, exclude=(7, 9))
    for p in (3, 12):
        senders[p] = 7
    for p in (20, 21, 22):
        senders[p] = 9
    return senders


def _run_all(ctx, ks, args, exp):
    """Per-share mode, then the RLC mode at both scalar widths under every check schedule."""
    ctx.set_verify_mode(N.MODE_PER_SHARE)
    st_ref = ctx.verify_dec_shares(ks, *args)
    assert (st_ref == exp).all(), ("per-share", np.nonzero(st_ref != exp))
    ctx.set_verify_mode(N.MODE_RLC)
    try:
        for bits in (128, 64):
            ctx.set_rlc_bits(bits)
            for sched in SCHEDULES:
                ctx.set_check_schedule(sched)
                st = ctx.verify_dec_shares(ks, *args)
                assert (st == exp).all(), (bits, sched, np.nonzero(st != exp)[0], st[st != exp])
    finally:
        ctx.set_rlc_bits(128)
        ctx.set_check_schedule(N.CHECK_AUTO)


def test_sender_scalars_equal_per_share_decisions(env):
    """One call holding every instance.

    A  70 shares in node order (a full tile and a ragged one of 6), position 65 wrong.
    B  two instances with the same permuted sender list, one wrong share in the second only:
       the call's sender table must not mix ciphertexts.
    C  duplicates of valid shares inside one tile: all ACCEPT.
    D  sender 11 at positions 5 and 40 of one tile with shares sk r + delta and sk r - delta.
       Both copies carry the sender's one scalar, so inside the group sums the two errors cancel
       and BOTH SHARES WOULD BE ACCEPTED WRONGLY IF THE DUPLICATE GUARD WERE MISSING; with it the
       later copy is checked exactly and the first alone fails its tile.  Both REJECT.
    E  the same cancelling pair at positions 10 and 100 of a 130-share instance: different
       tiles, different checks, no guard needed.  Both REJECT.
    F  a duplicate whose first copy has an invalid encoding (DECODE_ERR; the second copy is then
       the first to enter the sums: ACCEPT) and an unknown sender id (UNKNOWN_SENDER)."""
    ctx, rng, sks, pk, ks = env
    bt = Batch(rng, sks)
    bt.add("A", list(range(N_KEYS)), delta={65: rng.randrange(1, 1 << 40)})
    perm = _senders(rng, 64)
    bt.add("B1", perm)
    bt.add("B2", perm, delta={17: rng.randrange(1, R)})
    bt.add("C", _dup_instance(rng))
    d = rng.randrange(1, R)
    sd = _senders(rng, 64, exclude=(11,))
    sd[5] = sd[40] = 11
    bt.add("D", sd, delta={5: d, 40: R - d})
    se = _senders(rng, 64, exclude=(11,)) + _senders(rng, 64, exclude=(11,)) + _senders(rng, 2)
    se[10] = se[100] = 11
    bt.add("E", se, delta={10: d, 100: R - d})
    sf = _senders(rng, 64, exclude=(13,))
    sf[8] = sf[30] = 13
    sf[50] = N_KEYS + 2
    bt.add("F", sf, broken=(8,), expect={8: N.DECODE_ERR, 50: N.UNKNOWN_SENDER})
    H, w, counts, idx, shares, exp = bt.build(ctx)
    assert counts == [70, 64, 64, 64, 64, 130, 64]
    assert int((exp == N.REJECT).sum()) == 6
    _run_all(ctx, ks, (H, w, counts, idx, shares), exp)


def test_only_later_copies_take_the_exact_path(env):
    """Instance C as a call of its own: of the five entries of senders 7 and 9 the three later
    copies, and nothing else, reach the exact leaf checks."""
    ctx, rng, sks, pk, ks = env
    bt = Batch(rng, sks)
    bt.add("C", _dup_instance(rng))
    H, w, counts, idx, shares, exp = bt.build(ctx)
    ctx.set_verify_mode(N.MODE_RLC)
    try:
        for bits in (128, 64):
            ctx.set_rlc_bits(bits)
            st = ctx.verify_dec_shares(ks, H, w, counts, idx, shares)
            assert (st == N.ACCEPT).all(), (bits, st)
            assert ctx.rlc_last_leaves() == 3, (bits, ctx.rlc_last_leaves())
    finally:
        ctx.set_rlc_bits(128)


def test_sender_whose_key_failed_to_load(env):
    """A key set with one bad key encoding: every share of that sender is DECODE_ERR at every
    position (twice in one tile, once in the ragged tile); its sender-table entry is the
    identity and its fixed-base table rows are never read."""
    ctx, rng, sks, pk, ks = env
    pk2 = np.array(pk, dtype=np.uint8).reshape(N_KEYS, 48).copy()
    pk2[BAD_KEY, 0] &= 0x7F
    ks2, bad = ctx.keyset_load(pk2.reshape(-1))
    assert bad == 1
    try:
        senders = _senders(rng, 64, exclude=(BAD_KEY,)) + _senders(rng, 6, exclude=(BAD_KEY,))
        where = (2, 33, 66)
        for p in where:
            senders[p] = BAD_KEY
        bt = Batch(rng, sks)
        bt.add("F3", senders, delta={40: rng.randrange(1, R)},
               expect={p: N.DECODE_ERR for p in where})
        H, w, counts, idx, shares, exp = bt.build(ctx)
        _run_all(ctx, ks2, (H, w, counts, idx, shares), exp)
    finally:
        ctx.keyset_free(ks2)
