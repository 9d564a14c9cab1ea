"""The host rule of CoinEpoch(decide=True) (hbbft_amd/protocol.py): which t items one coin_decide
call selected, worked out from its item statuses, and when they are the items the deferred
combine would take -- so that the call's result may stand for the combine's.  Hand-made status
arrays and a stub context; no GPU.

The stub's coin_decide answers with parity 1 and its combine_sigs with parity 0, so a step's
output shows which path produced it: True = the call's result, False = the fallback combine.
"""
import numpy as np

from hbbft_amd import _native as N
from hbbft_amd import protocol as P

IDS = ["n%d" % i for i in range(7)]  # f = 2, t = 3
T = 3


def share(i, tag="ok"):
    return ("%s:%d" % (tag, i)).encode().ljust(96, b".")


class StubCtx:
    """coin_decide / combine_sigs / verify_sigs on labels: a share is ACCEPTed iff it starts with ok."""

    def __init__(self, master_ok=True):
        self.master_ok = master_ok
        self.calls = []

    def keyset_set_master(self, ks, mpk):
        self.calls.append(("set_master", ks, mpk))

    @staticmethod
    def _status(sigs):
        return np.array([N.ACCEPT if s.startswith(b"ok") else N.REJECT for s in sigs], np.int32)

    def verify_sig_shares(self, ks, H, counts, idx, sigs):
        self.calls.append(("verify_sig_shares", list(counts)))
        return self._status(sigs)

    def coin_decide(self, ks, H, counts, idx, sigs, t):
        self.calls.append(("coin_decide", list(counts)))
        st = self._status(sigs)
        cst, pos = [], 0
        for c in counts:
            acc = [idx[j] for j in range(pos, pos + c) if st[j] == N.ACCEPT][:t]
            if len(acc) < t:
                cst.append(N.NOT_ENOUGH_SHARES)
            elif len(set(acc)) < t:
                cst.append(N.DUPLICATE_ENTRY)
            else:
                cst.append(N.ACCEPT if self.master_ok else N.REJECT)
            pos += c
        n = len(counts)
        return st, [b"\x01" * 96] * n, np.ones(n, np.uint8), np.array(cst, np.int32)

    def combine_sigs(self, counts, idx, sigs, t):
        self.calls.append(("combine_sigs", list(counts)))
        n = len(counts)
        return [b"\x02" * 96] * n, np.zeros(n, np.uint8), np.full(n, N.ACCEPT, np.int32)

    def verify_sigs(self, pks, H, sigs):
        self.calls.append(("verify_sigs", len(sigs)))
        return np.full(len(sigs), N.ACCEPT if self.master_ok else N.REJECT, np.int32)


def epoch(ctx, our="n6", decide=True):
    ni = P.NetInfo(IDS, our, 1, master_pk=b"m" * 48)
    ep = P.CoinEpoch(ctx, ni, decide=decide)
    ep.add("k", b"H" * 96, share(IDS.index(our)))
    return ep


def feed(ep, events):
    for ev in events:
        if ev == "input":
            ep.handle_input("k")
        else:
            ep.handle_message("k", IDS[ev[0]], share(*ev))
    return ep.flush()["k"]


def outputs(steps):
    return [s["output"] for s in steps if s["output"] is not None]


def test_selection_from_statuses():
    idx = [4, 2, 9, 2, 0, 5, 1]
    sigs = [share(i) for i in idx]
    st = [N.ACCEPT, N.REJECT, N.DECODE_ERR, N.ACCEPT, N.ACCEPT, N.ACCEPT, N.ACCEPT]
    sel = P.coin_call_selection([5, 2], idx, sigs, st, 3)
    # instance 0: positions 0, 3, 4 (the rejected and the undecodable item are skipped)
    assert sel[0] == frozenset({(4, share(4)), (2, share(2)), (0, share(0))})
    assert sel[1] is None  # two ACCEPTed items only
    sel = P.coin_call_selection([7], idx, sigs, st, 3)
    assert sel[0] == frozenset({(4, share(4)), (2, share(2)), (0, share(0))})  # the FIRST t, not all


def test_serves_rule():
    sel = frozenset({(4, share(4)), (2, share(2)), (0, share(0))})
    items = [(0, share(0)), (2, share(2)), (4, share(4))]
    assert P.coin_call_serves(sel, items, 3)
    assert P.coin_call_serves(sel, items + [(5, share(5))], 3)  # the combine takes the first t only
    assert not P.coin_call_serves(sel, [(0, share(0)), (1, share(1))] + items[1:], 3)
    assert not P.coin_call_serves(sel, [(0, share(0)), (2, share(2, "ok2")), (4, share(4))], 3)  # other bytes
    assert not P.coin_call_serves(None, items, 3)
    assert not P.coin_call_serves(sel, items[:2], 3)
    dup = frozenset({(4, share(4)), (2, share(2))})  # a repeated (sender, share) collapsed: < t distinct
    assert not P.coin_call_serves(dup, items, 3)


def test_in_order_uses_the_call():
    ctx = StubCtx()
    ep = epoch(ctx)
    steps = feed(ep, ["input", (0,), (1,), (2,)])
    assert outputs(steps) == [True]
    assert (ep.decided, ep.fallback) == (1, 0)
    assert [c[0] for c in ctx.calls] == ["set_master", "coin_decide"]


def test_default_is_unchanged():
    ctx = StubCtx()
    ep = epoch(ctx, decide=False)
    steps = feed(ep, ["input", (0,), (1,), (2,)])
    assert outputs(steps) == [False]
    assert (ep.decided, ep.fallback) == (0, 0)
    assert [c[0] for c in ctx.calls] == ["verify_sig_shares", "combine_sigs", "verify_sigs"]


def test_no_master_key_keeps_the_default():
    ctx = StubCtx()
    ep = P.CoinEpoch(ctx, P.NetInfo(IDS, "n6", 1), decide=True)
    assert not ep.decide and ctx.calls == []


def test_rejected_share_among_the_first_t():
    ctx = StubCtx()
    ep = epoch(ctx)
    steps = feed(ep, ["input", (0,), (1, "bad"), (2,), (3,)])
    # the call skips the rejected share and selects own (6), 0, 2 -- what the replay holds at (2,)
    assert steps[2]["faults"] == [("n1", "UnverifiedSignatureShareSender")]
    assert outputs(steps) == [True] and steps[3]["output"] is True
    assert (ep.decided, ep.fallback) == (1, 0)


def test_late_input_falls_back():
    ctx = StubCtx()
    ep = epoch(ctx)
    # t + 2 shares in descending order, then the input: the combine takes the three LOWEST node
    # indices of the six it holds (1, 2, 3), the call selected the first three to arrive (5, 4, 3)
    steps = feed(ep, [(5,), (4,), (3,), (2,), (1,), "input"])
    assert outputs(steps) == [False]
    assert (ep.decided, ep.fallback) == (0, 1)
    assert [c[0] for c in ctx.calls] == ["set_master", "coin_decide", "combine_sigs", "verify_sigs"]


def test_late_input_with_the_same_items_uses_the_call():
    ctx = StubCtx()
    ep = epoch(ctx)
    # the rule compares items, not event kinds: arrivals 0, 1, 2, 3 then the input (own = 6) --
    # the first three to arrive are also the three lowest indices held
    steps = feed(ep, [(0,), (1,), (2,), (3,), "input"])
    assert outputs(steps) == [True]
    assert (ep.decided, ep.fallback) == (1, 0)


def test_duplicate_sender_falls_back():
    ctx = StubCtx()
    ep = epoch(ctx)
    # n0 repeats its share: the call's first three ACCEPTed items are own, n0, n0 (DUPLICATE_ENTRY
    # there), the queue holds own, n0, n1 when it reaches its threshold
    steps = feed(ep, ["input", (0,), (0,), (1,)])
    assert outputs(steps) == [False]
    assert (ep.decided, ep.fallback) == (0, 1)


def test_carried_state_falls_back():
    ctx = StubCtx()
    ep = epoch(ctx)
    assert outputs(feed(ep, ["input", (4,)])) == []
    assert (ep.decided, ep.fallback) == (0, 0)
    # the second flush's call sees (1,), (2,), (3,) only and selects them; the queue reaches its
    # threshold at (1,) already, holding own, 4 and 1 -- not the call's selection
    steps = feed(ep, [(1,), (2,), (3,)])
    assert outputs(steps) == [False] and steps[0]["output"] is False
    assert (ep.decided, ep.fallback) == (0, 1)


def test_wrong_master_is_verification_failed():
    ctx = StubCtx(master_ok=False)
    ep = epoch(ctx)
    steps = feed(ep, ["input", (0,), (1,), (2,)])
    # REJECT from the call, then the synchronous replay of the instance: every share past the
    # threshold retries the combine and fails the master check (coin.rs:163-181, :192-197)
    assert [s["error"] for s in steps] == [None, None, "VerificationFailed", "VerificationFailed"]
    assert outputs(steps) == []
    assert (ep.decided, ep.fallback) == (1, 0)
