"""hbbft_amd/dhb.py's queue -> one batched call -> replay against tests/dhb_rules.py's sequential
restatement of the reference, over random event streams at N = 4..7 with a fake context whose
verdicts are a lookup table (no GPU).  The streams hold obsolete, duplicate and wrong-era votes,
revotes with a higher `num`, bad signatures before and after an obsoleting vote, votes of nodes
without a key, stale-epoch key-gen messages and duplicates across contributions."""
import random

import numpy as np
import pytest

import dhb_rules
from hbbft_amd import _native as N
from hbbft_amd import dhb

ERA = 40


def _sig(rng):
    return bytes(rng.randrange(256) for _ in range(96))


class FakeContext:
    """verify_signed_msgs from a table {(signer index, bytes, sig): status}; a signer past the key
    set is UNKNOWN_SENDER, an unlisted triple REJECT.  Every call and its triples are recorded."""

    def __init__(self, n_keys, table):
        self.n_keys = n_keys
        self.table = table
        self.calls = []

    def verify_signed_msgs(self, keyset_id, signer, msgs, sigs):
        assert keyset_id == 7
        triples = list(zip([int(s) for s in signer], [bytes(m) for m in msgs], [bytes(s) for s in sigs]))
        assert len(set(triples)) == len(triples), "the call repeats a (signer, bytes, sig) triple"
        self.calls.append(triples)
        return np.array([N.UNKNOWN_SENDER if s >= self.n_keys else self.table.get((s, m, g), N.REJECT)
                         for s, m, g in triples], np.int32)


class World:
    """n validators 0..n-1 (key-set entry = id), a candidate n (entry n) and a stranger n + 1
    without a key; valid signatures are whatever the table lists as ACCEPT."""

    def __init__(self, rng, n):
        self.rng = rng
        self.n = n
        self.index = {i: i for i in range(n + 1)}
        self.table = {}
        self.ctx = FakeContext(n + 1, self.table)

    def verify(self, signer_id, ser, sig):  # the reference's pk_opt.map_or(false, |pk| pk.verify(..))
        idx = self.index.get(signer_id)
        return idx is not None and self.table.get((idx, bytes(ser), bytes(sig)), N.REJECT) == N.ACCEPT

    def sign(self, signer_id, ser, good=True):
        sig = _sig(self.rng)
        idx = self.index.get(signer_id)
        if idx is not None:
            # a bad signature is a well-formed point that fails (REJECT) or one that does not decode
            self.table[(idx, ser, sig)] = N.ACCEPT if good else self.rng.choice([N.REJECT, N.DECODE_ERR])
        return sig

    def vote(self, voter, change, era, num, good=True):
        ser = b"vote|%r|%r|%d|%d" % (voter, change, era, num)
        return dhb.SignedVote(voter, change, era, num, ser, self.sign(voter, ser, good))


def _vote_stream(w, n_events):
    """(kind, who, votes): pending votes from random senders and committed contributions."""
    rng, n = w.rng, w.n
    changes = [("add", n), ("remove", 0), ("remove", 1)]
    nums = {}
    made = []
    events = []
    for _ in range(n_events):
        def fresh():
            voter = rng.choice(list(range(n)) + [n + 1])  # the stranger has no key
            roll = rng.random()
            if roll < 0.15 and made:
                return rng.choice(made)                        # a duplicate
            era = ERA if roll > 0.3 else rng.choice([ERA - 1, ERA + 1])  # wrong era
            if roll > 0.7:
                num = nums.get(voter, -1) + 1                  # a revote with a higher num
            else:
                num = rng.randrange(0, nums.get(voter, 0) + 2)  # maybe obsolete
            nums[voter] = max(nums.get(voter, 0), num)
            sv = w.vote(voter, rng.choice(changes), era, num, good=rng.random() > 0.3)
            made.append(sv)
            return sv
        if rng.random() < 0.5:
            events.append(("pending", [(rng.randrange(n), fresh()) for _ in range(rng.randrange(1, 5))]))
        else:
            events.append(("committed", [(p, [fresh() for _ in range(rng.randrange(0, 4))])
                                         for p in rng.sample(range(n), rng.randrange(1, n + 1))]))
    return events


@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_vote_counter_replay_matches_the_sequential_rules(n, seed):
    rng = random.Random(1000 * n + seed)
    w = World(rng, n)
    f = (n - 1) // 3
    ours = dhb.VoteCounter(w.ctx, 7, {i: i for i in range(n)}, ERA, f)
    ref = dhb_rules.VoteCounter(ERA, f, lambda voter, ser, sig: voter < n and w.verify(voter, ser, sig))
    raised = {"InvalidVoteSignature": 0, "InvalidCommittedVote": 0}
    for kind, payload in _vote_stream(w, 60):
        if kind == "pending":
            got = ours.add_pending_votes(payload)
            want = [flt for sender, sv in payload for flt in ref.add_pending_vote(sender, sv)]
        else:
            got = ours.add_committed_votes(payload)
            want = [flt for p, votes in payload for flt in ref.add_committed_votes(p, votes)]
        assert got == want
        for _, k in got:
            raised[k] += 1
        assert ours.pending == ref.pending and ours.committed == ref.committed
        assert ours.pending_votes() == ref.pending_votes()
        assert ours.compute_winner() == ref.compute_winner()
    assert min(raised.values()) > 0  # the streams do reach both faults
    # every triple the reference validated was judged by a batched call, and in far fewer calls
    judged = {t for call in w.ctx.calls for t in call}
    for voter, ser, sig in ref.validated:
        assert (voter if voter < n else dhb.NO_KEY, ser, sig) in judged
    assert len(w.ctx.calls) <= 60 < len(ref.validated)


def test_single_pending_vote_and_a_bad_signature_behind_an_obsoleting_vote():
    w = World(random.Random(9), 4)
    vc = dhb.VoteCounter(w.ctx, 7, {i: i for i in range(4)}, ERA, 1)
    good = w.vote(2, ("remove", 0), ERA, 3)
    forged_old = w.vote(2, ("remove", 1), ERA, 1, good=False)
    forged_new = w.vote(2, ("remove", 1), ERA, 4, good=False)
    assert vc.add_pending_vote(0, forged_old) == [(0, "InvalidVoteSignature")]  # before: validated
    assert vc.add_pending_vote(1, good) == []
    assert vc.add_pending_vote(0, forged_old) == []       # behind num 3: obsolete, never validated
    assert vc.add_pending_vote(3, forged_new) == [(3, "InvalidVoteSignature")]
    assert vc.pending == {2: good}
    assert vc.add_committed_votes([(1, [forged_old]), (3, [good, good])]) == [(1, "InvalidCommittedVote")]
    assert vc.add_committed_votes([(0, [forged_old])]) == []   # obsolete now: no fault
    assert vc.compute_winner() is None and vc.pending_votes() == []
    other = w.vote(3, ("remove", 0), ERA, 0)
    assert vc.add_committed_votes([(2, [other])]) == []
    assert vc.compute_winner() == ("remove", 0)


def test_a_malformed_signature_never_reaches_the_call():
    w = World(random.Random(10), 4)
    assert dhb.verify_signed(w.ctx, 7, [(0, b"m", b"short"), (None, b"m", b"")]) == [False, False]
    assert w.ctx.calls == []


class FakeKeyGen:
    def __init__(self, index):
        self.index = index
        self.handled = []

    def handle_part(self, sender, part):
        self.handled.append(("part", sender, part))

    def handle_ack(self, sender, ack):
        self.handled.append(("ack", sender, ack))


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_key_gen_messages_replay_matches_the_sequential_rules(n):
    rng = random.Random(50 + n)
    w = World(rng, n)
    start_epoch = 12
    pool = []
    for k in range(3 * n):
        sender = rng.choice(list(range(n + 1)) + [n + 1])  # validators, the candidate, a stranger
        kind = rng.choice(["part", "ack"])
        ser = b"kg|%d|%s|%d" % (sender, kind.encode(), k)
        epoch = start_epoch if rng.random() > 0.25 else start_epoch - 1 - rng.randrange(3)  # stale
        pool.append(dhb.SignedKeyGenMsg(epoch, sender, kind, ("payload", k), ser,
                                        w.sign(sender, ser, good=rng.random() > 0.25)))
    # the same signed message in many proposers' contributions
    contributions = [(p, [rng.choice(pool) for _ in range(rng.randrange(0, 2 * n))]) for p in range(n)]
    ref_handled = []
    want, validated = dhb_rules.process_key_gen_messages(
        start_epoch, contributions, w.verify,
        lambda s, m: ref_handled.append(("part", s, m)), lambda s, m: ref_handled.append(("ack", s, m)))
    kg = FakeKeyGen(w.index)
    got = dhb.commit_key_gen_messages(w.ctx, 7, start_epoch, contributions, kg)
    assert got == want and kg.handled == ref_handled
    assert any(k == "InvalidKeyGenMessageSignature" for _, k in got) and kg.handled
    assert len(w.ctx.calls) == 1
    # one call over the distinct triples the reference validated: stale messages are not in it
    assert set(w.ctx.calls[0]) == {(w.index.get(s, dhb.NO_KEY), m, g) for s, m, g in validated}
    assert len(w.ctx.calls[0]) < len(validated)
