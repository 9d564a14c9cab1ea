"""DynamicHoneyBadger's signed votes and signed key-generation messages — the host-side mirror of
the reference's rules around its non-threshold ``PublicKey::verify(sig, bytes)`` calls, driving
hbtc_verify_signed_msgs:

  * VoteCounter (src/dynamic_honey_badger/votes.rs:30-155): ``validate`` (:150-155) runs for every
    pending vote received (:64-84) and every committed vote of every contribution (:97-133);
  * DynamicHoneyBadger::verify_signature (dynamic_honey_badger.rs:425-440): on receipt of a key-gen
    message (:216) and again for every SignedKeyGenMsg of every contribution of every committed
    batch (:277-295).

The reference verifies one signature at a time, in the middle of its state changes.  A verdict
depends only on (signer, bytes, signature), never on state, so here — as in protocol.py and
skg.py — the messages of a batch queue up, ONE call judges every distinct triple (the same signed
message sits in the contributions of many proposers: ``verify_signed`` dedups), and the
reference's state rules are then replayed in order with those verdicts.  A fault is raised only
for a message the reference would have validated: an obsolete vote or a stale key-gen message is
skipped before its verdict is looked at, exactly where the reference skips it before validating.

The signers are entries of a loaded key set: the validators' individual public keys in node
order, a joining candidate's key appended (candidate_key, dynamic_honey_badger.rs:433-438); a
node without an entry (``public_key(id) == None``) verifies as false.  The bincode of ``Vote<N>``
and ``KeyGenMessage`` depends on the caller's node-id type, so messages carry their serialized
bytes.  Out of scope: the HoneyBadger restart, the candidate message cap (:232-245).
"""
from collections import namedtuple

from . import _native as N

NO_KEY = 0xFFFFFFFF  # a signer without a key-set entry: HBTC_UNKNOWN_SENDER, i.e. false

# votes.rs:158-175: Vote { change, era, num } signed by `voter`; ser = bincode(Vote), the signed bytes
SignedVote = namedtuple("SignedVote", "voter change era num ser sig")
# dynamic_honey_badger/mod.rs SignedKeyGenMsg(epoch, sender, KeyGenMessage, sig): kind "part" | "ack",
# msg the skg.Part / skg.Ack, ser = bincode(KeyGenMessage), the signed bytes
SignedKeyGenMsg = namedtuple("SignedKeyGenMsg", "epoch sender kind msg ser sig")


def verify_signed(ctx, keyset_id, items):
    """PublicKey::verify for every (key-set index or None, bytes, signature) of `items`: one
    hbtc_verify_signed_msgs call over the distinct triples, one bool per input item.  A signature
    that is not 96 bytes never reaches the call (serde would have refused the message)."""
    slot, uniq, out = {}, [], []
    for who, msg, sig in items:
        key = (NO_KEY if who is None else int(who), bytes(msg), bytes(sig))
        if len(key[2]) != 96:
            out.append(None)
            continue
        if key not in slot:
            slot[key] = len(uniq)
            uniq.append(key)
        out.append(slot[key])
    if not uniq:
        return [False] * len(out)
    st = ctx.verify_signed_msgs(keyset_id, [k[0] for k in uniq], [k[1] for k in uniq], [k[2] for k in uniq])
    return [s is not None and int(st[s]) == N.ACCEPT for s in out]


class VoteCounter:
    """votes.rs:18-147 with batched validation.  `index` maps a node id to its key-set entry
    (NetworkInfo::public_key); ids must be sortable (the reference keeps BTreeMaps)."""

    def __init__(self, ctx, keyset_id, index, era, num_faulty):
        self.ctx = ctx
        self.keyset_id = keyset_id
        self.index = dict(index)
        self.era = era
        self.num_faulty = num_faulty
        self.pending = {}    # voter -> SignedVote
        self.committed = {}  # voter -> SignedVote (the reference keeps its Vote)

    def _verdicts(self, votes):
        ok = verify_signed(self.ctx, self.keyset_id,
                           [(self.index.get(v.voter), v.ser, v.sig) for v in votes])
        return dict(zip([id(v) for v in votes], ok))

    def add_pending_votes(self, received):
        """add_pending_vote (:64-84) for every (sender_id, SignedVote) in order; the faults
        [(sender_id, "InvalidVoteSignature")].  A vote of another era is never validated; the
        `num` rule is replayed in order, after the one call."""
        received = list(received)
        ok = self._verdicts([sv for _, sv in received if sv.era == self.era])
        faults = []
        for sender, sv in received:
            have = self.pending.get(sv.voter)
            if sv.era != self.era or (have is not None and have.num >= sv.num):
                continue  # obsolete or already there
            if not ok[id(sv)]:
                faults.append((sender, "InvalidVoteSignature"))
                continue
            self.pending[sv.voter] = sv
        return faults

    def add_pending_vote(self, sender_id, signed_vote):
        return self.add_pending_votes([(sender_id, signed_vote)])

    def pending_votes(self):
        """:88-94: the pending votes newer than their voter's committed vote, by voter."""
        return [sv for voter, sv in sorted(self.pending.items())
                if voter not in self.committed or self.committed[voter].num < sv.num]

    def add_committed_votes(self, contributions):
        """add_committed_votes (:97-133) over all contributions [(proposer_id, [SignedVote])] of a
        batch, in order; the faults [(proposer_id, "InvalidCommittedVote")].  A wrong-era vote is a
        fault without a verification (the `||` at :125)."""
        contributions = [(p, list(votes)) for p, votes in contributions]
        ok = self._verdicts([sv for _, votes in contributions for sv in votes if sv.era == self.era])
        faults = []
        for proposer, votes in contributions:
            for sv in votes:
                have = self.committed.get(sv.voter)
                if have is not None and have.num >= sv.num:
                    continue  # obsolete or already there
                if sv.era != self.era or not ok[id(sv)]:
                    faults.append((proposer, "InvalidCommittedVote"))
                    continue
                self.committed[sv.voter] = sv
        return faults

    def compute_winner(self):
        """:136-147: the first change, by voter order, with more than num_faulty votes."""
        counts = {}
        for _, sv in sorted(self.committed.items()):
            counts[sv.change] = counts.get(sv.change, 0) + 1
            if counts[sv.change] > self.num_faulty:
                return sv.change
        return None


def commit_key_gen_messages(ctx, keyset_id, start_epoch, contributions, key_gen, index=None):
    """The key-gen half of process_output (dynamic_honey_badger.rs:277-295) for the contributions
    [(proposer_id, [SignedKeyGenMsg])] of a committed batch.  In contribution order, then message
    order: a message with epoch < start_epoch is skipped; a bad signature is
    InvalidKeyGenMessageSignature for the PROPOSER of the contribution, and the message is dropped;
    every other message goes to key_gen.handle_part / handle_ack (skg.SyncKeyGen, whose flush then
    runs the era's checks).  `index` maps a node id to its key-set entry (default: key_gen's node
    order, for a key set loaded in that order).  Returns the faults."""
    index = key_gen.index if index is None else index
    contributions = [(p, list(msgs)) for p, msgs in contributions]
    live = [m for _, msgs in contributions for m in msgs if m.epoch >= start_epoch]
    ok = dict(zip([id(m) for m in live],
                  verify_signed(ctx, keyset_id, [(index.get(m.sender), m.ser, m.sig) for m in live])))
    faults = []
    for proposer, msgs in contributions:
        for m in msgs:
            if m.epoch < start_epoch:
                continue  # obsolete key generation message
            if not ok[id(m)]:
                faults.append((proposer, "InvalidKeyGenMessageSignature"))
                continue
            if m.kind == "part":
                key_gen.handle_part(m.sender, m.msg)
            else:
                key_gen.handle_ack(m.sender, m.msg)
    return faults
