"""DynamicHoneyBadger's vote and key-gen-message rules restated sequentially -- TEST HELPER ONLY.

A line-by-line restatement of the two rule sets hbbft_amd/dhb.py replays in batches, verifying each
signature the moment the reference would, through an injected verify(signer_id, bytes, sig) ->
bool (as oracle/hbbft_rules.py does for the Coin and ThresholdDecryption):

  VoteCounter           src/dynamic_honey_badger/votes.rs:30-155
  key-gen transactions  src/dynamic_honey_badger/dynamic_honey_badger.rs:277-295, 425-440

Votes are dhb.SignedVote tuples (voter, change, era, num, ser, sig); key-gen messages are
dhb.SignedKeyGenMsg tuples (epoch, sender, kind, msg, ser, sig).  `validated` records every
(signer, bytes, sig) the rules verified, in order: what the reference would have validated.
"""


class VoteCounter:
    def __init__(self, era, num_faulty, verify):  # :35-42
        self.era = era
        self.num_faulty = num_faulty
        self.verify = verify
        self.pending = {}    # BTreeMap<N, SignedVote<N>>
        self.committed = {}  # BTreeMap<N, Vote<N>>
        self.validated = []

    def validate(self, sv):  # :150-155 (pk_opt == None is verify's business: false)
        self.validated.append((sv.voter, sv.ser, sv.sig))
        return self.verify(sv.voter, sv.ser, sv.sig)

    def add_pending_vote(self, sender_id, sv):  # :64-84
        have = self.pending.get(sv.voter)
        if sv.era != self.era or (have is not None and have.num >= sv.num):  # :69-73
            return []  # :74
        if not self.validate(sv):  # :76
            return [(sender_id, "InvalidVoteSignature")]  # :77-80
        self.pending[sv.voter] = sv  # :82
        return []

    def pending_votes(self):  # :88-94
        return [sv for voter, sv in sorted(self.pending.items())
                if self.committed.get(voter) is None or self.committed[voter].num < sv.num]

    def add_committed_votes(self, proposer_id, signed_votes):  # :97-110
        faults = []
        for sv in signed_votes:
            faults.extend(self.add_committed_vote(proposer_id, sv))
        return faults

    def add_committed_vote(self, proposer_id, sv):  # :113-133
        have = self.committed.get(sv.voter)
        if have is not None and have.num >= sv.num:  # :118-122
            return []  # :123
        if sv.era != self.era or not self.validate(sv):  # :125 (`||` short-circuits)
            return [(proposer_id, "InvalidCommittedVote")]  # :126-129
        self.committed[sv.voter] = sv  # :131
        return []

    def compute_winner(self):  # :136-147
        counts = {}
        for voter in sorted(self.committed):  # BTreeMap::values: by voter
            change = self.committed[voter].change
            counts[change] = counts.get(change, 0) + 1
            if counts[change] > self.num_faulty:  # :142
                return change
        return None


def process_key_gen_messages(start_epoch, contributions, verify, handle_part, handle_ack):
    """dynamic_honey_badger.rs:266-296, the key_gen_messages of every contribution; returns
    (faults, validated)."""
    faults, validated = [], []
    for proposer_id, key_gen_messages in contributions:  # :266
        for m in key_gen_messages:  # :277
            if m.epoch < start_epoch:  # :278
                continue  # :280
            validated.append((m.sender, m.ser, m.sig))
            if not verify(m.sender, m.ser, m.sig):  # :282
                faults.append((proposer_id, "InvalidKeyGenMessageSignature"))  # :287-288
                continue  # :289
            if m.kind == "part":  # :291-294
                handle_part(m.sender, m.msg)
            else:
                handle_ack(m.sender, m.msg)
    return faults, validated
