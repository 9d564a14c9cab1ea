"""One DynamicHoneyBadger-style key-generation era at N = 4, t = 1 through hbbft_amd/dhb.py on the
GPU: every node's Part (SyncKeyGen.new) and Ack (flush) is signed with hbtc_sign_shares, committed
in contributions with repeats across proposers, a stale message and one forged Ack signature, and
passed through commit_key_gen_messages (hbtc_verify_signed_msgs, the grouped path).  Exactly one
InvalidKeyGenMessageSignature is raised, on the proposer who included the forgery, and
generate_keys() gives the key set of the same era fed to skg.SyncKeyGen directly without that Ack."""
import random

import pytest

from hbbft_amd import _native as N
from hbbft_amd import dhb, skg
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu
R = B.R
G1 = B.g1_compress(B.G1_GEN)
N_NODES, T, START = 4, 1, 30


def _ser(kind, msg):
    """Stand-in for bincode(KeyGenMessage): the bytes that are signed."""
    if kind == "part":
        cts = msg.rows
        head = b"part" + b"".join(msg.commit)
    else:
        cts = msg.values
        head = b"ack" + msg.proposer.to_bytes(8, "little")
    return head + b"".join(bytes(c.u) + bytes(c.v) + bytes(c.w) for c in cts)


def test_key_generation_era_with_a_forged_ack():
    ctx = N.Context(0)
    try:
        ctx.set_exact_below(0)
        rng = random.Random(404)
        sks = [rng.randrange(1, R) for _ in range(N_NODES)]
        out, st = ctx.g1_mul(G1, sks)
        assert not st.any()
        pub_keys = {i: bytes(out[48 * i:48 * i + 48]) for i in range(N_NODES)}
        ks, bad = ctx.keyset_load([pub_keys[i] for i in range(N_NODES)])  # node order: entry = id
        assert bad == 0

        def signed(sender, kind, msg, epoch=START):
            ser = _ser(kind, msg)
            return dhb.SignedKeyGenMsg(epoch, sender, kind, msg, ser, ctx.sign_shares(sks[sender], [ser], want_H=False)[0][0])

        nodes, parts = [], []
        for i in range(N_NODES):
            kg, part = skg.SyncKeyGen.new(ctx, i, sks[i], pub_keys, T)
            nodes.append(kg)
            parts.append(signed(i, "part", part))
        ours = nodes[0]
        direct = skg.SyncKeyGen(ctx, 0, sks[0], pub_keys, T)  # the same era, fed without signatures

        # batch 1: every proposer commits its own Part and its neighbour's; one stale message whose
        # signature is never looked at
        stale = parts[1]._replace(epoch=START - 1, sig=parts[2].sig)
        contributions = [(p, [parts[p], parts[(p + 1) % N_NODES]]) for p in range(N_NODES)]
        contributions[0][1].insert(0, stale)
        assert dhb.commit_key_gen_messages(ctx, ks, START, contributions, ours) == []
        outs = ours.flush()
        assert len(outs) == 2 * N_NODES  # the stale message never reached the key generation
        acks = [(0, o[1]) for o in outs if o is not None]
        assert len(acks) == N_NODES and all(o is None or o[0] == "valid" for o in outs)
        for i in range(1, N_NODES):
            for p in parts:
                nodes[i].handle_part(p.sender, p.msg)
            node_outs = nodes[i].flush()
            assert all(o is not None and o[0] == "valid" for o in node_outs)
            acks += [(i, o[1]) for o in node_outs]
        sacks = [signed(i, "ack", a) for i, a in acks]

        # batch 2: every proposer commits its own Acks and its neighbour's; node 3's Ack of Part 2
        # appears only once, from proposer 2, under another Ack's signature (a subgroup point)
        victim = next(m for m in sacks if m.sender == 3 and m.msg.proposer == 2)
        forged = victim._replace(sig=next(m.sig for m in sacks if m.sender == 3 and m.msg.proposer == 1))
        contributions = []
        for p in range(N_NODES):
            mine = [m for m in sacks if m.sender in (p, (p + 1) % N_NODES) and m is not victim]
            if p == 2:
                mine.insert(len(mine) // 2, forged)
            contributions.append((p, mine))
        faults = dhb.commit_key_gen_messages(ctx, ks, START, contributions, ours)
        assert faults == [(2, "InvalidKeyGenMessageSignature")]
        ack_outs = ours.flush()
        # every Ack but the victim arrived twice: the second copy is the key generation's DuplicateAck
        assert sum(1 for f in ack_outs if f == []) == len(sacks) - 1
        assert all(f == [] or f[0][1] == ("AckMessage", "DuplicateAck") for f in ack_outs)

        for p in parts:
            direct.handle_part(p.sender, p.msg)
        assert all(o is not None and o[0] == "valid" for o in direct.flush())
        for m in sacks:
            if m is not victim:
                direct.handle_ack(m.sender, m.msg)
        assert all(f == [] for f in direct.flush())
        assert ours.is_ready() and direct.is_ready()
        commit_a, sk_a, pks_a, kid_a = ours.generate_keys()
        commit_b, sk_b, pks_b, kid_b = direct.generate_keys()
        assert (commit_a, sk_a, pks_a) == (commit_b, sk_b, pks_b)
        assert kid_a is not None and kid_b is not None and sk_a is not None
    finally:
        ctx.close()
