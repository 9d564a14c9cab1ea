"""SyncKeyGen batch queue — the host-side mirror of the reference's dealerless key generation
(/root/reference/src/sync_key_gen.rs:272-509) driving the GPU verifier.

The reference handles every Part / Ack synchronously: decrypt our row (our value), bincode-decode
it, check it against the proposer's bivariate commitment — one BivarCommitment::row (Part) or
BivarCommitment::evaluate (Ack) per message, G1-MSM heavy.  Here messages queue in arrival order;
``flush`` then
  1. decrypts every queued ciphertext addressed to us in one batch (SecretKey::decrypt:
     Ciphertext::verify + sk u + the hash_bytes pad; hbtc_decrypt),
  2. checks every decoded row in one hbtc_skg_check_parts call and every decoded value in one
     hbtc_skg_check_acks call (the value check of an Ack uses the commitment of the FIRST Part
     received from its proposer, the only one the reference ever stores, :346-354),
  3. replays the queue in order with those verdicts, so every state change and fault is the
     reference's: parts are stored before their row is checked (:346-354), an Ack is recorded in
     ``acks`` before its value is checked (:474-476), and the fault order is NodeCount ->
     SenderExist -> DuplicateAck -> ValueDecryption -> ValueDeserialization -> ValueInvalid
     (:467-495); a Part whose row fails to decrypt yields no outcome (the `?` at :358), one whose
     row does not decode or match yields InvalidPartMessage (:359-370),
  4. encrypts the Ack values of every valid Part in one batch (:372-380).
Verdicts depend only on the message and the stored commitment, never on later state, so the
replay reproduces the sequential outcomes exactly (tests/test_gpu_skg_protocol.py checks this
against oracle/hbbft_rules.py's line-by-line restatement).

Keys: ``generate`` (:428-447) sums row(0) of the complete Parts' commitments and interpolates our
secret share on the device (hbtc_skg_generate); ``generate_keys`` also evaluates every node's
public key share and leaves them loaded as the new era's key set (NetworkInfo::new,
src/messaging.rs:253-256) in the same call; ``public_key_shares`` is Commitment::evaluate(i + 1)
for every node of a given commitment (hbtc_commitment_evaluate).
Producing: ``SyncKeyGen.new`` and ``_emit_acks`` compose g1_mul, hbtc_fr_poly_eval, the numpy
framing and hbtc_encrypt; with ``one_call=True`` they are one hbtc_skg_part / hbtc_skg_acks call
each, the recipients a key set loaded once per instance (same bytes for the same scalars).
Values on the wire use hbbft_amd/wire.py's bincode framing (parity-unpinned Fr layout).
"""
import secrets
from collections import namedtuple

import numpy as np

from . import _native as N
from . import wire

R = wire.R
G1_GEN = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
G1_INF = bytes([0xC0]) + bytes(47)

Ciphertext = namedtuple("Ciphertext", "u v w")   # threshold_crypto Ciphertext(U, V, W)
Part = namedtuple("Part", "commit rows")         # sync_key_gen.rs:201: (BivarCommitment, rows)
Ack = namedtuple("Ack", "proposer values")       # sync_key_gen.rs:218: (proposer index, values)


def coeff_pos(i, j):
    """Index of coefficient (i, j) of a symmetric bivariate polynomial (packed upper triangle)."""
    return j * (j + 1) // 2 + i if j >= i else i * (i + 1) // 2 + j


def _fr_le(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).copy()


# ------------------------------------------------------------------------------ encryption
def encrypt_batch(ctx, pks, msgs, rs=None):
    """PublicKey::encrypt_with_rng for n (pk_i, msg_i): u = r G1, v = msg XOR hash_bytes(r pk),
    w = r hash_g1_g2(u, v), in one hbtc_encrypt call (device-resident between its stages)."""
    n = len(msgs)
    if n == 0:
        return []
    rs = rs or [secrets.randbelow(R - 1) + 1 for _ in range(n)]
    cts, st = ctx.encrypt([bytes(p) for p in pks], rs, msgs)
    if st.any():
        raise N.HbtcError("encrypt: a public key failed to decode")
    return [Ciphertext(u, v, w) for u, v, w in cts]


def bivar_rows(ctx, b, t, n):
    """The wire-framed rows 1..n of the symmetric bivariate polynomial b (packed, coeff_pos
    order): row_x coefficient k = poly_k(x) with poly_k = b[k, .], one hbtc_fr_poly_eval call
    (_bivar_row is the Python-integer form of one row)."""
    polys = [[b[coeff_pos(k, j)] for j in range(t + 1)] for k in range(t + 1)]
    out = ctx.fr_poly_eval(polys, list(range(1, n + 1)))  # [k, x, 32]
    return wire.polys_to_wire(np.ascontiguousarray(out.transpose(1, 0, 2)))


def ack_values(ctx, rows, n):
    """Per verified row the wire-framed values row(1) .. row(n) of its Ack, one
    hbtc_fr_poly_eval call for all rows (_poly_eval is the Python-integer form of one value)."""
    if not rows:
        return []
    out = ctx.fr_poly_eval([list(r) for r in rows], list(range(1, n + 1)))  # [row, x, 32]
    return [wire.frs_to_wire(out[a]) for a in range(len(rows))]


def decrypt_batch(ctx, sk, cts):
    """SecretKey::decrypt for n ciphertexts under one key (hbtc_decrypt): None where
    Ciphertext::verify fails (or u / w does not decode), else v XOR hash_bytes(sk u)."""
    if not cts:
        return []
    pts, _ = ctx.decrypt(sk, [bytes(c.u) for c in cts], [bytes(c.w) for c in cts],
                         [bytes(c.v) for c in cts])
    return pts


# ------------------------------------------------------------------------------ SyncKeyGen
class _Proposal:
    """ProposalState (:231-254): the commitment, the verified values, the acking nodes."""

    def __init__(self, commit):
        self.commit = commit
        self.values = {}       # sender_idx + 1 -> Fr
        self.acks = set()
        self.our_row = None    # our row, once it matched the commitment (fast Ack check)

    def is_complete(self, t):
        return len(self.acks) > 2 * t


class SyncKeyGen:
    """One node's SyncKeyGen instance with batched message handling (see module docstring)."""

    def __init__(self, ctx, our_id, sec_key, pub_keys, threshold, one_call=False):
        self.ctx = ctx
        self.our_id = our_id
        self.sec_key = int(sec_key)
        self.ids = sorted(pub_keys)
        self.pub_keys = {i: bytes(pub_keys[i]) for i in self.ids}
        self.index = {n: i for i, n in enumerate(self.ids)}
        self.our_idx = self.index.get(our_id)
        self.t = int(threshold)
        self.parts = {}
        self.queue = []
        # one_call: our Part and our Acks through hbtc_skg_part / hbtc_skg_acks, the recipients a key
        # set loaded once here (an observer produces nothing and loads nothing)
        self.one_call = bool(one_call) and self.our_idx is not None
        self.rcpt_keyset = None
        if self.one_call:
            self.rcpt_keyset, bad = ctx.keyset_load([self.pub_keys[n] for n in self.ids])
            if bad:
                self.close()
                raise N.HbtcError("encrypt: a public key failed to decode")

    def close(self):
        """Free the recipients' key set of a one_call instance."""
        kid, self.rcpt_keyset = self.rcpt_keyset, None
        if kid is not None and getattr(self.ctx, "h", None):
            self.ctx.keyset_free(kid)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def new(cls, ctx, our_id, sec_key, pub_keys, threshold, one_call=False):
        """SyncKeyGen::new (:293-330): the instance and our Part (None for an observer).  one_call:
        the Part and the instance's Acks are made by one device call each (hbtc_skg_part,
        hbtc_skg_acks) instead of the composed g1_mul / fr_poly_eval / encrypt calls; same bytes."""
        kg = cls(ctx, our_id, sec_key, pub_keys, threshold, one_call)
        if kg.our_idx is None:
            return kg, None
        t = kg.t
        b = [secrets.randbelow(R) for _ in range((t + 1) * (t + 2) // 2)]  # BivarPoly::random
        if kg.one_call:
            n = len(kg.ids)
            rs = [secrets.randbelow(R - 1) + 1 for _ in range(n)]
            commit, cts, st = ctx.skg_part(kg.rcpt_keyset, n, t, b, rs)
            if st.any():
                raise N.HbtcError("encrypt: a public key failed to decode")
            return kg, Part(commit, [Ciphertext(u, v, w) for u, v, w in cts])
        cm, st = ctx.g1_mul(G1_GEN, _fr_le(b))
        if st.any():
            raise N.HbtcError("commitment failed")
        commit = [bytes(cm[48 * i:48 * i + 48]) for i in range(len(b))]
        rows = bivar_rows(ctx, b, t, len(kg.ids))
        cts = encrypt_batch(ctx, [kg.pub_keys[n] for n in kg.ids], rows)
        return kg, Part(commit, cts)

    # ---------------------------------------------------------------- queue
    def handle_part(self, sender_id, part):
        self.queue.append(("part", sender_id, part))

    def handle_ack(self, sender_id, ack):
        self.queue.append(("ack", sender_id, ack))

    def flush(self):
        """Process the queue; one result per queued message, in order:
        Part -> None | ("valid", Ack) | ("invalid", [(sender, "InvalidPartMessage")]);
        Ack  -> list of faults [(sender, ("AckMessage", fault))] (empty when handled)."""
        q, self.queue = self.queue, []
        n, t, our = len(self.ids), self.t, self.our_idx
        # 1. ciphertexts addressed to us (stateless pre-pass)
        jobs = []
        for m, (kind, sender, msg) in enumerate(q):
            if our is None or sender not in self.index:
                continue
            cts = msg.rows if kind == "part" else msg.values
            if kind == "ack" and len(cts) != n:
                continue  # NodeCount: nothing to decrypt
            if our < len(cts):
                jobs.append((m, cts[our]))
        plain = dict(zip([m for m, _ in jobs], decrypt_batch(self.ctx, self.sec_key, [c for _, c in jobs])))
        # 2. decode; the commitment each message is checked against (first Part per proposer)
        rows, vals, commit_of = {}, {}, {}
        first_part = {p: st.commit for p, st in self.parts.items()}
        for m, (kind, sender, msg) in enumerate(q):
            if sender not in self.index:
                continue
            if kind == "part":
                s_idx = self.index[sender]
                if s_idx not in first_part:
                    first_part[s_idx] = msg.commit
                    commit_of[m] = msg.commit
                if m in plain and plain[m] is not None:
                    try:
                        row = wire.poly_from_wire(plain[m])
                        rows[m] = row if len(row) == t + 1 else None
                    except wire.WireError:
                        rows[m] = None
            else:
                if m in plain and plain[m] is not None:
                    try:
                        vals[m] = wire.fr_value_from_wire(plain[m])
                    except wire.WireError:
                        vals[m] = None
                if msg.proposer in first_part:
                    commit_of[m] = first_part[msg.proposer]
        # 3. batched checks: rows of the stored Parts, values of every decodable Ack
        row_ok = {}
        pm = [m for m in rows if rows[m] is not None and m in commit_of]
        if pm:
            st = self.ctx.skg_check_parts(t, our, [p for m in pm for p in commit_of[m]],
                                          [rows[m] for m in pm])
            row_ok = {m: int(st[i]) == N.ACCEPT for i, m in enumerate(pm)}
        val_ok = {}
        am = [m for m in vals if vals[m] is not None and m in commit_of]
        if am:
            val_ok = self._check_values(q, am, vals, commit_of, rows, row_ok)
        # 4. replay in order
        out, new_acks = [], []
        for m, (kind, sender, msg) in enumerate(q):
            if kind == "part":
                out.append(self._replay_part(m, sender, msg, plain, rows, row_ok, new_acks))
            else:
                out.append(self._replay_ack(m, sender, msg, plain, vals, val_ok))
        self._emit_acks(new_acks, out)
        return out

    def _check_values(self, q, am, vals, commit_of, rows, row_ok):
        t, our = self.t, self.our_idx
        keys, commits, prow, pok = {}, [], [], []
        for m in am:
            c = commit_of[m]
            key = id(c)
            if key not in keys:
                keys[key] = len(commits)
                commits.append(c)
                # our verified row for this commitment, if we have one: the scalar fast path
                row = None
                for st in self.parts.values():
                    if st.commit is c and st.our_row is not None:
                        row = st.our_row
                for mm, r in rows.items():
                    if row is None and r is not None and row_ok.get(mm) and commit_of.get(mm) is c:
                        row = r
                prow.append(row if row is not None else [0] * (t + 1))
                pok.append(1 if row is not None else 0)
        ack_part = [keys[id(commit_of[m])] for m in am]
        ack_sender = [self.index[q[m][1]] for m in am]
        st = self.ctx.skg_check_acks(t, our, [p for c in commits for p in c], prow, pok, ack_part,
                                     ack_sender, [vals[m] for m in am])
        return {m: int(st[i]) == N.ACCEPT for i, m in enumerate(am)}

    def _replay_part(self, m, sender, part, plain, rows, row_ok, new_acks):  # :338-381
        if sender not in self.index:
            return None
        s_idx = self.index[sender]
        if s_idx in self.parts:
            return None  # multiple parts: ignored
        st = _Proposal(part.commit)
        self.parts[s_idx] = st
        if self.our_idx is None:
            return None
        if self.our_idx >= len(part.rows) or plain.get(m) is None:
            return None  # rows.get(our_idx)? / decrypt(..)?
        if rows.get(m) is None or not row_ok.get(m, False):
            return ("invalid", [(sender, "InvalidPartMessage")])
        st.our_row = rows[m]
        new_acks.append((m, s_idx, rows[m]))
        return ("valid", None)  # the Ack is filled in by _emit_acks

    def _replay_ack(self, m, sender, ack, plain, vals, val_ok):  # :387-396, :462-498
        if sender not in self.index:
            return []
        s_idx = self.index[sender]

        def fault(kind):
            return [(sender, ("AckMessage", kind))]
        if len(ack.values) != len(self.ids):
            return fault("NodeCount")
        st = self.parts.get(ack.proposer)
        if st is None:
            return fault("SenderExist")
        if s_idx in st.acks:
            return fault("DuplicateAck")
        st.acks.add(s_idx)
        if self.our_idx is None:
            return []
        if plain.get(m) is None:
            return fault("ValueDecryption")
        if vals.get(m) is None:
            return fault("ValueDeserialization")
        if not val_ok.get(m, False):  # checked against this (the stored) commitment
            return fault("ValueInvalid")
        st.values[s_idx + 1] = vals[m]
        return []

    def _emit_acks(self, new_acks, out):
        """Ack(sender_idx, values): row(idx + 1) encrypted to every node (:371-380), batched."""
        if not new_acks:
            return
        n = len(self.ids)
        if self.one_call:
            rs = [secrets.randbelow(R - 1) + 1 for _ in range(n * len(new_acks))]
            raw, st = self.ctx.skg_acks(self.rcpt_keyset, n, [list(row) for _, _, row in new_acks], rs)
            if st.any():
                raise N.HbtcError("encrypt: a public key failed to decode")
            cts = [Ciphertext(u, v, w) for u, v, w in raw]
            for a, (m, s_idx, _) in enumerate(new_acks):
                out[m] = ("valid", Ack(s_idx, cts[a * n:(a + 1) * n]))
            return
        msgs = [m for vals in ack_values(self.ctx, [row for _, _, row in new_acks], n) for m in vals]
        pks = [self.pub_keys[self.ids[i]] for i in range(n)] * len(new_acks)
        cts = encrypt_batch(self.ctx, pks, msgs)
        for a, (m, s_idx, _) in enumerate(new_acks):
            out[m] = ("valid", Ack(s_idx, cts[a * n:(a + 1) * n]))

    # ---------------------------------------------------------------- keys
    def count_complete(self):
        return sum(1 for st in self.parts.values() if st.is_complete(self.t))

    def is_node_ready(self, proposer_id):
        st = self.parts.get(self.index.get(proposer_id))
        return bool(st and st.is_complete(self.t))

    def is_ready(self):
        return self.count_complete() > self.t

    def _generate(self, n_nodes, load_keyset):
        """One hbtc_skg_generate call over the complete Parts: (commit, sk, pk_shares, keyset id)."""
        t = self.t
        done = [self.parts[p] for p in sorted(self.parts) if self.parts[p].is_complete(t)]
        if not done:
            # Poly::zero().commitment(): no coefficients, so every share is the point at infinity
            # and there is nothing to load
            return [], (0 if self.our_idx is not None else None), [G1_INF] * n_nodes, None
        row0 = [[st.commit[coeff_pos(0, j)] for j in range(t + 1)] for st in done]
        values = None
        if self.our_idx is not None:  # Poly::interpolate(values.take(t + 1)).evaluate(0)
            values = [sorted(st.values.items())[:t + 1] for st in done]
        commit, sk, pks, kid, status = self.ctx.skg_generate(t, row0, values, n_nodes, load_keyset)
        if status == N.DECODE_ERR:
            raise N.HbtcError("generate: a commitment point failed to decode")
        if status != N.ACCEPT:
            raise N.HbtcError("generate: %s" % N.STATUS_NAMES.get(status, status))
        return commit, sk, pks, kid

    def generate(self):
        """(public key set commitment [t+1 compressed G1], our secret key share or None)."""
        commit, sk, _, _ = self._generate(0, False)
        return commit, sk

    def generate_keys(self):
        """SyncKeyGen::generate followed by NetworkInfo::new in one device call: (commit, our secret
        key share or None, every node's public key share, the id of the key set loaded from those
        shares with commit[0] as its master key; None when no Part is complete)."""
        return self._generate(len(self.ids), True)

    def public_key_shares(self, commit):
        """public_key_share(i) = commitment.evaluate(i + 1) for every node (messaging.rs:253-256)."""
        pks, st = self.ctx.commitment_evaluate(commit, [i + 1 for i in range(len(self.ids))])
        if st.any():
            raise N.HbtcError("public key shares: commitment failed to decode")
        return pks


def _poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def _bivar_row(b, t, x):
    xp = [pow(x, j, R) for j in range(t + 1)]
    return [sum(b[coeff_pos(i, j)] * xp[j] for j in range(t + 1)) % R for i in range(t + 1)]


def _lagrange_at_zero(items):
    """Poly::interpolate(items).evaluate(0) over (x, y) pairs with distinct x."""
    xs = [x % R for x, _ in items]
    acc = 0
    for x, y in items:
        num, den = 1, 1
        for x0 in xs:
            if x0 != x % R:
                num = num * x0 % R
                den = den * (x0 - x) % R
        acc = (acc + y * num * pow(den, R - 2, R)) % R
    return acc
