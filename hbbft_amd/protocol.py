"""Batch queues for hbbft's crypto call sites — the host-side mirror of the reference's Coin and
ThresholdDecryption decision logic, driving the GPU verifier.

The reference verifies every share synchronously on arrival (src/coin.rs:149-161,
src/threshold_decryption.rs:120-161).  Here every instance of an epoch queues its events; one
``flush`` verifies all queued shares of all instances in ONE batched GPU call, then REPLAYS each
instance's queue in arrival order with those verdicts.  Verdicts depend only on (sender, share,
nonce/ciphertext), never on protocol state, so the replay produces exactly the reference's faults,
errors and outputs; shares that arrive after termination are verified needlessly but, as in the
reference (coin.rs:105, td.rs:121-123), produce nothing.  Combines triggered during the replay
(try_output) are batched too; an instance whose deferred combine fails is replayed again in
synchronous mode so the reference's retry-on-error behaviour is kept.

Inputs are hbbft's wire encodings (compressed points).  By default H = hash_g2(nonce) /
hash_g1_g2(u, v) and this node's own share are supplied by the caller, as before.  With
``sk_share=`` (this node's secret key share, an int) the queues make both on the GPU instead:
CoinEpoch's flush signs every instance added with a nonce in ONE ctx.sign_shares call
(SecretKeyShare::sign, coin.rs:142), and DecryptionEpoch's flush replaces its ciphertext check
by ONE ctx.decrypt_shares call (SecretKeyShare::decrypt_share, td.rs:98: H, Ciphertext::verify
and sk u); ``own_share(key)`` is the share to multicast.  ThresholdDecryption outputs the combined point
g = sum l_i d_i (compressed) by default; DecryptionEpoch(plaintext=True) outputs what the
reference's try_output does, the plaintext v XOR hash_bytes(g, |v|), made on the GPU behind the
combine (hbtc_threshold_decrypt).  CoinEpoch(decide=True) sends a flush through ONE
ctx.coin_decide call (checks, combine, master check) and keeps that call's result for every
instance whose deferred combine would take exactly the items the call selected.
"""
from . import _native as N


def _step(faults=None, output=None, error=None):
    return {"faults": list(faults or []), "output": output, "error": error}


class NetInfo:
    """The parts of NetworkInfo (src/messaging.rs:222-269) the hot path reads."""

    def __init__(self, node_ids, our_id, keyset_id, master_pk=None):
        self.ids = sorted(node_ids)
        self.index = {n: i for i, n in enumerate(self.ids)}
        self.our_id = our_id
        self.num_faulty = (len(self.ids) - 1) // 3  # messaging.rs:260
        self.keyset = keyset_id
        self.master_pk = master_pk

    def is_validator(self):
        return self.our_id in self.index


# ================================================================================== Coin
class _CoinState:
    def __init__(self, H, our_share, nonce=None):
        self.H = H
        self.our_share = our_share
        self.nonce = nonce
        self.events = []
        self.received = {}
        self.had_input = False
        self.terminated = False


def coin_call_selection(counts, idx, sigs, status, t):
    """What one coin_decide call combined, worked out on the host from its item statuses: per
    instance the first t ACCEPTed items in call order as a frozenset of (node index, share
    bytes), or None when the instance has fewer than t of them."""
    sel, pos = [], 0
    for c in counts:
        acc = [j for j in range(pos, pos + c) if int(status[j]) == N.ACCEPT][:t]
        sel.append(frozenset((int(idx[j]), bytes(sigs[j])) for j in acc) if len(acc) == t else None)
        pos += c
    return sel


def coin_call_serves(selected, items, t):
    """Whether the call's result for an instance is the deferred combine's: `items` is what
    _try_output hands the combine (node index, share), sorted by node index; the combine takes
    its first t.  True when those are exactly the t distinct items the call selected -- shares
    carried over from an earlier flush, an input after more than t shares, or a repeated sender
    make the two differ (or the selection hold fewer than t distinct items)."""
    if selected is None or len(selected) != t or len(items) < t:
        return False
    return frozenset((int(i), bytes(s)) for i, s in items[:t]) == selected


class CoinEpoch:
    """Every Coin instance (coin.rs:64) of one epoch behind one batch queue.

    decide=False (the default): a flush is ctx.verify_sig_shares, then one combine_sigs and one
    verify_sigs for the instances that reach their threshold.  decide=True, with the NetInfo's
    master_pk: the flush sends the same items through ONE ctx.coin_decide call, and an instance
    whose deferred combine would take exactly the items that call selected uses the call's
    result; any other instance goes through the combine as before.  `decided` and `fallback`
    count the instances that took each path."""

    def __init__(self, ctx, netinfo, *, sk_share=None, decide=False):
        self.ctx = ctx
        self.ni = netinfo
        self.inst = {}
        self.sk_share = sk_share
        self.decide = bool(decide) and netinfo.master_pk is not None
        self.decided = 0
        self.fallback = 0
        if self.decide:  # once: the key set keeps the decoded master key resident
            ctx.keyset_set_master(netinfo.keyset, netinfo.master_pk)

    def add(self, key, H_c96=None, our_share_c96=None, nonce=None):
        """H_c96 (and our_share_c96 for a validator) from the caller, or, with sk_share set,
        nonce=...: the next flush makes H = hash_g2(nonce) and the share sk_share H."""
        if H_c96 is None:
            if nonce is None or self.sk_share is None:
                raise ValueError("an instance needs H_c96, or a nonce and the epoch's sk_share")
            self.inst[key] = _CoinState(None, None, bytes(nonce))
        else:
            self.inst[key] = _CoinState(bytes(H_c96), our_share_c96)

    def own_share(self, key):
        """This node's signature share of the instance (coin.rs:142), None for an observer or
        before the flush that signs it."""
        return self.inst[key].our_share if self.ni.is_validator() else None

    def H(self, key):
        return self.inst[key].H

    def _sign_own(self):
        todo = [k for k, st in self.inst.items() if st.H is None and st.nonce is not None]
        if not todo:
            return
        sigs, Hs = self.ctx.sign_shares(self.sk_share, [self.inst[k].nonce for k in todo])
        for k, sg, h in zip(todo, sigs, Hs):
            self.inst[k].H = h
            if self.ni.is_validator():
                self.inst[k].our_share = sg

    def handle_input(self, key):
        self.inst[key].events.append(("input",))

    def handle_message(self, key, sender, share_c96):
        self.inst[key].events.append(("msg", sender, bytes(share_c96)))

    # ---------------------------------------------------------------- flush
    def flush(self):
        """Verify every queued share in one GPU call, replay, batch the combines.  Returns
        {key: [step per queued event]}."""
        ni = self.ni
        self._sign_own()
        keys = [k for k in self.inst if self.inst[k].events]
        # state at the start of the flush: a failed deferred combine replays from here
        snap = {k: (dict(self.inst[k].received), self.inst[k].had_input, self.inst[k].terminated)
                for k in keys}
        counts, idx, sigs, where = [], [], [], {}
        for k in keys:
            st = self.inst[k]
            c = 0
            if st.terminated:  # coin.rs:105: nothing after termination is looked at
                counts.append(0)
                continue
            for e_i, ev in enumerate(st.events):
                share = None
                sender = None
                if ev[0] == "input" and ni.is_validator() and st.our_share is not None:
                    sender, share = ni.our_id, st.our_share
                elif ev[0] == "msg":
                    sender, share = ev[1], ev[2]
                if share is not None and sender in ni.index:
                    where[(k, e_i)] = len(idx)
                    idx.append(ni.index[sender])
                    sigs.append(share)
                    c += 1
            counts.append(c)
        verdict = {}
        call = {}  # decide: per instance (the call's selection, coin status, parity)
        if idx:
            Hs = [self.inst[k].H for k in keys]
            if self.decide:
                t = ni.num_faulty + 1
                status, _, par, cst = self.ctx.coin_decide(ni.keyset, Hs, counts, idx, sigs, t)
                sel = coin_call_selection(counts, idx, sigs, status, t)
                call = {k: (sel[j], int(cst[j]), bool(par[j])) for j, k in enumerate(keys)}
            else:
                status = self.ctx.verify_sig_shares(ni.keyset, Hs, counts, idx, sigs)
            for key_ev, pos in where.items():
                verdict[key_ev] = int(status[pos]) == N.ACCEPT
        results, pending = {}, []
        for k in keys:
            results[k] = self._replay(k, verdict, pending)
        self._finish_combines(pending, results, verdict, snap, call)
        for k in keys:
            self.inst[k].events = []
        return results

    def _replay(self, k, verdict, pending, sync=False):
        st, ni = self.inst[k], self.ni
        steps = []
        for e_i, ev in enumerate(st.events):
            if ev[0] == "input":
                if st.had_input:
                    steps.append(_step())
                    continue
                st.had_input = True
                if not ni.is_validator():
                    steps.append(self._try_output(k, e_i, pending, sync))
                else:
                    steps.append(self._handle_share(k, e_i, ni.our_id, verdict, pending, sync))
            else:
                if st.terminated:
                    steps.append(_step())
                else:
                    steps.append(self._handle_share(k, e_i, ev[1], verdict, pending, sync))
        return steps

    def _handle_share(self, k, e_i, sender, verdict, pending, sync):  # coin.rs:149-161
        st, ni = self.inst[k], self.ni
        if sender not in ni.index:
            return _step(error="UnknownSender")
        if not verdict.get((k, e_i), False):
            return _step(faults=[(sender, "UnverifiedSignatureShareSender")])
        ev = st.events[e_i]
        st.received[sender] = ev[2] if ev[0] == "msg" else st.our_share
        return self._try_output(k, e_i, pending, sync)

    def _try_output(self, k, e_i, pending, sync):  # coin.rs:163-181
        st, ni = self.inst[k], self.ni
        if st.had_input and len(st.received) > ni.num_faulty:
            items = [(ni.index[i], st.received[i]) for i in sorted(st.received)]
            step = _step()
            if sync:
                res = self._combine([k], [items])[0]
                if res[0] is not None:
                    step["error"] = res[0]
                    return step
                step["output"] = res[1]
            else:
                pending.append((k, e_i, items, step))
            st.terminated = True
            return step
        return _step()

    def _combine(self, keys, item_lists):
        """[(error-or-None, parity)] via one hbtc_combine_sigs + one hbtc_verify_sigs call
        (the master-key check of coin.rs:192-197)."""
        t = self.ni.num_faulty + 1
        counts = [len(it) for it in item_lists]
        idx = [i for it in item_lists for i, _ in it]
        sigs = [s for it in item_lists for _, s in it]
        out, par, cst = self.ctx.combine_sigs(counts, idx, sigs, t)
        res = [None] * len(item_lists)
        ok_pos = [j for j in range(len(item_lists)) if int(cst[j]) == N.ACCEPT]
        for j in range(len(item_lists)):
            if int(cst[j]) != N.ACCEPT:
                res[j] = ("CombineAndVerifySigCrypto:%s" % N.STATUS_NAMES[int(cst[j])], None)
        if ok_pos and self.ni.master_pk is not None:
            Hs = [self.inst[keys[j]].H for j in ok_pos]
            vs = self.ctx.verify_sigs([self.ni.master_pk] * len(ok_pos), Hs, [out[j] for j in ok_pos])
            for j, v in zip(ok_pos, vs):
                res[j] = (None, bool(par[j])) if int(v) == N.ACCEPT else ("VerificationFailed", None)
        else:
            for j in ok_pos:
                res[j] = (None, bool(par[j]))
        return res

    def _finish_combines(self, pending, results, verdict, snap, call=None):
        if not pending:
            return
        t = self.ni.num_faulty + 1
        res = [None] * len(pending)
        rest = []
        for j, (k, e_i, items, step) in enumerate(pending):
            sel, cst, parity = (call or {}).get(k, (None, None, None))
            if not coin_call_serves(sel, items, t):
                rest.append(j)
            elif cst == N.ACCEPT:
                res[j] = (None, parity)
            elif cst == N.REJECT:  # the master check of coin.rs:192-197
                res[j] = ("VerificationFailed", None)
            else:
                res[j] = ("CombineAndVerifySigCrypto:%s" % N.STATUS_NAMES[cst], None)
        self.decided += len(pending) - len(rest)
        self.fallback += len(rest) if self.decide else 0
        if rest:
            for j, r in zip(rest, self._combine([pending[j][0] for j in rest], [pending[j][2] for j in rest])):
                res[j] = r
        failed = set()
        for (k, e_i, items, step), (err, parity) in zip(pending, res):
            if err is None:
                step["output"] = parity
            else:
                failed.add(k)
        for k in failed:  # rare: redo this flush of the instance with synchronous combines,
            st = self.inst[k]  # from its state at the start of the flush (coin.rs:163-181 retries)
            received, had_input, terminated = snap[k]
            st.received, st.had_input, st.terminated = dict(received), had_input, terminated
            results[k] = self._replay(k, verdict, [], sync=True)


# ================================================================================== ThresholdDecryption
class _TdState:
    def __init__(self, our_share):
        self.our_share = our_share
        self.events = []
        self.ct = None  # (u_c48, v, w_c96, H_c96)
        self.shares = {}
        self.terminated = False


class DecryptionEpoch:
    """Every ThresholdDecryption instance (threshold_decryption.rs:45) of one epoch.

    plaintext=False: a terminated instance outputs the combined point g (48 bytes).
    plaintext=True: it outputs the plaintext bytes, as try_output does (td.rs:187): the flush's
    pending combines go through ONE ctx.threshold_decrypt call (shares -> g -> plaintext on the
    device) with the v, w and H of each instance's stored ciphertext.  That call verifies the
    shares it combines once more, this node's own share included.

    sk_share=None: the caller passes H with every ciphertext and this node's share with add().
    sk_share set: both may be omitted; the flush's ONE ctx.decrypt_shares call over the queued
    ciphertexts gives their validity, their H and this node's shares."""

    def __init__(self, ctx, netinfo, plaintext=False, *, sk_share=None):
        self.ctx = ctx
        self.ni = netinfo
        self.inst = {}
        self.plaintext = plaintext
        self.sk_share = sk_share

    def add(self, key, our_share_c48=None):
        self.inst[key] = _TdState(our_share_c48)

    def set_ciphertext(self, key, u_c48, v, w_c96, H_c96=None):
        if H_c96 is None and self.sk_share is None:
            raise ValueError("a ciphertext needs H_c96, or the epoch's sk_share")
        self.inst[key].events.append(("ct", (bytes(u_c48), bytes(v), bytes(w_c96),
                                             None if H_c96 is None else bytes(H_c96))))

    def own_share(self, key):
        """The share to multicast (td.rs:107-108): None before the instance has a valid
        ciphertext, and for an observer."""
        st = self.inst[key]
        return st.our_share if self.ni.is_validator() and st.ct is not None else None

    def handle_message(self, key, sender, share_c48):
        self.inst[key].events.append(("msg", sender, bytes(share_c48)))

    def flush(self):
        ni = self.ni
        keys = [k for k in self.inst if self.inst[k].events]
        # every queued ciphertext of an instance that has none yet: set_ciphertext leaves the
        # instance without one after an invalid ciphertext (td.rs:94-105), so a later valid one
        # in the same queue is accepted
        ct_ev = []
        for k in keys:
            st = self.inst[k]
            if st.ct is None:
                ct_ev += [(k, e_i, ev[1]) for e_i, ev in enumerate(st.events) if ev[0] == "ct"]
        ct_ok, own = {}, {}
        if ct_ev and self.sk_share is not None:
            # SecretKeyShare::decrypt_share (td.rs:98) of every queued ciphertext in one call
            g, Hs, vs = self.ctx.decrypt_shares(self.sk_share, [c[0] for _, _, c in ct_ev],
                                                [c[1] for _, _, c in ct_ev], [c[2] for _, _, c in ct_ev])
            ct_ev = [(k, e_i, c[:3] + (h,)) for (k, e_i, c), h in zip(ct_ev, Hs)]
            for (k, e_i, c), v, gi in zip(ct_ev, vs, g):
                self.inst[k].events[e_i] = ("ct", c)  # H is stored with the ciphertext
                ct_ok[(k, e_i)] = int(v) == N.ACCEPT
                own[(k, e_i)] = gi
        elif ct_ev:
            vs = self.ctx.verify_ciphertexts([c[0] for _, _, c in ct_ev], [c[3] for _, _, c in ct_ev],
                                             [c[2] for _, _, c in ct_ev])
            for (k, e_i, _), v in zip(ct_ev, vs):
                ct_ok[(k, e_i)] = int(v) == N.ACCEPT
        # the ciphertext each instance will know by the end of its queue: the stored one, else
        # the first valid queued one
        ct_of = {}
        for k in keys:
            st = self.inst[k]
            ct = st.ct
            if ct is None:
                ct = next((ev[1] for e_i, ev in enumerate(st.events)
                           if ev[0] == "ct" and ct_ok.get((k, e_i), False)), None)
            ct_of[k] = ct
        # shares that will be checked against that ciphertext: the stored (still unverified)
        # ones when it is set in this flush (remove_invalid_shares, td.rs:136-149), and every
        # queued message of an instance that has not terminated (td.rs:121-128)
        vkeys, counts, idx, shares, where = [], [], [], [], {}
        for k in keys:
            st, ct = self.inst[k], ct_of[k]
            if ct is None or st.terminated:
                continue
            cand = [("stored", s, sh) for s, sh in st.shares.items()] if st.ct is None else []
            cand += [("ev%d" % e_i, ev[1], ev[2]) for e_i, ev in enumerate(st.events) if ev[0] == "msg"]
            c = 0
            for tag, sender, sh in cand:
                if sender in ni.index:
                    where[(k, tag, sender)] = len(idx)
                    idx.append(ni.index[sender])
                    shares.append(sh)
                    c += 1
            if c:
                vkeys.append(k)
                counts.append(c)
        verdict = {}
        if idx:
            status = self.ctx.verify_dec_shares(ni.keyset, [ct_of[k][3] for k in vkeys],
                                                [ct_of[k][2] for k in vkeys], counts, idx, shares)
            for key, pos in where.items():
                verdict[key] = int(status[pos]) == N.ACCEPT
        results, pending = {}, []
        for k in keys:
            results[k] = self._replay(k, verdict, ct_ok, pending, own)
        if pending:
            t = ni.num_faulty + 1
            counts = [len(p[2]) for p in pending]
            idx = [i for p in pending for i, _ in p[2]]
            shares = [s for p in pending for _, s in p[2]]
            if self.plaintext:
                cts = [self.inst[p[0]].ct for p in pending]  # (u, v, w, H) of a terminated instance
                _, g, _, cst = self.ctx.threshold_decrypt(ni.keyset, [c[3] for c in cts], [c[2] for c in cts],
                                                          counts, idx, shares, t, [c[1] for c in cts])
            else:
                g, cst = self.ctx.combine_dec(counts, idx, shares, t)
            for (k, step, items), gk, c in zip(pending, g, cst):
                if int(c) == N.ACCEPT:
                    step["output"] = gk
                else:
                    step["error"] = "Decryption:%s" % N.STATUS_NAMES[int(c)]
        for k in keys:
            self.inst[k].events = []
            for step in results[k]:
                step.pop("_pending", None)
        return results

    def _valid(self, k, tag, sender, verdict):  # td.rs:152-161 (with the ciphertext known)
        if sender not in self.ni.index:
            return False
        return verdict.get((k, tag, sender), False)

    def _replay(self, k, verdict, ct_ok, pending, own):
        st, ni = self.inst[k], self.ni
        steps = []
        stored_tag = {s: "stored" for s in st.shares}
        for e_i, ev in enumerate(st.events):
            if ev[0] == "ct":  # set_ciphertext, td.rs:94-113
                if st.ct is not None:
                    steps.append(_step(error="MultipleInputs"))
                    continue
                if not ct_ok.get((k, e_i), False):
                    steps.append(_step(error="InvalidCiphertext"))
                    continue
                st.ct = ev[1]
                bad = [s for s in sorted(st.shares) if not self._valid(k, stored_tag[s], s, verdict)]
                for s in bad:
                    del st.shares[s]
                step = _step(faults=[(s, "UnverifiedDecryptionShareSender") for s in bad])
                if ni.is_validator():
                    if (k, e_i) in own:
                        st.our_share = own[(k, e_i)]
                    st.shares[ni.our_id] = st.our_share
                    stored_tag[ni.our_id] = "own"
                r = self._try_output(k, pending)
                step["faults"] += r["faults"]
                step["output"] = r["output"]
                if r is not step and r.get("_pending"):
                    pending[-1] = (pending[-1][0], step, pending[-1][2])
                steps.append(step)
            else:  # handle_message, td.rs:120-133
                sender, share = ev[1], ev[2]
                if st.terminated:
                    steps.append(_step())
                    continue
                tag = "ev%d" % e_i
                if st.ct is not None and not self._valid(k, tag, sender, verdict):
                    steps.append(_step(faults=[(sender, "UnverifiedDecryptionShareSender")]))
                    continue
                dup = sender in st.shares
                st.shares[sender] = share
                stored_tag[sender] = tag
                if dup:
                    steps.append(_step(faults=[(sender, "MultipleDecryptionShares")]))
                    continue
                steps.append(self._try_output(k, pending))
        return steps

    def _try_output(self, k, pending):  # td.rs:164-188
        st, ni = self.inst[k], self.ni
        if st.terminated or len(st.shares) <= ni.num_faulty or st.ct is None:
            return _step()
        st.terminated = True
        items = [(ni.index[i], st.shares[i]) for i in sorted(st.shares)]
        step = _step()
        step["_pending"] = True
        pending.append((k, step, items))
        return step
