"""DecryptionEpoch(plaintext=True): the batch queue outputs what the reference's try_output does,
the plaintext v XOR hash_bytes(g, |v|) (threshold_decryption.rs:187), through ONE
ctx.threshold_decrypt call per flush; the default mode still outputs g.  CPU only.

The scenarios are those of tests/test_protocol.py's run_decryption (its generator and its replay
against oracle/hbbft_rules.py), run here with the epoch switched to plaintext mode and the restated
rules' decrypt extended by the pad; the context is a stand-in computing with the C oracle."""
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from hbbft_amd import protocol as P
from oracle import bls12_381 as B
from oracle import cbaseline as cb
from oracle import hbbft_rules as RULES
from oracle import threshold_crypto as TC
from tests import test_protocol as TP


def _pad_xor(g48, v):
    return bytes(a ^ b for a, b in zip(v, TC.hash_bytes(B.g1_decompress(g48), len(v))))


class PlainOracleCtx(TP.OracleCtx):
    """OracleCtx plus threshold_decrypt: the shares verified by the C oracle's pairing check, the
    first t ACCEPTed ones combined, the plaintext by oracle.threshold_crypto.hash_bytes."""

    def __init__(self, allow_plain=True):
        super().__init__()
        self.allow_plain = allow_plain
        self.plain_calls = 0
        self.combine_calls = 0

    def combine_dec(self, counts, idx, shares, t):
        self.combine_calls += 1
        return super().combine_dec(counts, idx, shares, t)

    def threshold_decrypt(self, ks, H, w, counts, idx, shares, t, vs, offsets=None):
        assert self.allow_plain, "the default mode must not ask for plaintexts"
        assert offsets is None and len(H) == len(w) == len(vs) == len(counts)
        self.plain_calls += 1
        st = self.verify_dec_shares(ks, H, w, counts, idx, shares)
        plains, gs, cst, pos = [], [], [], 0
        for k, c in enumerate(counts):
            kept = [j for j in range(pos, pos + c) if st[j] == N.ACCEPT][:t]
            s, g = cb.combine(1, [idx[j] for j in kept], [shares[j] for j in kept], t)
            cst.append({0: N.ACCEPT, 5: N.NOT_ENOUGH_SHARES, 6: N.DUPLICATE_ENTRY}.get(s, N.DECODE_ERR))
            gs.append(g if s == 0 else bytes(48))
            plains.append(_pad_xor(g, vs[k]) if s == 0 else None)
            pos += c
        return st, plains, gs, np.array(cst, np.int32)


class _Recorder:
    """Wraps DecryptionEpoch so every flush's steps are kept, in order."""

    def __init__(self, log, **kw):
        self.log, self.kw = log, kw

    def __call__(self, ctx, ni):
        ep = P_DecryptionEpoch(ctx, ni, **self.kw)
        flush, log = ep.flush, self.log

        def recording_flush():
            res = flush()
            log.append({k: [dict(s) for s in steps] for k, steps in res.items()})
            return res

        ep.flush = recording_flush
        return ep


P_DecryptionEpoch = P.DecryptionEpoch
RULES_ThresholdDecryption = RULES.ThresholdDecryption


def _run(monkeypatch, seed, plaintext, **kw):
    """run_decryption's scenarios and its comparison with the restated rules; returns the steps of
    every flush and the context."""
    log = []
    ctx = PlainOracleCtx(allow_plain=plaintext)
    monkeypatch.setattr(P, "DecryptionEpoch", _Recorder(log, **({"plaintext": True} if plaintext else {})))
    if plaintext:
        def rules(ids, our, f, own, verify, decrypt, ct_valid):  # PublicKeySet::decrypt, whole
            return RULES_ThresholdDecryption(ids, our, f, own, verify,
                                             lambda items, ct: _pad_xor(decrypt(items, ct), ct[1]), ct_valid)
        monkeypatch.setattr(RULES, "ThresholdDecryption", rules)
    TP.run_decryption(ctx, random.Random(seed), **kw)  # asserts steps == the reference rules'
    return log, ctx


@pytest.mark.parametrize("seed", [3, 4, 21])
def test_plaintext_mode_outputs_the_reference_plaintext(monkeypatch, seed):
    log, ctx = _run(monkeypatch, seed, True)
    outs = [s["output"] for fl in log for steps in fl.values() for s in steps if s["output"] is not None]
    assert outs and all(isinstance(o, bytes) and len(o) == 24 for o in outs)  # the scenarios' |v|
    # one threshold_decrypt call per flush that had a pending combine, and no combine_dec
    assert ctx.combine_calls == 0
    assert 1 <= ctx.plain_calls <= len(log)


@pytest.mark.parametrize("seed", [3, 4])
def test_faults_and_errors_equal_the_default_mode(monkeypatch, seed):
    plain, _ = _run(monkeypatch, seed, True, n_flush=3)
    monkeypatch.undo()
    default, dctx = _run(monkeypatch, seed, False, n_flush=3)
    assert dctx.plain_calls == 0 and dctx.combine_calls >= 1
    assert len(plain) == len(default)
    n_out = 0
    for fp, fd in zip(plain, default):
        assert fp.keys() == fd.keys()
        for k in fp:
            assert len(fp[k]) == len(fd[k])
            for sp, sd in zip(fp[k], fd[k]):
                assert sp["faults"] == sd["faults"] and sp["error"] == sd["error"]
                assert (sp["output"] is None) == (sd["output"] is None)
                n_out += sp["output"] is not None
    assert n_out >= 1


def test_default_mode_still_outputs_g(monkeypatch):
    log, ctx = _run(monkeypatch, 3, False)
    outs = [s["output"] for fl in log for steps in fl.values() for s in steps if s["output"] is not None]
    assert outs
    for g in outs:
        assert len(g) == 48 and B.g1_decompress(g) is not None
    assert P_DecryptionEpoch.__init__.__defaults__ == (False,)
