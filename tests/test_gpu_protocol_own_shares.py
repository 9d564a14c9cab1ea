"""DecryptionEpoch and CoinEpoch with sk_share= (the queues make H and this node's own shares on
the GPU: one decrypt_shares / sign_shares call per flush) against the same queues fed H and the
own share by the caller, as before: one scripted event sequence at N = 4, as a validator and as
an observer; the step lists must be equal and own_share() must be the supplied share."""
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from hbbft_amd import protocol as P
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
IDS = [0, 1, 2, 3]
OBSERVER = 9


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def net(ctx):
    """N = 4, f = 1: key shares f(i + 1) of a degree-1 polynomial, the key set, three ciphertexts
    under the master key and three coin nonces, with every node's shares by the existing calls."""
    rng = random.Random(4242)
    f = [rng.randrange(1, R) for _ in range(2)]
    ev = ctx.fr_poly_eval([f], [1, 2, 3, 4])
    sks = [int.from_bytes(ev[0, j].tobytes(), "little") for j in range(4)]
    out, st = ctx.g1_mul(G1, sks + [f[0]])
    assert not st.any()
    pks = [bytes(out[48 * i:48 * i + 48]) for i in range(4)]
    master = bytes(out[192:240])
    ks, bad = ctx.keyset_load(pks)
    assert bad == 0
    ctx.keyset_set_master(ks, master)
    msgs = [b"contribution a", bytes(range(90)), b"c"]
    cts, st = ctx.encrypt(master, [rng.randrange(1, R) for _ in msgs], msgs)
    assert not st.any()
    H = ctx.hash_g1_g2_batch([c[0] for c in cts], [c[1] for c in cts])
    dec = {}  # (ciphertext, node) -> decryption share
    for j in range(4):
        g, st = ctx.g1_mul([c[0] for c in cts], [sks[j]] * 3)
        assert not st.any()
        for k in range(3):
            dec[(k, j)] = bytes(g[48 * k:48 * k + 48])
    nonces = [b"Nonce for Honey Badger @0:1:0", b"Nonce for Honey Badger @0:2:1", b""]
    cH = ctx.hash_g2_batch(nonces)
    sig = {}
    for j in range(4):
        s, st = ctx.g2_mul(cH, [sks[j]] * 3)
        assert not st.any()
        for k in range(3):
            sig[(k, j)] = bytes(s[96 * k:96 * k + 96])
    yield {"ks": ks, "master": master, "sks": sks, "cts": cts, "H": H, "dec": dec, "nonces": nonces,
           "cH": cH, "sig": sig}
    ctx.keyset_free(ks)


def _strip(res):
    return {k: [(s["faults"], s["output"], s["error"]) for s in steps] for k, steps in res.items()}


def _run_decryption(ctx, net, our, own_mode):
    """The scripted sequence; own_mode: the queue makes H and the own share.  Returns the step
    lists of both flushes and own_share() of every instance after each."""
    ni = P.NetInfo(IDS, our, net["ks"], net["master"])
    validator = our in IDS
    sk = net["sks"][our] if validator else 1  # an observer's share is never used
    ep = P.DecryptionEpoch(ctx, ni, sk_share=sk) if own_mode else P.DecryptionEpoch(ctx, ni)
    cts, H, dec = net["cts"], net["H"], net["dec"]

    def add(key, k):
        if own_mode or not validator:
            ep.add(key)
        else:
            ep.add(key, dec[(k, our)])

    def set_ct(key, k, w=None):
        u, v, w0 = cts[k]
        if own_mode:
            ep.set_ciphertext(key, u, v, w or w0)
        else:
            ep.set_ciphertext(key, u, v, w or w0, H[k])

    others = [j for j in IDS if j != our]
    add("a", 0), add("b", 1), add("c", 2), add("d", 0)
    # a: shares before the ciphertext, one sender corrupted (another ciphertext's share)
    ep.handle_message("a", others[0], dec[(0, others[0])])
    ep.handle_message("a", others[2], dec[(1, others[2])])
    set_ct("a", 0)
    ep.handle_message("a", others[1], dec[(0, others[1])])
    # b: an invalid ciphertext (another one's w), then the valid one, then shares
    set_ct("b", 1, cts[2][2])
    set_ct("b", 1)
    ep.handle_message("b", others[0], dec[(1, others[0])])
    # c: the ciphertext now, its shares in the next flush
    set_ct("c", 2)
    # d: only an invalid ciphertext
    set_ct("d", 0, cts[1][2])
    ep.handle_message("d", others[0], dec[(0, others[0])])
    out = [_strip(ep.flush())]
    own = [{k: ep.own_share(k) for k in "abcd"}]
    ep.handle_message("b", others[1], dec[(1, others[1])])
    ep.handle_message("c", others[2], dec[(0, others[2])])  # corrupted, after the ciphertext
    ep.handle_message("c", others[0], dec[(2, others[0])])
    ep.handle_message("c", others[1], dec[(2, others[1])])
    ep.handle_message("c", 77, dec[(2, others[1])])  # not a node
    set_ct("a", 0)  # MultipleInputs
    out.append(_strip(ep.flush()))
    own.append({k: ep.own_share(k) for k in "abcd"})
    return out, own


@pytest.mark.parametrize("our", [0, 2, OBSERVER], ids=["node0", "node2", "observer"])
def test_decryption_epoch_steps_are_equal(ctx, net, our):
    want, want_own = _run_decryption(ctx, net, our, False)
    got, got_own = _run_decryption(ctx, net, our, True)
    assert got == want
    assert got_own == want_own
    flat = [s for fl in want for steps in fl.values() for s in steps]
    assert any(s[1] is not None for s in flat), "an instance terminates"
    assert any(f[1] == "UnverifiedDecryptionShareSender" for s in flat for f in s[0])
    assert any(s[2] == "InvalidCiphertext" for s in flat) and any(s[2] == "MultipleInputs" for s in flat)
    for own in got_own:
        assert own["d"] is None  # only an invalid ciphertext
    if our in IDS:
        assert got_own[0] == {"a": net["dec"][(0, our)], "b": net["dec"][(1, our)],
                              "c": net["dec"][(2, our)], "d": None}
    else:
        assert all(v is None for own in got_own for v in own.values())


def test_decryption_epoch_plaintext_mode(ctx, net):
    """plaintext=True with sk_share: the stored H feeds threshold_decrypt; the messages come back."""
    ni = P.NetInfo(IDS, 1, net["ks"], net["master"])
    ep = P.DecryptionEpoch(ctx, ni, plaintext=True, sk_share=net["sks"][1])
    for k, key in enumerate("abc"):
        ep.add(key)
        ep.set_ciphertext(key, *net["cts"][k])
        ep.handle_message(key, 3, net["dec"][(k, 3)])
    res = ep.flush()
    assert [res[key][-1]["output"] for key in "abc"] == [b"contribution a", bytes(range(90)), b"c"]


def test_decryption_epoch_needs_h_without_sk_share(ctx, net):
    ep = P.DecryptionEpoch(ctx, P.NetInfo(IDS, 0, net["ks"], net["master"]))
    ep.add("a", net["dec"][(0, 0)])
    with pytest.raises(ValueError):
        ep.set_ciphertext("a", *net["cts"][0])
    with pytest.raises(ValueError):
        P.CoinEpoch(ctx, P.NetInfo(IDS, 0, net["ks"], net["master"])).add("x", nonce=b"n")


def _run_coin(ctx, net, our, own_mode):
    ni = P.NetInfo(IDS, our, net["ks"], net["master"])
    validator = our in IDS
    sk = net["sks"][our] if validator else 1
    ep = P.CoinEpoch(ctx, ni, sk_share=sk) if own_mode else P.CoinEpoch(ctx, ni)
    sig, cH, nonces = net["sig"], net["cH"], net["nonces"]
    for k, key in enumerate("xyz"):
        if own_mode:
            ep.add(key, nonce=nonces[k])
        else:
            ep.add(key, cH[k], sig[(k, our)] if validator else None)
    others = [j for j in IDS if j != our]
    # x: shares before the input, one sender corrupted (another nonce's share)
    ep.handle_message("x", others[0], sig[(0, others[0])])
    ep.handle_message("x", others[2], sig[(1, others[2])])
    ep.handle_input("x")
    ep.handle_message("x", others[1], sig[(0, others[1])])
    # y: the input now, shares in the next flush
    ep.handle_input("y")
    # z: shares only
    ep.handle_message("z", others[0], sig[(2, others[0])])
    out = [_strip(ep.flush())]
    own = [{k: ep.own_share(k) for k in "xyz"}]
    Hs = [{k: ep.H(k) for k in "xyz"}]
    ep.handle_message("y", others[1], sig[(1, others[1])])
    ep.handle_message("y", others[2], sig[(1, others[2])])
    ep.handle_message("z", others[1], sig[(2, others[1])])
    ep.handle_input("z")
    ep.handle_input("z")
    out.append(_strip(ep.flush()))
    own.append({k: ep.own_share(k) for k in "xyz"})
    Hs.append({k: ep.H(k) for k in "xyz"})
    return out, own, Hs


@pytest.mark.parametrize("our", [0, 3, OBSERVER], ids=["node0", "node3", "observer"])
def test_coin_epoch_steps_are_equal(ctx, net, our):
    want, want_own, want_H = _run_coin(ctx, net, our, False)
    got, got_own, got_H = _run_coin(ctx, net, our, True)
    assert got == want
    assert got_own == want_own and got_H == want_H
    flat = [s for fl in want for steps in fl.values() for s in steps]
    assert sum(isinstance(s[1], (bool, np.bool_)) for s in flat) == 3, "every coin is decided"
    assert any(f[1] == "UnverifiedSignatureShareSender" for s in flat for f in s[0])
    assert got_H[0] == dict(zip("xyz", net["cH"]))
    if our in IDS:
        assert got_own[0] == {k: net["sig"][(i, our)] for i, k in enumerate("xyz")}
    else:
        assert all(v is None for own in got_own for v in own.values())
