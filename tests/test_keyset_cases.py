"""The key-set construction of tests/keyset_cases.py against the oracle: the status rule of a key
at infinity against the two pairing equations of threshold_crypto, and the builder's claims about
its own sets and batches as conditions.  No GPU and no library."""
import itertools
import random

import pytest

import keyset_cases as KC
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

R = B.R
SETS = [KC.small(k) for k in KC.BAD_KINDS] + [KC.small(), KC.large(), KC.signed()]
SET_IDS = ["small_" + k for k in KC.BAD_KINDS] + ["small_pure", "large", "signed"]


def test_infinity_rule_equals_the_pairing_equations():
    """Rules 4 and 5 against e(pk, H) == e(G1, sig) (PublicKeyShare::verify) and e(share, H) ==
    e(pk, w) (verify_decryption_share), once per class: twelve oracle pairings.  pk = [sk] G1,
    H = [h] G2, w = [r h] G2 (u = [r] G1); a SignatureShare is [s h] G2, a DecryptionShare [s r] G1."""
    rng = random.Random(4)
    ks = KC.small()
    h, r = rng.randrange(1, R), rng.randrange(1, R)
    H = B.g2_mul(B.G2_GEN, h)
    w = B.g2_mul(B.G2_GEN, r * h % R)
    z, o = ks.Z[0], KC.ordinary(ks)[0]
    classes = [(z, 0, KC.ACCEPT),                     # infinity key, infinity share
               (z, rng.randrange(1, R), KC.REJECT),   # infinity key, a valid non-zero point
               (o, 0, KC.REJECT)]                     # ordinary key, infinity share
    for idx, s, want in classes:
        pk = B.g1_mul(B.G1_GEN, ks.sks[idx]) if ks.sks[idx] else None
        assert (pk is None) == (idx in ks.Z)
        sig = B.g2_mul(B.G2_GEN, s * h % R) if s else None
        share = B.g1_mul(B.G1_GEN, s * r % R) if s else None
        assert (B.pairing(pk, H) == B.pairing(B.G1_GEN, sig)) == (want == KC.ACCEPT), (idx, s)
        assert (B.pairing(share, H) == B.pairing(pk, w)) == (want == KC.ACCEPT), (idx, s)
        assert KC.item_status(ks, idx, s) == want


@pytest.mark.parametrize("ks", SETS, ids=SET_IDS)
def test_polynomial(ks):
    assert len(ks.coeffs) == ks.t and ks.coeffs[-1] != 0  # degree t - 1
    assert [i for i in range(ks.N) if ks.sks[i] == 0] == list(ks.Z)
    assert all(KC.poly_eval(ks.coeffs, z + 1) == 0 for z in ks.Z)
    assert KC.master(ks) == KC.poly_eval(ks.coeffs, 0) != 0
    assert not set(ks.Z) & set(KC.bad_nodes(ks))
    assert len(KC.ordinary(ks)) == ks.N - len(ks.Z) - len(ks.B)


def test_the_sets_are_the_ones_asked_for():
    s, l, g = KC.small("not_on_curve"), KC.large(), KC.signed()
    assert (s.N, s.t, s.Z, s.B) == (10, 4, (2, 7), ((5, "not_on_curve"),))
    assert (l.N, l.t, l.Z) == (80, 65, (0, 37, 79))
    assert l.B == tuple(zip((1, 20, 63, 64, 78), KC.BAD_KINDS))
    assert (g.N, g.Z, KC.bad_nodes(g)) == (70, (3, 66), (9, 64))
    assert KC.small().coeffs == s.coeffs and KC.small().B == ()  # the same f with and without B


@pytest.mark.parametrize("ks", SETS, ids=SET_IDS)
def test_any_t_nodes_interpolate_to_f0(ks):
    """The integer interpolation of t nodes' secrets gives f(0): the first t, the last t, t that
    hold all of Z, and seeded selections in shuffled order."""
    rng = random.Random(ks.name)
    rest = [i for i in range(ks.N) if i not in ks.Z]
    sels = [list(range(ks.t)), list(range(ks.N - ks.t, ks.N)), list(ks.Z) + rest[:ks.t - len(ks.Z)]]
    sels += [rng.sample(range(ks.N), ks.t) for _ in range(4)]
    pure = ks._replace(B=())  # the secrets of the B nodes are on the polynomial too
    for n, sel in enumerate(sels):
        inst = [(i, ks.sks[i]) for i in sel]
        assert KC.combine(pure, inst) == (KC.ACCEPT, KC.master(ks)), sel
        if n in (2, 3):  # the oracle's coefficients (an inversion per pair of x) on two of them
            lam = TC.lagrange_at_zero([i + 1 for i in sel])
            assert sum(l * ks.sks[i] for l, i in zip(lam, sel)) % R == KC.master(ks)
    assert KC.combine(pure, [(i, ks.sks[i]) for i in range(ks.t - 1)]) == (KC.NOT_ENOUGH_SHARES, None)


def test_bad_encodings_do_not_decode():
    for kind in KC.BAD_KINDS:
        with pytest.raises(B.DecodeError):
            B.g1_decompress(KC.G1_BAD[kind])
    assert B.g1_decompress(KC.G1_INF) is None and B.g2_decompress(KC.G2_INF) is None


def test_key_bytes():
    ks = KC.small("x_not_reduced")
    good = [B.g1_compress(B.g1_mul(B.G1_GEN, sk)) if sk else KC.G1_INF for sk in ks.sks]
    keys = KC.key_bytes(ks, good)
    assert [keys[z] for z in ks.Z] == [KC.G1_INF] * 2 and keys[5] == KC.G1_BAD["x_not_reduced"]
    for i in KC.ordinary(ks):
        assert B.g1_decompress(keys[i]) == B.g1_mul(B.G1_GEN, ks.sks[i])
    assert B.g1_compress(None) == KC.G1_INF  # what [0] G1 encodes to


# ---------------------------------------------------------------------------------- the batches
def _count(st, code):
    return sum(1 for s in st if s == code)


def test_share_batch_large():
    ks = KC.large()
    bt = KC.share_batch(ks)
    assert [len(v) for v in bt.values()] == [70, 8, 64]
    A, st = bt["A"], KC.statuses(ks, bt["A"])
    # the full tile: the trio and the four other bad keys DECODE_ERR, one wrong share, one stranger
    assert _count(st[:64], KC.DECODE_ERR) == 7 and _count(st[:64], KC.REJECT) == 1
    assert _count(st[:64], KC.UNKNOWN_SENDER) == 1 and _count(st[:64], KC.ACCEPT) == 55
    trio = sorted((s is None, s or 0) for i, s in A[:64] if i == 1)
    assert trio == [(False, 0), (False, ks.sks[1]), (True, 0)]
    assert not any(i in ks.Z for i, _ in A[:64])
    # the ragged tile: Z only, one liar, later copies of every sender
    assert all(i in ks.Z for i, _ in A[64:]) and st[64:] == [0, 1, 0, 0, 0, 0]
    assert [i for i, _ in A[64:]] == [0, 37, 79, 0, 37, 79] and A[65][1] != 0
    assert all(i in ks.Z and s == 0 for i, s in bt["B"]) and KC.statuses(ks, bt["B"]) == [0] * 8
    C = bt["C"]
    assert KC.statuses(ks, C) == [0] * 64 and sorted(i for i, s in C if s == 0) == [37, 37]
    assert len({i for i, _ in C}) == 63


@pytest.mark.parametrize("kind", [None] + list(KC.BAD_KINDS))
def test_share_batch_small(kind):
    ks = KC.small(kind)
    bt = KC.share_batch(ks, trio=5)
    st = KC.statuses(ks, bt["A"])
    assert len(bt["A"]) == 7 + 4 + 6 and _count(st, KC.UNKNOWN_SENDER) == 1
    # without a bad key sender 5 is an ordinary one: its own share, O (REJECT), a broken encoding
    assert _count(st, KC.DECODE_ERR) == (3 if kind else 1)
    assert _count(st, KC.REJECT) == (2 if kind else 3)
    assert KC.statuses(ks, bt["B"]) == [0] * 8 and KC.statuses(ks, bt["C"]) == [0] * len(bt["C"])


@pytest.mark.parametrize("kind", KC.BAD_KINDS)
def test_coin_small_sits_where_its_name_says(kind):
    ks = KC.small(kind)
    t, insts = ks.t, KC.coin_small(ks)
    assert list(insts) == ["i", "ii", "iii", "iv", "v"]
    head = {k: KC.statuses(ks, v)[:t + 1] for k, v in insts.items()}
    assert head["i"] == [0] * 5 and (2, 0) in insts["i"][:t]
    assert head["ii"] == [0, KC.DECODE_ERR, 0, 0, 0] and (2, 0) in insts["ii"][:t + 1]
    assert head["iii"] == [KC.DECODE_ERR, 0, KC.REJECT, 0, 0]
    assert head["iv"] == [KC.REJECT, 0, 0, 0, 0] and insts["iv"][0][0] == 7
    for k in ("i", "ii", "iii", "iv"):
        st, key = KC.combine(ks, insts[k])
        assert (st, key) == (KC.ACCEPT, KC.master(ks)), k
        sel = [i for i, s in insts[k] if KC.item_status(ks, i, s) == 0][:t]
        assert set(sel) & set(ks.Z), k  # an infinity share is part of every selection
    assert _count(KC.statuses(ks, insts["v"]), KC.ACCEPT) == t - 1
    assert KC.combine(ks, insts["v"]) == (KC.NOT_ENOUGH_SHARES, None)
    # every instance fits 55 of them into one call above the speculation's limit
    assert 5 * (t + 1) <= 256 < 55 * (t + 1)
    assert list(KC.coin_small(KC.small())) == ["i", "iv"]


def test_coin_large_sits_where_its_name_says():
    ks = KC.large()
    insts = KC.coin_large(ks)
    a, st = insts["all_z"], KC.statuses(ks, insts["all_z"])
    assert len(a) == 80 and sorted(i for i, _ in a) == list(range(80))
    pos = [p for p, s in enumerate(st) if s == KC.ACCEPT]
    last = pos[ks.t - 1]  # everything unusual sits in front of the 65th ACCEPTed item
    assert {a[p][0] for p in pos[:ks.t]} >= set(ks.Z)
    assert _count(st[:last], KC.DECODE_ERR) == 5 and _count(st[:last], KC.REJECT) == 1
    assert KC.combine(ks, a) == (KC.ACCEPT, KC.master(ks))
    assert _count(KC.statuses(ks, insts["short"]), KC.ACCEPT) == 64
    assert KC.combine(ks, insts["short"]) == (KC.NOT_ENOUGH_SHARES, None)


def test_signed_items():
    ks = KC.signed()
    items = KC.signed_items(ks)
    runs = {j: [(s, n) for i, s, n in items if i == j] for j in range(ks.N + 1)}
    assert all(1 <= len(runs[j]) <= 3 for j in runs) and len(items) < 256
    assert {n for _, _, n in items} == {9, 136}
    st = {j: [KC.item_status(ks, j, s) for s, _ in runs[j]] for j in runs}
    assert st[3] == [0, 0, 0] and sorted(st[66]) == [0, 0, 1]
    assert st[9] == [KC.DECODE_ERR] * 2 and st[64] == [KC.DECODE_ERR] * 3
    assert st[70] == [KC.UNKNOWN_SENDER] and KC.REJECT in st[40]
    flat = list(itertools.chain.from_iterable(st.values()))
    assert _count(flat, KC.REJECT) == 2 and _count(flat, KC.DECODE_ERR) == 5
