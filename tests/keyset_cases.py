"""Key sets with keys at infinity and keys that do not load, and what every consumer of a loaded
key set must decide on them; shared by tests/test_keyset_cases.py (CPU) and
tests/test_gpu_keyset_edges.py (gfx950).

The polynomial of a key set is f(X) = c * prod_{z in Z} (X - (z + 1)) * g(X) over Fr, of degree
t - 1 (t = the number of shares a combine takes, as in the C ABI), with f(0) != 0.  Node i holds
sk_i = f(i + 1) and pk_i = [sk_i] G1: for i in Z the secret is 0 and the key is the point at
infinity (C0 00 ..), a legitimate key (threshold_crypto never excludes it: SyncKeyGen::generate can
produce one).  The nodes of B, disjoint from Z, carry a g1_bad encoding of tests/golden/codec.json
instead of their key: hbtc_keyset_load counts them in n_bad and every item they send is DECODE_ERR.

A share is (idx, s): the sender and the scalar of the share over the instance's base point (the
share is [s] H for a SignatureShare, [s] u for a DecryptionShare, [s] hash_g2(msg) for a signed
message); s = 0 is the point at infinity, s = None an encoding that does not decode.  Every
expectation follows from the integers here: no library call, no oracle call.
"""
import collections
import functools
import json
import os
import random

from oracle import bls12_381 as B
from combine_cases import lagrange

R = B.R

# Statuses of include/hbtc.h (hbbft_amd/_native.py restates them too).
ACCEPT, REJECT, DECODE_ERR, UNKNOWN_SENDER, NOT_ENOUGH_SHARES, DUPLICATE_ENTRY = 0, 1, 2, 3, 5, 6

G1_INF = bytes([0xC0]) + bytes(47)
G2_INF = bytes([0xC0]) + bytes(95)
BAD_KINDS = ("no_compression_flag", "infinity_with_payload", "x_not_reduced", "not_on_curve",
             "not_in_subgroup")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec.json")) as _fh:
    _CODEC = json.load(_fh)
G1_BAD = {e["name"]: bytes.fromhex(e["enc"]) for e in _CODEC["g1_bad"]}
assert sorted(G1_BAD) == sorted(BAD_KINDS)

KeySet = collections.namedtuple("KeySet", "name N t Z B coeffs sks")
# Z: the sorted nodes whose key is at infinity; B: ((node, kind), ..) the nodes whose key does not
# load; coeffs: f, constant term first; sks[i] = f(i + 1) for every node (the B nodes' too: what
# their share would be had their key loaded).


def _rng(name):
    return random.Random("keyset_cases:" + name)


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def _poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R
    return out


@functools.lru_cache(maxsize=None)
def build(name, N, t, Z, B_):
    """The key set `name`: Z a tuple of nodes, B_ a tuple of (node, kind)."""
    Z = tuple(sorted(Z))
    assert not set(Z) & {i for i, _ in B_} and all(k in BAD_KINDS for _, k in B_)
    assert all(0 <= i < N for i in Z) and all(0 <= i < N for i, _ in B_) and len(Z) < t <= N
    rng = _rng(name)
    g = [rng.randrange(1, R) for _ in range(t - len(Z))]  # degree t - 1 - |Z|, g(0) != 0
    f = [rng.randrange(1, R)]  # c
    for z in Z:
        f = _poly_mul(f, [-(z + 1) % R, 1])
    f = _poly_mul(f, g)
    assert len(f) == t and f[-1] != 0
    sks = tuple(poly_eval(f, i + 1) for i in range(N))
    assert all((sks[i] == 0) == (i in Z) for i in range(N))  # g has no root at a node
    return KeySet(name, N, t, Z, tuple(B_), tuple(f), sks)


def small(kind=None):
    """N = 10, t = 4, keys 2 and 7 at infinity, key 5 a bad encoding of `kind` (None: no bad key,
    the same polynomial: the set hbtc_skg_generate makes from f's commitment)."""
    return build("small", 10, 4, (2, 7), ((5, kind),) if kind else ())


def large():
    """N = 80, t = 65: the smallest set on the combine routes above t = 64, a full block of 64
    keys and a ragged one; infinity at both ends and inside, one bad key of every kind at the
    second position, inside, on both sides of the block boundary and next to the last."""
    return build("large", 80, 65, (0, 37, 79), tuple(zip((1, 20, 63, 64, 78), BAD_KINDS)))


def signed():
    """N = 70 for the signed-message path: 64-signer tiles with a remainder."""
    return build("signed", 70, 24, (3, 66), ((9, "not_on_curve"), (64, "not_in_subgroup")))


def master(ks):
    return ks.coeffs[0]


def bad_nodes(ks):
    return tuple(i for i, _ in ks.B)


def ordinary(ks):
    return [i for i in range(ks.N) if i not in ks.Z and i not in bad_nodes(ks)]


def key_bytes(ks, good):
    """The N key encodings: good[i] (= [sk_i] G1 compressed, from any source) for an ordinary node,
    C0 00.. for a node of Z, the codec fixture's bad encoding for a node of B."""
    out = [bytes(k) for k in good]
    assert len(out) == ks.N
    for z in ks.Z:
        out[z] = G1_INF
    for i, kind in ks.B:
        out[i] = G1_BAD[kind]
    return out


# ---------------------------------------------------------------------------------- expectations
def item_status(ks, idx, s):
    """The status of share (idx, s), in the order of the rules."""
    if idx >= ks.N:
        return UNKNOWN_SENDER
    if idx in bad_nodes(ks):  # whatever s is: a valid share, the one at infinity, a broken one
        return DECODE_ERR
    if s is None:
        return DECODE_ERR
    if idx in ks.Z:  # e(O, H) == e(G1, s): only the share at infinity passes
        return ACCEPT if s % R == 0 else REJECT
    return ACCEPT if s % R == ks.sks[idx] else REJECT  # s = O under an ordinary key: REJECT


def statuses(ks, inst):
    return [item_status(ks, i, s) for i, s in inst]


def combine(ks, inst, t=None):
    """(status, k): the first t ACCEPTed items in item order interpolated at 0 over x = idx + 1
    with integer Lagrange coefficients; the combined point is [k] base.  k is None on a failure."""
    t = ks.t if t is None else t
    sel = [(i, s) for i, s in inst if item_status(ks, i, s) == ACCEPT][:t]
    if len(sel) < t:
        return NOT_ENOUGH_SHARES, None
    xs = [i + 1 for i, _ in sel]
    if len(set(xs)) < t:
        return DUPLICATE_ENTRY, None
    return ACCEPT, sum(l * s for l, (_, s) in zip(lagrange(xs), sel)) % R


# ------------------------------------------------------------------------------------ share batch
def _wrong(ks, i, rng):
    return (i, (ks.sks[i] + rng.randrange(1, R)) % R)


def share_batch(ks, trio=None, tile=64):
    """Instances A, B and C of the share checks (SignatureShares and DecryptionShares alike).

    A  one tile of up to `tile` items, then a ragged one of 6.  The first holds ordinary senders
       with valid shares, one of them wrong; sender `trio` (default: the set's first bad key)
       three times, with the share it would owe, the share at infinity and a broken encoding; every
       other bad key once; and idx = N.  The ragged tile holds only senders of Z: all at infinity
       but one valid non-zero point, so the tile's G1 side sums to infinity and its G2 side does
       not; the later copy of every sender goes to the exact leaf check.
    B  8 items, all from senders of Z at infinity: both sums are the identity.
    C  a tile in which one sender of Z appears twice, both at infinity, among ordinary senders."""
    rng = _rng("share_batch:%s:%s" % (ks.name, trio))
    bad, ords, Z = list(bad_nodes(ks)), ordinary(ks), list(ks.Z)
    trio = bad[0] if trio is None else trio
    ords = [i for i in ords if i != trio]
    special = [(trio, ks.sks[trio]), (trio, 0), (trio, None), (ks.N, rng.randrange(1, R))]
    special += [(i, ks.sks[i]) for i in bad if i != trio]
    senders = rng.sample(ords, min(len(ords), tile - len(special)))
    first = [(i, ks.sks[i]) for i in senders]
    first[len(first) // 2] = _wrong(ks, first[len(first) // 2][0], rng)
    first += special
    rng.shuffle(first)
    ragged = [(z, 0) for z in Z]
    ragged[1] = (Z[1], rng.randrange(1, R))
    while len(ragged) < 6:
        ragged.append((Z[len(ragged) % len(Z)], 0))
    A = tuple(first + ragged)
    Bi = tuple((Z[j % len(Z)], 0) for j in range(8))
    c = [(i, ks.sks[i]) for i in rng.sample(ords, min(len(ords), tile - 2))]
    c.insert(len(c) // 12, (Z[1], 0))
    c.insert(2 * len(c) // 3, (Z[1], 0))
    return collections.OrderedDict((("A", A), ("B", Bi), ("C", tuple(c))))


# ------------------------------------------------------------------------------------ coin rounds
def coin_small(ks):
    """The coin instances of a small set, named by their first t + 1 items (t = 4):
    i    all ACCEPTed, a Z sender's share at infinity among the first t;
    ii   one item from the bad key: the leave-one-out subset without it is committed;
    iii  the bad key's item and a wrong share: recombined from the statuses;
    iv   a Z sender's non-zero share (REJECT), enough others;
    v    the bad key and lying Z senders use the items up: NOT_ENOUGH_SHARES.
    ii, iii and v need a bad key and are left out of a set without one."""
    rng = _rng("coin_small:" + ks.name)
    z0, z1 = ks.Z
    o = [i for i in range(ks.N) if i not in ks.Z and i != 5]
    v = lambda i: (i, ks.sks[i])
    out = collections.OrderedDict()
    out["i"] = (v(o[0]), (z0, 0), v(o[1]), v(o[2]), v(o[3]), v(o[4]), (z1, 0), v(o[5]))
    if ks.B:
        b = bad_nodes(ks)[0]
        assert b == 5
        out["ii"] = (v(o[0]), v(b), (z0, 0), v(o[1]), v(o[2]), v(o[3]), v(o[6]))
        out["iii"] = (v(b), v(o[0]), _wrong(ks, o[1], rng), (z0, 0), v(o[2]), v(o[3]), v(o[4]))
    out["iv"] = ((z1, rng.randrange(1, R)), v(o[0]), v(o[1]), (z0, 0), v(o[2]), v(o[3]))
    if ks.B:
        out["v"] = (v(b), (z0, rng.randrange(1, R)), (z1, rng.randrange(1, R)), v(o[0]), v(o[1]),
                    (b, 0), v(o[2]))
    return out


def coin_large(ks):
    """Two instances at t = 65.  "all_z": the three Z senders at infinity, every bad key and one
    wrong share come before the 65th ACCEPTed item, so the selection holds all of Z and steps
    over the rest.  "short": 3 Z senders and 61 ordinary ones ACCEPTed, 64 in all."""
    rng = _rng("coin_large:" + ks.name)
    ords, bad, Z = ordinary(ks), list(bad_nodes(ks)), list(ks.Z)
    v = lambda i: (i, ks.sks[i])
    head = [(Z[2], 0), v(bad[0]), (Z[0], 0), _wrong(ks, ords[0], rng), (Z[1], 0)]
    head += [v(i) for i in bad[1:]]
    all_z = head + [v(i) for i in ords[1:]]
    short = [v(i) for i in ords[:61]] + [_wrong(ks, i, rng) for i in ords[61:]]
    short += [(z, 0) for z in Z] + [v(i) for i in bad]
    rng.shuffle(short)
    return collections.OrderedDict((("all_z", tuple(all_z)), ("short", tuple(short))))


# -------------------------------------------------------------------------------- signed messages
def signed_items(ks):
    """[(signer, s, message length)] for hbtc_verify_signed_msgs: every signer a run of 1 to 3
    items over messages of 9 and 136 bytes.  The first Z signer's items are all the signature at
    infinity; the second has one non-zero signature (another signer's) among them; the bad keys'
    signatures are the ones they would owe; one ordinary signature is another signer's; one item
    is a stranger's (signer = N).  In a seeded order."""
    rng = _rng("signed:" + ks.name)
    z0, z1 = ks.Z
    items = []
    for j in range(ks.N):
        n = 3 if j in ks.Z or j == bad_nodes(ks)[1] else 2 if j == bad_nodes(ks)[0] else 1 + j % 3
        run = [[j, ks.sks[j]] for _ in range(n)]
        if j == z1:
            run[1][1] = ks.sks[0]
        if j == 40:
            run[0][1] = ks.sks[41]
        items += run
    items.append([ks.N, ks.sks[0]])
    rng.shuffle(items)
    return [(j, s, (9, 136)[p % 2]) for p, (j, s) in enumerate(items)]
