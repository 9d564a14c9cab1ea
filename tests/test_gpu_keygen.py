"""hbtc_skg_generate on the GPU, through the C ABI: the era's commitment, our secret key share,
every public key share and the loaded key set from one call, against the Python oracle for the
small cases, against Fr arithmetic plus hbtc_g1_mul for the larger ones, and against the path
it replaces (hbtc_g1_msm with all-ones scalars, hbtc_commitment_evaluate, the Python Lagrange
interpolation, hbtc_keyset_load + hbtc_keyset_set_master).

The commitment evaluation splits the coefficients into segments of 8 (keygen.h KG_SEG): the long
commitments below have 16, 17 and 33 coefficients (whole segments, and one coefficient into the
third and into the fifth) beside 64, 65 and 129; the host test covers 8, 9 and 17."""
import ctypes
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from hbbft_amd import skg
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

pytestmark = pytest.mark.gpu
R = B.R
G1 = B.g1_compress(B.G1_GEN)
INF = bytes([0xC0]) + bytes(47)
GAPPED = [2, 5, 9]
SPARSE = [70000, (1 << 32) - 1, 3]


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def points(ctx, scalars):
    """[k] G1 for every k (0 gives the point at infinity), by the already tested hbtc_g1_mul."""
    out, st = ctx.g1_mul(G1, [k % R for k in scalars])
    assert not st.any()
    b = bytes(out)
    return [b[48 * i:48 * i + 48] for i in range(len(scalars))]


def poly_at(coeffs, x):
    return sum(c * pow(x, j, R) for j, c in enumerate(coeffs)) % R


def expected_from_scalars(ctx, row_scalars, n_nodes):
    """(commit, pk_shares) of Parts whose row0 points are [c] G1 for known c."""
    t1 = len(row_scalars[0])
    s = [sum(r[j] for r in row_scalars) % R for j in range(t1)]
    pts = points(ctx, s + [poly_at(s, i + 1) for i in range(n_nodes)])
    return pts[:t1], pts[t1:]


def sk_of(values):
    return sum(skg._lagrange_at_zero(v) for v in values) % R


def random_values(rng, n_parts, t):
    """t + 1 values per Part on a random polynomial's graph at x = 1 .. t + 1."""
    out = []
    for _ in range(n_parts):
        f = [rng.randrange(R) for _ in range(t + 1)]
        out.append([(x, poly_at(f, x)) for x in range(1, t + 2)])
    return out


# ------------------------------------------------------------------------------ small cases
def test_t0_one_part_one_node(ctx):
    c, y = 123456789, R - 5
    row0 = [points(ctx, [c])]
    commit, sk, pks, kid, st = ctx.skg_generate(0, row0, [[(1, y)]], 1)
    want = B.g1_compress(B.g1_mul(B.G1_GEN, c))
    assert st == N.ACCEPT and kid is None
    assert commit == [want] and pks == [want] and sk == y


def test_small_against_python_oracle(ctx):
    """t = 2, 3 Parts, 4 nodes, random polynomials: byte-equal to the oracle's group arithmetic."""
    rng = random.Random(1)
    t, n_parts, n = 2, 3, 4
    sc = [[rng.randrange(R) for _ in range(t + 1)] for _ in range(n_parts)]
    row0 = [points(ctx, r) for r in sc]
    values = random_values(rng, n_parts, t)
    commit, sk, pks, _, st = ctx.skg_generate(t, row0, values, n)
    assert st == N.ACCEPT
    dec = [[B.g1_decompress(p) for p in r] for r in row0]
    want_commit = []
    for j in range(t + 1):
        acc = None
        for r in dec:
            acc = B.g1_add(acc, r[j])
        want_commit.append(acc)
    assert commit == [B.g1_compress(p) for p in want_commit]
    assert pks == [B.g1_compress(TC.commitment_evaluate(want_commit, i + 1)) for i in range(n)]
    assert sk == sk_of(values)
    assert (commit, pks) == expected_from_scalars(ctx, sc, n)


@pytest.mark.parametrize("n_parts,t,n", [(3, 2, 4), (7, 5, 16)])
def test_matches_the_path_it_replaces(ctx, n_parts, t, n):
    rng = random.Random(10 * n)
    sc = [[rng.randrange(R) for _ in range(t + 1)] for _ in range(n_parts)]
    flat = points(ctx, [c for r in sc for c in r])
    row0 = [flat[p * (t + 1):(p + 1) * (t + 1)] for p in range(n_parts)]
    values = random_values(rng, n_parts, t)
    commit, sk, pks, _, st = ctx.skg_generate(t, row0, values, n)
    assert st == N.ACCEPT
    by_col = [row0[p][j] for j in range(t + 1) for p in range(n_parts)]
    old_commit, mst = ctx.g1_msm(t + 1, n_parts, by_col, [1] * len(by_col))
    assert not mst.any() and commit == old_commit
    old_pks, est = ctx.commitment_evaluate(old_commit, [i + 1 for i in range(n)])
    assert not est.any() and pks == old_pks
    assert sk == sk_of(values)


# ------------------------------------------------------------------------------ edge operands
def test_column_sum_edge_operands(ctx):
    rng = random.Random(2)
    k = rng.randrange(1, R)
    p, neg, dbl = points(ctx, [k, R - k, 2 * k])
    # columns [P, P], [P, -P], [O, P], [O, O] of two Parts
    commit, _, pks, _, st = ctx.skg_generate(3, [[p, p, INF, INF], [p, neg, p, INF]], None, 2)
    assert st == N.ACCEPT and commit == [dbl, INF, p, INF]
    s = [2 * k % R, 0, k, 0]
    assert pks == points(ctx, [poly_at(s, 1), poly_at(s, 2)])
    # every column cancels: the commitment and every share are the point at infinity
    commit, _, pks, _, st = ctx.skg_generate(1, [[p, neg], [neg, p]], None, 3)
    assert st == N.ACCEPT and commit == [INF, INF] and pks == [INF] * 3


def test_horner_edge_operands(ctx):
    rng = random.Random(3)
    k = rng.randrange(1, R)
    c, neg, dbl = points(ctx, [k, R - k, 2 * k])
    # [C, C] and [C, -C] at x = 1: the addition's doubling and its cancellation
    _, _, pks, _, st = ctx.skg_generate(1, [[c, c]], None, 2)
    assert st == N.ACCEPT and pks == points(ctx, [2 * k, 3 * k])
    assert pks[0] == dbl
    _, _, pks, _, st = ctx.skg_generate(1, [[c, neg]], None, 2)
    assert st == N.ACCEPT and pks == [INF, points(ctx, [R - k])[0]]
    # an infinity coefficient first, in the middle, last
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    for s in ([0, a, b], [a, 0, b], [a, b, 0], [0, 0, 0]):
        commit, _, pks, _, st = ctx.skg_generate(2, [points(ctx, s)], None, 3)
        assert st == N.ACCEPT
        assert (commit, pks) == expected_from_scalars(ctx, [s], 3)
        assert pks == points(ctx, [poly_at(s, x) for x in (1, 2, 3)]), s


# ------------------------------------------------------------------------------ wider shapes
def test_key_shares_past_eight_bits(ctx):
    rng = random.Random(4)
    sc = [[rng.randrange(R), rng.randrange(R)]]
    commit, _, pks, _, st = ctx.skg_generate(1, [points(ctx, sc[0])], None, 300)
    want_commit, want_pks = expected_from_scalars(ctx, sc, 300)
    assert st == N.ACCEPT and commit == want_commit and pks == want_pks


@pytest.mark.parametrize("t1", [16, 17, 33, 64, 65, 129])
def test_long_commitments(ctx, t1):
    rng = random.Random(500 + t1)
    sc = [[rng.randrange(R) for _ in range(t1)] for _ in range(2)]
    sc[0][15] = (-sc[1][15]) % R  # the last coefficient of the second segment sums to infinity
    flat = points(ctx, sc[0] + sc[1])
    commit, _, pks, _, st = ctx.skg_generate(t1 - 1, [flat[:t1], flat[t1:]], None, 3)
    want_commit, want_pks = expected_from_scalars(ctx, sc, 3)
    assert st == N.ACCEPT and commit == want_commit and pks == want_pks
    assert commit[15] == INF


def test_value_counts_and_abscissae(ctx):
    """One call whose Parts hold 0, 1, t and t + 1 values, at the gapped and the sparse abscissae,
    with the edge values taken mod r."""
    rng = random.Random(5)
    t = 3
    values = [[],
              [(SPARSE[1], (1 << 256) - 1)],
              list(zip(GAPPED, [0, R - 1, R])),
              list(zip(SPARSE + [12], [rng.randrange(1 << 256) for _ in range(4)]))]
    sc = [[rng.randrange(R) for _ in range(t + 1)] for _ in range(4)]
    flat = points(ctx, [c for r in sc for c in r])
    row0 = [flat[4 * p:4 * p + 4] for p in range(4)]
    commit, sk, pks, _, st = ctx.skg_generate(t, row0, values, 2)
    assert st == N.ACCEPT
    assert sk == sk_of([[(x, y % R) for x, y in v] for v in values])
    assert (commit, pks) == expected_from_scalars(ctx, sc, 2)


def test_interpolation_of_300_values(ctx):
    """Fr only (n_nodes = 0), t + 1 = 300: a Part of 300 values at dense x and one of 257 at sparse
    x, so lanes of the 256-lane workgroup hold a second item; row0 is the generator throughout."""
    rng = random.Random(6)
    t1 = 300
    dense = [(x, rng.randrange(R)) for x in range(1, t1 + 1)]
    xs = set(SPARSE)
    while len(xs) < 257:
        xs.add(rng.randrange(1, 1 << 32))
    sparse = [(x, rng.randrange(1 << 256)) for x in sorted(xs)]
    commit, sk, pks, kid, st = ctx.skg_generate(t1 - 1, [[G1] * t1, [G1] * t1], [dense, sparse], 0)
    assert st == N.ACCEPT and pks is None and kid is None
    assert commit == points(ctx, [2]) * t1
    assert sk == sk_of([dense, [(x, y % R) for x, y in sparse]])


# ------------------------------------------------------------------------------ statuses
def raw_generate(ctx, t, row0, off, xs, vals, n_nodes):
    """The C call itself with sentinel-filled outputs: (rc, status, keyset id, commit, pk, sk)."""
    rb = np.frombuffer(b"".join(row0), np.uint8).copy()
    off = np.asarray(off, np.uint32)
    xs = np.asarray(xs, np.uint32)
    vb = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).copy()
    commit = np.full(48 * (t + 1), 0xAA, np.uint8)
    pk = np.full(48 * n_nodes, 0xAA, np.uint8)
    sk = np.full(32, 0xAA, np.uint8)
    kid, st = ctypes.c_uint32(0xDEAD), ctypes.c_int32(-7)
    rc = ctx.lib.hbtc_skg_generate(ctx.h, len(off) - 1, t, N._ptr(rb), N._ptr(off), N._ptr(xs), N._ptr(vb),
                                   n_nodes, N._ptr(commit), N._ptr(pk), N._ptr(sk), ctypes.byref(kid),
                                   ctypes.byref(st))
    return rc, st.value, kid.value, commit, pk, sk


def test_status_cases(ctx):
    rng = random.Random(7)
    p0, p1, p2, p3 = points(ctx, [rng.randrange(1, R) for _ in range(4)])
    good = dict(t=1, row0=[p0, p1, p2, p3], off=[0, 2, 3], xs=[1, 2, 4], vals=[5, 6, 7], n_nodes=3)
    first, _ = ctx.keyset_load([p0])
    rc, st, kid, commit, pk, sk = raw_generate(ctx, **good)
    assert (rc, st) == (0, N.ACCEPT) and kid == first + 1
    assert commit.tobytes() != bytes(96) and pk.tobytes() != bytes(144)
    ctx.keyset_free(kid)
    # a row0 point that does not decode: no compression flag / not on the curve's subgroup list
    bad = bytes([p2[0] & 0x7F]) + p2[1:]
    rc, st, kid, commit, pk, sk = raw_generate(ctx, **dict(good, row0=[p0, p1, bad, p3]))
    assert (rc, st, kid) == (0, N.DECODE_ERR, 0xDEAD)
    assert not commit.any() and not pk.any() and not sk.any()
    _, mst = ctx.g1_msm(1, 1, [bad], [1])
    assert mst[0] == N.DECODE_ERR  # the same bytes are what hbtc_g1_msm rejects
    # an x repeated inside one Part (the same x in two Parts is fine: `good` has none, add one)
    rc, st, kid, commit, pk, sk = raw_generate(ctx, **dict(good, xs=[2, 2, 2]))
    assert (rc, st, kid) == (0, N.DUPLICATE_ENTRY, 0xDEAD)
    assert not commit.any() and not pk.any() and not sk.any()
    rc, st, kid, *_ = raw_generate(ctx, **dict(good, xs=[1, 2, 2]))
    assert (rc, st) == (0, N.ACCEPT)
    ctx.keyset_free(kid)
    # no key set was created by the two refused calls
    nxt, _ = ctx.keyset_load([p0])
    assert nxt == first + 3
    ctx.keyset_free(first)
    ctx.keyset_free(nxt)
    # argument errors: more than t + 1 values in a Part, x = 0, no Parts, a key set of no nodes
    assert raw_generate(ctx, **dict(good, off=[0, 3, 3]))[:3] == (-1, -7, 0xDEAD)
    assert raw_generate(ctx, **dict(good, xs=[1, 0, 4]))[:3] == (-1, -7, 0xDEAD)
    assert raw_generate(ctx, **dict(good, n_nodes=0))[0] == -1
    assert raw_generate(ctx, t=1, row0=[], off=[0], xs=[], vals=[], n_nodes=3)[0] == -1
    with pytest.raises(N.HbtcError):
        ctx.skg_generate(1, [[p0, p1]], [[(1, 1), (2, 2), (3, 3)]], 2)


def test_observer_form(ctx):
    rng = random.Random(8)
    t, n = 2, 5
    sc = [[rng.randrange(R) for _ in range(t + 1)] for _ in range(2)]
    row0 = [points(ctx, r) for r in sc]
    values = random_values(rng, 2, t)
    commit, sk, pks, _, st = ctx.skg_generate(t, row0, values, n)
    ocommit, osk, opks, _, ost = ctx.skg_generate(t, row0, None, n)
    assert st == ost == N.ACCEPT
    assert osk is None and sk == sk_of(values)
    assert (ocommit, opks) == (commit, pks) == expected_from_scalars(ctx, sc, n)


# ------------------------------------------------------------------------------ the key set
def test_generated_key_set(ctx):
    """N = 4, t = 1: the key set behind the returned id verifies like one loaded from the returned
    bytes, and the coin round needs no hbtc_keyset_set_master."""
    rng = random.Random(9)
    t, n = 1, 4
    sc = [[rng.randrange(R) for _ in range(t + 1)] for _ in range(3)]
    row0 = [points(ctx, r) for r in sc]
    commit, _, pks, kid, st = ctx.skg_generate(t, row0, None, n, load_keyset=True)
    assert st == N.ACCEPT and kid is not None
    s = [sum(r[j] for r in sc) % R for j in range(t + 1)]
    sks = [poly_at(s, i + 1) for i in range(n)]
    H = N.hash_g2(b"a coin nonce")
    sig, gst = ctx.g2_mul(H, sks[:2] + [sks[2] + 1] + sks[3:])  # node 2's share is wrong
    assert not gst.any()
    idx = np.arange(n, dtype=np.uint32)
    loaded, bad = ctx.keyset_load(pks)
    assert bad == 0
    got = ctx.verify_sig_shares(kid, [H], [n], idx, sig)
    assert list(got) == list(ctx.verify_sig_shares(loaded, [H], [n], idx, sig))
    assert list(got) == [N.ACCEPT, N.ACCEPT, N.REJECT, N.ACCEPT]
    ctx.keyset_set_master(loaded, commit[0])
    a = ctx.coin_decide(kid, [H], [n], idx, sig, t + 1)  # no keyset_set_master on kid
    b = ctx.coin_decide(loaded, [H], [n], idx, sig, t + 1)
    assert list(a[0]) == list(b[0]) and a[1] == b[1] and list(a[2]) == list(b[2])
    assert list(a[3]) == list(b[3]) == [N.ACCEPT]
    want_sig, wst = ctx.g2_mul(H, [s[0]])
    assert not wst.any() and a[1][0] == bytes(want_sig)
    ctx.keyset_free(kid)
    ctx.keyset_free(loaded)
    with pytest.raises(N.HbtcError):
        ctx.keyset_free(kid)


def test_generated_key_set_with_an_infinity_share(ctx):
    """[C, -C]: node 0's share (x = 1) is the point at infinity, in the generated key set as in
    the one loaded from the bytes."""
    rng = random.Random(11)
    k = rng.randrange(1, R)
    c, neg = points(ctx, [k, R - k])
    n = 3
    commit, _, pks, kid, st = ctx.skg_generate(1, [[c, neg]], None, n, load_keyset=True)
    assert st == N.ACCEPT and pks[0] == INF and kid is not None
    loaded, bad = ctx.keyset_load(pks)
    assert bad == 0
    H = N.hash_g2(b"another nonce")
    sks = [poly_at([k, R - k], i + 1) for i in range(n)]
    sig, gst = ctx.g2_mul(H, [sks[0], sks[1], sks[2] + 3, 77])
    assert not gst.any()
    idx = np.array([0, 1, 2, 0], dtype=np.uint32)
    got = ctx.verify_sig_shares(kid, [H], [4], idx, sig)
    assert list(got) == list(ctx.verify_sig_shares(loaded, [H], [4], idx, sig))
    assert got[1] == N.ACCEPT and got[2] == N.REJECT and got[3] == N.REJECT
    ctx.keyset_free(kid)
    ctx.keyset_free(loaded)


# ------------------------------------------------------------------------------ the protocol
@pytest.mark.parametrize("node_num", [4, 8])
def test_generate_keys_in_the_reference_scenario(ctx, node_num):
    """tests/sync_key_gen.rs:14-101 through the batch queue, then generate_keys() on every node:
    the same commitment and shares everywhere, equal to generate() + public_key_shares(), and a
    signature made with the new secret key shares verifies under the returned key set."""
    rng = random.Random(node_num)
    t = (node_num - 1) // 3
    sec = [rng.randrange(1, R) for _ in range(node_num)]
    pub = dict(enumerate(points(ctx, sec)))
    nodes, proposals = [], []
    for i in range(node_num):
        kg, part = skg.SyncKeyGen.new(ctx, i, sec[i], pub, t)
        nodes.append(kg)
        proposals.append(part)
    acks = []
    for sender_id, proposal in enumerate(proposals[:t + 1]):
        for node in nodes:
            node.handle_part(sender_id, proposal)
    for node_id, node in enumerate(nodes):
        outs = node.flush()
        assert all(o is not None and o[0] == "valid" for o in outs)
        if node_id <= 2 * t:
            acks += [(node_id, o[1]) for o in outs]
    for node in nodes:
        for sender_id, ack in acks:
            node.handle_ack(sender_id, ack)
        assert all(f == [] for f in node.flush())
        assert node.is_ready()
    results = [node.generate_keys() for node in nodes]
    commit, _, pks, _ = results[0]
    assert all(r[0] == commit and r[2] == pks and r[3] is not None for r in results)
    assert nodes[0].generate() == (commit, results[0][1])
    assert nodes[0].public_key_shares(commit) == pks
    sks = [r[1] for r in results]
    assert pks == points(ctx, sks)  # the shares are the secret key shares' public keys
    H = N.hash_g2(b"Help I'm trapped in a unit test factory")
    sig, st = ctx.g2_mul(H, sks)
    assert not st.any()
    idx = np.arange(node_num, dtype=np.uint32)
    for r in results[:2]:
        assert (ctx.verify_sig_shares(r[3], [H], [node_num], idx, sig) == N.ACCEPT).all()
    stt, out, _, cst = ctx.coin_decide(results[0][3], [H], [node_num], idx, sig, t + 1)
    assert (stt == N.ACCEPT).all() and cst[0] == N.ACCEPT
    assert (ctx.verify_sigs([commit[0]], [H], [out[0]]) == N.ACCEPT).all()
    for r in results:
        ctx.keyset_free(r[3])
    # an observer derives the same public values and no secret share
    obs = skg.SyncKeyGen(ctx, "observer", 1, pub, t)
    obs.parts = nodes[0].parts
    ocommit, osk, opks, okid = obs.generate_keys()
    assert (ocommit, osk, opks) == (commit, None, pks)
    ctx.keyset_free(okid)
