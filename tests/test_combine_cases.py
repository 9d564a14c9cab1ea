"""The combine case tables and their reference (tests/combine_cases.py) against the oracle's
restatement of threshold_crypto (oracle/threshold_crypto.py), and the coverage of the tables as a
condition: every case must sit on the route and give the status its place in the table claims.
No GPU and no library."""
import pytest

import combine_cases as CC
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

R = B.R
A, NES, DUP, DEC = CC.ACCEPT, CC.NOT_ENOUGH_SHARES, CC.DUPLICATE_ENTRY, CC.DECODE_ERR


def _ids(cases):
    return [c.name for c in cases]


ALL = CC.all_cases()
SMALL_T = [c for c in ALL if c.t <= 257]


def test_case_names_are_unique():
    assert len(set(_ids(ALL))) == len(ALL)


@pytest.mark.parametrize("case", SMALL_T, ids=_ids(SMALL_T))
def test_lambda_equals_oracle(case):
    ref = CC.reference(case)
    if ref.status != A:
        assert ref.lam is None
        return
    assert ref.lam == TC.lagrange_at_zero(ref.xs)


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_lambda_sums_to_one(case):
    ref = CC.reference(case)
    if ref.status == A:
        assert len(ref.lam) == case.t and sum(ref.lam) % R == 1
        assert all(0 < l < R for l in ref.lam)


def _small(name, t, idx, verified=False, statuses=None):
    rng = CC._rng(name)
    st = statuses or [A] * len(idx)
    return CC.Case(name, t, tuple((i, s, rng.randrange(1, R)) for i, s in zip(idx, st)), verified,
                   None, None)


@pytest.mark.parametrize("group", [1, 2])
def test_reference_equals_interpolate(group):
    """Statuses and points of the reference equal threshold_crypto's interpolate on three small
    instances (and a fourth for the order of the two errors): interpolate raises where the reference
    names a status."""
    gen, mul, comp = (B.G1_GEN, B.g1_mul, B.g1_compress) if group == 1 else \
        (B.G2_GEN, B.g2_mul, B.g2_compress)

    def items(case):
        return [(i, mul(gen, s)) for i, _, s in CC.select(case)]

    ok = _small("tc_ok", 4, [9, 2, 2 ** 32 - 1, 0, 5])
    got, par, st = CC.expected(ok, group)
    p = TC.interpolate(4, items(ok), group)
    assert st == A and got == comp(p)
    if group == 2:
        assert par == int(TC.signature_parity(p))
    # the verified form hands interpolate the accepted shares only
    ver = _small("tc_ver", 3, [4, 4, 7, 1, 8], True, [CC.REJECT, A, A, CC.DECODE_ERR, A])
    assert [i for i, _, _ in CC.select(ver)] == [4, 7, 8]
    assert CC.expected(ver, group)[0] == comp(TC.interpolate(3, items(ver), group))
    size = 48 if group == 1 else 96
    for case, status, err in ((_small("tc_dup", 4, [3, 1, 6, 3, 8]), DUP, "DuplicateEntry"),
                              (_small("tc_short", 4, [3, 1, 6]), NES, "NotEnoughShares"),
                              (_small("tc_short_dup", 4, [3, 1, 3]), NES, "NotEnoughShares")):
        assert CC.expected(case, group) == (bytes(size), 0, status)
        with pytest.raises(TC.CryptoError, match=err):
            TC.interpolate(4, items(case), group)


# --------------------------------------------------------------------------------------- coverage
# The table of the index cases: name -> (route with the factorial tables on, status).
INDEX_TABLE = {
    "dense": ("fact", A),
    "first_x_2": ("fact", A),
    "gaps256_block": ("fact", A),
    "gaps256_scattered": ("fact", A),
    "gaps257_scattered": ("generic", A),
    "gaps257_front": ("generic", A),
    "large": ("generic", A),
    "decreasing": ("generic", A),
    "swap": ("generic", A),
    "shuffle": ("generic", A),
    "dup_adjacent": (None, DUP),
    "dup_first_last": (None, DUP),
    "dup_past_t": (None, A),
    "short_dup": (None, NES),
}


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_case_route_and_status_as_declared(case):
    assert CC.route_of(case) == case.route
    assert CC.reference(case).status == case.status


def _xs(case):
    return [i + 1 for i, _, _ in CC.select(case)]


def test_index_cases_cover_the_table():
    cases = {c.name[len("idx_"):]: c for c in CC.index_cases()}
    assert set(cases) == set(INDEX_TABLE) and len(CC.index_cases()) == len(INDEX_TABLE)
    for name, (route, status) in INDEX_TABLE.items():
        c = cases[name]
        assert c.t == CC.T_IDX == 70 > CC.COMB_SMALL_T and not c.verified
        assert CC.reference(c).status == status, name
        if route is not None:
            assert CC.route_of(c) == route, name
    t = CC.T_IDX
    xs = {n: _xs(c) for n, c in cases.items()}
    assert xs["dense"] == list(range(1, t + 1)) and xs["first_x_2"] == list(range(2, t + 2))
    for n in ("gaps256_block", "gaps256_scattered"):
        assert xs[n] == sorted(set(xs[n])) and xs[n][-1] - t == 256 == CC.LG_FACT_RMAX
    assert xs["gaps256_block"][:-1] == list(range(1, t))  # one block before the last x
    scat = xs["gaps256_scattered"]
    assert len({b - a for a, b in zip([0] + scat, scat)}) > 2  # gaps in several places
    for n in ("gaps257_scattered", "gaps257_front"):
        assert xs[n] == sorted(set(xs[n])) and xs[n][-1] - t == 257
    assert xs["gaps257_front"][0] == 258
    assert xs["large"] == sorted(set(xs["large"]))
    assert {65535, 65536, 10 ** 6 + 1, 2 ** 32 - 1, 2 ** 32} < set(xs["large"]) and 1 in xs["large"]
    assert xs["decreasing"] == list(range(t, 0, -1))
    sw = [p for p in range(t) if xs["swap"][p] != p + 1]
    assert len(sw) == 2 and sw[1] == sw[0] + 1 and sorted(xs["swap"]) == xs["dense"]
    assert sorted(xs["shuffle"]) == xs["dense"] and xs["shuffle"] != xs["dense"]
    d = xs["dup_adjacent"]
    assert [p for p in range(t - 1) if d[p] == d[p + 1]] and len(set(d)) == t - 1
    d = xs["dup_first_last"]
    assert d[0] == d[-1] and len(set(d)) == t - 1
    c = cases["dup_past_t"]
    assert c.items[t][0] in [i for i, _, _ in c.items[:t]] and len(set(_xs(c))) == t
    c = cases["short_dup"]
    assert len(c.items) == t - 1 and len(set(_xs(c))) < t - 1
    for n in CC.BOUNDARY_NAMES:
        assert n in cases


def test_chunk_cases_cover_chunks_1_to_4():
    cs = CC.chunk_cases()
    assert tuple(cs) == (65, 255, 256, 257, 511, 512, 513, 769)
    assert {CC.inv_chunk(t) for t in cs} == {1, 2, 3, 4}
    ragged = empty = 0
    mixed = set()
    for t, group in cs.items():
        sparse = group[0]
        xs = _xs(sparse)
        assert sparse.t == t and xs == sorted(set(xs))
        assert xs[-1] - t > CC.LG_FACT_RMAX and CC.route_of(sparse) == "generic"
        for dense in group[1:]:
            assert dense.t == t and CC.route_of(dense) == "fact"
            mixed.add(CC.inv_chunk(t))
        ch = CC.inv_chunk(t)
        ragged += t % ch != 0                    # a thread with a short chunk
        empty += -(-t // ch) < CC.LG_BS          # threads with no term at all
    assert ragged >= 3 and empty >= 3 and mixed == {1, 2, 3, 4}


def test_limit_cases_sit_at_the_t_switch():
    lo, hi = CC.limit_cases()
    assert lo.t == CC.LG_FACT_TMAX == 4096 and hi.t == 4097
    xs = _xs(lo)
    assert xs == sorted(set(xs)) and xs[-1] == 4352 and xs[-1] - lo.t == CC.LG_FACT_RMAX
    assert lo.route == CC.route_of(lo) == "fact"
    assert _xs(hi) == list(range(1, 4098)) and hi.route == CC.route_of(hi) == "generic"
    assert CC.inv_chunk(hi.t) == 17


def test_selection_cases_cover_the_ballot_edges():
    cs = {c.name: c for c in CC.selection_cases()}
    t = CC.T_IDX
    ver = [c for c in cs.values() if c.verified]
    assert all(c.t == t for c in cs.values())
    assert {len(c.items) for c in ver} >= {64, 65, 128, 129, 200}
    assert {CC.tth_position(c) for c in ver} >= {127, 128}
    used = {st for c in ver for _, st, _ in c.items}
    assert used == {A, CC.REJECT, DEC}
    c = cs["sel_first64_rejected"]
    assert all(st != A for _, st, _ in c.items[:CC.BALLOT]) and CC.reference(c).status == A
    c = cs["sel_exact_last"]
    assert [st for _, st, _ in c.items].count(A) == t and CC.tth_position(c) == len(c.items) - 1
    c = cs["sel_t_minus_1"]
    assert [st for _, st, _ in c.items].count(A) == t - 1 and CC.reference(c).status == NES
    c = cs["sel_dup_first_rejected"]
    idx = [i for i, _, _ in c.items]
    rep = [i for i in set(idx) if idx.count(i) == 2]
    assert len(rep) == 1 and c.items[idx.index(rep[0])][1] == CC.REJECT
    assert rep[0] + 1 in _xs(c) and CC.reference(c).status == A
    c = cs["sel_bad_around"]
    bad = [p for p, (_, _, s) in enumerate(c.items) if s is None]
    first = min(p for p, (_, st, _) in enumerate(c.items) if st == A)
    assert len(bad) == 2 and bad[0] < first and bad[1] > CC.tth_position(c)
    assert all(c.items[p][1] != A for p in bad) and CC.reference(c).status == A
    c = cs["sel_bad_selected_plain"]
    assert not c.verified and any(s is None for _, _, s in CC.select(c))
    assert CC.reference(c).status == DEC
    # ACCEPT is trusted by the combine: such a share is always a valid point
    for c in CC.all_cases():
        if c.verified:
            assert all(s is not None for _, st, s in c.items if st == A)


def test_small_cases_cover_both_ends():
    sm = CC.small_cases()
    assert tuple(sm) == (8, 64) and max(sm) == CC.COMB_SMALL_T
    for t, cases in sm.items():
        cs = {c.name[len("small%d_" % t):]: c for c in cases}
        assert all(c.t == t for c in cases)
        for n in CC.SMALL_INDEX_NAMES:
            route, status = INDEX_TABLE[n]
            assert CC.reference(cs[n]).status == status
            if route is not None:
                assert CC.route_of(cs[n]) == route
        assert 2 ** 32 in _xs(cs["large"])
        ver = [c for c in cases if c.verified]
        assert {len(c.items) for c in ver} >= {64, 65, 129}
        assert {CC.tth_position(c) for c in ver} >= {63, 64, 128}
        assert all(st != A for _, st, _ in cs["sel_n129_tth128"].items[:CC.BALLOT])
        assert CC.reference(cs["sel_t_minus_1"]).status == NES
        assert CC.reference(cs["sel_dup_first_rejected"]).status == A
