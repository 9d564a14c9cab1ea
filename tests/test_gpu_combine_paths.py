"""GPU parity of every route of the Lagrange combines (hbtc_combine_dec / hbtc_combine_sigs and
their _verified_dev forms) against the Python-integer reference of tests/combine_cases.py: the small
combine (hbtc_comb.hip), k_select, the factorial tables (k_lagrange_fact) and the generic
k_lagrange_x / _den / _inv (hbtc_msm.hip), on both sides of every switch between them (M - t = 256 /
257, t = 4096 / 4097, t = 64 / 65), with unsorted, wrapping (idx = 2^32 - 1) and repeated indices,
k_lagrange_inv at 1 to 4 (and 17) terms per thread, and selections that end on a ballot boundary.
The shares are [s_i] G for independent random s_i, so one wrong coefficient moves the result.
Bar: byte-identical points, parity bits and instance statuses; the settings agree with each other.
"""
import json
import os

import pytest

import combine_cases as CC
from hbbft_amd import _native as N
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_KEYS = ("HBTC_LAGRANGE_FACT", "HBTC_COMB_SMALL")
SETTINGS = {
    "default": {},
    "fact1": {"HBTC_LAGRANGE_FACT": "1"},
    "fact0": {"HBTC_LAGRANGE_FACT": "0"},
    "nosmall": {"HBTC_COMB_SMALL": "0"},
}


def _open(env):
    """A fresh context under exactly these settings (a context reads them when it is created)."""
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env)
    try:
        return N.Context(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    """One context per setting.  No verification call ever runs on them: the combine reuses the
    decoded shares of the last verification by pointer identity, and a recycled allocation of these
    tests must not match one."""
    cs = {name: _open(env) for name, env in SETTINGS.items()}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def shares():
    """{case name: (G1 shares, G2 shares)}: [s] G of every item, made once with hbtc_g1_mul /
    hbtc_g2_mul; an undecodable encoding of tests/golden/codec.json where s is None.  The two
    t-limit cases are G1 only."""
    with open(os.path.join(HERE, "golden", "codec.json")) as fh:
        codec = json.load(fh)
    bad = {1: [bytes.fromhex(x["enc"]) for x in codec["g1_bad"]],
           2: [bytes.fromhex(x["enc"]) for x in codec["g2_bad"]]}
    gen = {1: B.g1_compress(B.G1_GEN), 2: B.g2_compress(B.G2_GEN)}
    limit = {c.name for c in CC.limit_cases()}
    cases = CC.all_cases()
    out = {c.name: [None, None] for c in cases}
    ctx = N.Context(0)
    try:
        for group, size in ((1, 48), (2, 96)):
            use = [c for c in cases if group == 1 or c.name not in limit]
            sc = [s or 1 for c in use for _, _, s in c.items]
            buf, st = (ctx.g1_mul if group == 1 else ctx.g2_mul)(gen[group], sc)
            assert not st.any()
            buf, pos = bytes(buf), 0
            for c in use:
                pts = []
                for j, (_, _, s) in enumerate(c.items):
                    pts.append(buf[size * pos:size * (pos + 1)] if s is not None
                               else bad[group][j % len(bad[group])])
                    pos += 1
                out[c.name][group - 1] = pts
    finally:
        ctx.close()
    return out


def _combine(ctx, group, cases, shares):
    """One call over the instances `cases` (one t, one form): [(point, parity, status)]."""
    t, verified = cases[0].t, cases[0].verified
    assert len(cases) <= 16 and all(c.t == t and c.verified == verified for c in cases)
    counts = [len(c.items) for c in cases]
    idx = [i for c in cases for i, _, _ in c.items]
    pts = [p for c in cases for p in shares[c.name][group - 1]]
    if verified:
        st = [s for c in cases for _, s, _ in c.items]
        if group == 1:
            out, cst = ctx.combine_dec_verified(counts, idx, pts, st, t)
            par = [0] * len(cases)
        else:
            out, par, cst = ctx.combine_sigs_verified(counts, idx, pts, st, t)
    elif group == 1:
        out, cst = ctx.combine_dec(counts, idx, pts, t)
        par = [0] * len(cases)
    else:
        out, par, cst = ctx.combine_sigs(counts, idx, pts, t)
    return [(o, int(p), int(s)) for o, p, s in zip(out, par, cst)]


def _check(ctxs, settings, group, cases, shares):
    """The call under every one of `settings` equals the reference, instance by instance (so the
    settings agree with each other as well)."""
    want = [CC.expected(c, group) for c in cases]
    for name in settings:
        got = _combine(ctxs[name], group, list(cases), shares)
        for c, g, w in zip(cases, got, want):
            assert g == w, (name, c.name, N.STATUS_NAMES.get(g[2]), N.STATUS_NAMES.get(w[2]))


FACT = ("fact1", "fact0")


@pytest.mark.parametrize("group", [1, 2])
def test_index_cases_in_one_call(ctxs, shares, group):
    """All index cases at t = 70 side by side: factorial and generic instances share done[]."""
    _check(ctxs, FACT, group, CC.index_cases(), shares)


@pytest.mark.parametrize("group", [1, 2])
def test_route_boundary_cases_alone(ctxs, shares, group):
    """256 / 257 gaps, dense and decreasing, one instance per call."""
    cases = {c.name[len("idx_"):]: c for c in CC.index_cases()}
    for name in CC.BOUNDARY_NAMES:
        _check(ctxs, FACT, group, [cases[name]], shares)


@pytest.mark.parametrize("t", CC.CHUNK_TS)
@pytest.mark.parametrize("group", [1, 2])
def test_chunk_cases(ctxs, shares, group, t):
    """k_lagrange_inv at 1, 2, 3 and 4 terms per thread, empty and ragged last chunks; a call has
    one t, so one call per t, the sparse (generic) instance beside a dense (factorial) one."""
    _check(ctxs, FACT, group, CC.chunk_cases()[t], shares)


@pytest.fixture(scope="module")
def limit_want():
    """The references of the two t-limit cases (2 - 3 s of Python each), computed once."""
    return {c.name: CC.expected(c, 1) for c in CC.limit_cases()}


@pytest.mark.parametrize("which", [0, 1], ids=["t4096_fact", "t4097_generic"])
def test_t_limit(ctxs, shares, limit_want, which):
    """t = 4096 over x = 1..4352 (the factorial route at its table top, xs[] full) and t = 4097
    (generic, 17 terms per thread), G1, default setting."""
    case = CC.limit_cases()[which]
    got = _combine(ctxs["default"], 1, [case], shares)
    assert got == [limit_want[case.name]]


@pytest.mark.parametrize("group", [1, 2])
def test_selection_cases(ctxs, shares, group):
    """k_select through hbtc_combine_*_verified_dev with the status array uploaded here: item
    counts and t-th accepted items around the 64-item ballots, a whole ballot rejected, a repeat
    whose first copy is rejected, undecodable encodings around the selection; and one selected, in
    the plain form (DECODE_ERR)."""
    ver = [c for c in CC.selection_cases() if c.verified]
    plain = [c for c in CC.selection_cases() if not c.verified]
    assert plain
    _check(ctxs, FACT, group, ver, shares)
    _check(ctxs, FACT, group, plain, shares)


@pytest.mark.parametrize("t", CC.SMALL_TS)
@pytest.mark.parametrize("group", [1, 2])
def test_small_cases(ctxs, shares, group, t):
    """hbtc_comb.hip's own selection and lambda loop (default), and the same instances through
    k_select and the Lagrange kernels (HBTC_COMB_SMALL=0)."""
    cases = CC.small_cases()[t]
    _check(ctxs, ("default", "nosmall"), group, [c for c in cases if not c.verified], shares)
    _check(ctxs, ("default", "nosmall"), group, [c for c in cases if c.verified], shares)
