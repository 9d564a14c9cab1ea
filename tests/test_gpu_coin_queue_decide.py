"""CoinEpoch(decide=True) -- the flush through ONE hbtc_coin_decide call -- against
CoinEpoch(decide=False) and against the reference's sequential coin (oracle/hbbft_rules.py, driven
as tests/test_protocol.py drives it): the same event streams give equal step lists, and the
`decided` / `fallback` counters say which path every instance took.

Key sets of N = 10 (t = 4, the one-workgroup combines) and N = 196 (t = 66, the Pippenger path), three
instances each.  Scenarios: every share valid with the input first; a forged share before the
threshold; the input after t + 2 shares; a sender repeating its share; state carried across two
flushes; a wrong master key (VerificationFailed and the synchronous replay).

The oracle's crypto is the construction: share i of instance k is (sk_i h_k) G2, valid iff its
bytes are those; t valid shares combine to (poly[0] h_k) G2, whose parity the Python oracle reads.
"""
import random

import pytest

from hbbft_amd import _native as N
from hbbft_amd import protocol as P
from oracle import bls12_381 as B
from oracle import hbbft_rules as RULES
from oracle import threshold_crypto as T

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
G2 = B.g2_compress(B.G2_GEN)
N_INST = 3
SCENARIOS = ["valid_input_first", "forged_before_threshold", "late_input", "repeated_sender",
             "two_flushes", "wrong_master"]


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[10, 196])
def world(request, ctx):
    """Key set, shares and expected coins of N_INST instances, computed once per N."""
    n = request.param
    rng = random.Random(n)
    f = (n - 1) // 3
    t = f + 1
    poly = [rng.randrange(1, R) for _ in range(t)]
    sks = [sum(c * pow(i + 1, e, R) for e, c in enumerate(poly)) % R for i in range(n)]
    pk, st = ctx.g1_mul(G1, sks)
    assert not st.any()
    pks = [bytes(pk[48 * i:48 * i + 48]) for i in range(n)]
    mpk, _ = ctx.g1_mul(G1, [poly[0]])
    wrong, _ = ctx.g1_mul(G1, [(poly[0] + 1) % R])
    hs = [rng.randrange(1, R) for _ in range(N_INST)]
    Hs, _ = ctx.g2_mul(G2, hs)
    H = [bytes(Hs[96 * k:96 * k + 96]) for k in range(N_INST)]
    sg, st = ctx.g2_mul(G2, [sks[i] * h % R for h in hs for i in range(n)])
    assert not st.any()
    good = [[bytes(sg[96 * (k * n + i):96 * (k * n + i) + 96]) for i in range(n)] for k in range(N_INST)]
    fg, _ = ctx.g2_mul(G2, [(sks[1] * h + 1) % R for h in hs])
    forged = [bytes(fg[96 * k:96 * k + 96]) for k in range(N_INST)]
    cs, _ = ctx.g2_mul(G2, [poly[0] * h % R for h in hs])
    coin = [bytes(cs[96 * k:96 * k + 96]) for k in range(N_INST)]
    parity = [T.signature_parity(B.g2_decompress(c, check_subgroup=False)) for c in coin]
    ids = ["n%03d" % i for i in range(n)]
    ks, nbad = ctx.keyset_load(pks)
    assert nbad == 0
    yield dict(n=n, f=f, t=t, ids=ids, ks=ks, mpk=bytes(mpk), wrong=bytes(wrong), H=H, good=good,
               forged=forged, coin=coin, parity=parity)
    ctx.keyset_free(ks)


def _events(w, scenario, k):
    """The event stream of instance k (this node is ids[0]) and where to cut it into flushes."""
    n, t, ids, good = w["n"], w["t"], w["ids"], w["good"][k]
    rng = random.Random(100 * k + len(scenario))
    msg = lambda i, s=None: ("msg", ids[i], good[i] if s is None else s)
    others = list(range(1, n))
    rng.shuffle(others)
    cut = None
    if scenario in ("valid_input_first", "wrong_master"):
        ev = [("input",)] + [msg(i) for i in others[:t + 1]]
    elif scenario == "forged_before_threshold":
        ev = [("input",), msg(others[0]), msg(others[1], w["forged"][k])] + [msg(i) for i in others[2:t + 2]]
    elif scenario == "late_input":  # t + 2 shares from the highest indices down, then the input
        ev = [msg(n - 1 - j) for j in range(t + 2)] + [("input",)]
    elif scenario == "repeated_sender":
        ev = [("input",), msg(others[0]), msg(others[0])] + [msg(i) for i in others[1:t + 1]]
    else:  # two_flushes: the input and two shares, then the rest
        ev = [("input",), msg(others[0]), msg(others[1])] + [msg(i) for i in others[2:t + 2]]
        cut = 3
    return ev, cut


def _strip(steps):
    return [{"faults": s["faults"], "output": s["output"], "error": s["error"]} for s in steps]


def _run_queue(ctx, w, scenario, decide):
    mpk = w["wrong"] if scenario == "wrong_master" else w["mpk"]
    ni = P.NetInfo(w["ids"], w["ids"][0], w["ks"], master_pk=mpk)
    ep = P.CoinEpoch(ctx, ni, decide=decide)
    streams = {}
    for k in range(N_INST):
        ep.add(k, w["H"][k], w["good"][k][0])
        streams[k] = _events(w, scenario, k)
    got = {k: [] for k in streams}
    counters = []
    for part in (0, 1):
        fed = False
        for k, (ev, cut) in streams.items():
            seg = ev[:cut] if part == 0 else (ev[cut:] if cut is not None else [])
            for e in seg:
                fed = True
                (ep.handle_input(k) if e[0] == "input" else ep.handle_message(k, e[1], e[2]))
        if fed:
            for k, steps in ep.flush().items():
                got[k] += _strip(steps)
            counters.append((ep.decided, ep.fallback))
    return got, counters, streams


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_decide_queue_equals_default_and_reference(ctx, world, scenario):
    w = world
    plain, c0, streams = _run_queue(ctx, w, scenario, decide=False)
    fast, c1, _ = _run_queue(ctx, w, scenario, decide=True)
    print(w["n"], scenario, c0, c1)
    assert fast == plain
    for k, (ev, _) in streams.items():
        good = w["good"][k]
        ref = RULES.Coin(w["ids"], w["ids"][0], w["f"], good[0],
                         lambda sender, share, good=good: share == good[w["ids"].index(sender)],
                         lambda items, k=k: (w["coin"][k], w["parity"][k]),
                         lambda sig: scenario != "wrong_master")
        assert fast[k] == ref.run(ev), (scenario, k)
        outs = [s["output"] for s in fast[k] if s["output"] is not None]
        if scenario == "wrong_master":
            assert outs == [] and sum(s["error"] == "VerificationFailed" for s in fast[k]) >= 2
        else:
            assert outs == [w["parity"][k]]
    assert all(c == (0, 0) for c in c0)  # the default queue never takes the one-call path
    if scenario in ("valid_input_first", "forged_before_threshold", "wrong_master"):
        assert c1 == [(N_INST, 0)]
    elif scenario in ("late_input", "repeated_sender"):
        assert c1 == [(0, N_INST)]
    else:  # two flushes: nothing to combine in the first, carried shares in the second
        assert c1 == [(0, 0), (0, N_INST)]
