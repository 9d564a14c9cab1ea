"""GPU parity of hbtc_coin_decide above the one-workgroup combines (t > 64: one selection, the
G2 Pippenger combine, the G1 Pippenger master check over the key set's shares gathered by node
index, the status merged on the device) against the separate entry points it replaces:
hbtc_verify_sig_shares, the first t ACCEPTed shares through hbtc_combine_sigs, hbtc_verify_sigs
against the master key -- and against the construction: every instance with t valid shares
combines to (poly[0] h_k) G2.

Shapes (n, t, n_inst): (70, 65, 8) the first threshold over the limit, 560 items, the batch (RLC)
route; (70, 65, 3) 210 items, below exact_below, the exact route (also under MODE_PER_SHARE);
(70, 64, 8) the boundary, still on the small path; (140, 129, 4) a selection longer than two
waves and an MSM plan of another size.  Patterns cycle over the instances, shifted call by call
so that every shape sees all of them: valid; one wrong share among the first t; the wrong share
right after them; two wrong; fewer than t valid; a bad G2 encoding; an unknown sender; a
repeated node index; the items in descending node order.  Each with the right master key and
with a wrong one (every otherwise-ACCEPT instance REJECT).  Bar: identical statuses, bytes,
parities and coin statuses.
"""
import json
import os
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu

R = B.R
HERE = os.path.dirname(os.path.abspath(__file__))
PATTERNS = ["valid", "one_wrong_first", "wrong_after", "two_wrong", "short", "bad_enc", "unknown",
            "dup", "descending"]


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def _instances(n, t, n_inst, start, sks, hs, bad2):
    """counts, idx, sig scalars, byte overrides and the pattern of every instance."""
    counts, idx, scal, edits, kinds = [], [], [], [], []
    for k in range(n_inst):
        kind = PATTERNS[(start + k) % len(PATTERNS)]
        ids = list(range(n))
        if kind == "unknown":
            ids = [0, n + 5] + list(range(1, n))  # sender n + 5 is not in the key set
        if kind == "dup":
            ids = [0, 1, 1] + list(range(2, n))
        if kind == "descending":
            ids = ids[::-1]
        wrong = set()
        if kind == "one_wrong_first":
            wrong = {2}
        elif kind == "wrong_after":
            wrong = {t}
        elif kind == "two_wrong":
            wrong = {0, 1}
        elif kind == "short":
            wrong = set(range(n - t + 1))  # only t - 1 valid shares
        base = len(scal)
        for j, i in enumerate(ids):
            s = sks[i % len(sks)] * hs[k] % R
            scal.append((s + 1) % R if j in wrong else s)
        if kind == "bad_enc":
            edits.append((base + 1, bad2[k % len(bad2)]))
        counts.append(len(ids))
        idx += ids
        kinds.append(kind)
    return counts, idx, scal, edits, kinds


def _reference(ctx, ks, H, counts, idx, sigs, t, mpk):
    """The separate entry points, as hbbft calls them per share / per combine / per check."""
    st = ctx.verify_sig_shares(ks, H, counts, idx, sigs)
    sel_counts, sel_idx, sel_sigs = [], [], []
    pos = 0
    for c in counts:
        acc = [j for j in range(pos, pos + c) if st[j] == N.ACCEPT][:t]
        sel_counts.append(len(acc))
        sel_idx += [idx[j] for j in acc]
        sel_sigs += [sigs[j] for j in acc]
        pos += c
    out, par, cst = ctx.combine_sigs(sel_counts, sel_idx, sel_sigs, t)
    coin = [int(c) for c in cst]
    ok = [k for k in range(len(counts)) if coin[k] == N.ACCEPT]
    if ok:
        v = ctx.verify_sigs([mpk] * len(ok), [H[k] for k in ok], [out[k] for k in ok])
        for k, r in zip(ok, v):
            coin[k] = int(r)
    return st, out, par, cst, coin


# what the composed calls give per pattern with the right master key
WANT_COIN = {"valid": N.ACCEPT, "one_wrong_first": N.ACCEPT, "wrong_after": N.ACCEPT, "two_wrong": N.ACCEPT,
             "short": N.NOT_ENOUGH_SHARES, "bad_enc": N.ACCEPT, "unknown": N.ACCEPT,
             "dup": N.DUPLICATE_ENTRY, "descending": N.ACCEPT}


def _run(ctx, n, t, n_inst, mode=None):
    rng = random.Random(1000 * n + 10 * t + n_inst)
    poly = [rng.randrange(1, R) for _ in range(t)]
    sks = [sum(c * pow(i + 1, e, R) for e, c in enumerate(poly)) % R for i in range(n)]
    g1 = B.g1_compress(B.G1_GEN)
    g2 = B.g2_compress(B.G2_GEN)
    pk, st = ctx.g1_mul(g1, sks)
    assert not st.any()
    mpk, _ = ctx.g1_mul(g1, [poly[0]])
    wrong_mpk, _ = ctx.g1_mul(g1, [(poly[0] + 1) % R])
    codec = json.load(open(os.path.join(HERE, "golden", "codec.json")))
    bad2 = [bytes.fromhex(x["enc"]) for x in codec["g2_bad"]]
    c2 = N.Context(0)  # the call under test on a context of its own (and its own verify mode)
    try:
        if mode is not None:
            ctx.set_verify_mode(mode)
            c2.set_verify_mode(mode)
        ks, nbad = ctx.keyset_load(pk)
        ks2, nbad2 = c2.keyset_load(pk)
        assert nbad == 0 and nbad2 == 0
        for start in range(0, len(PATTERNS), n_inst):
            hs = [rng.randrange(1, R) for _ in range(n_inst)]
            Hs, _ = ctx.g2_mul(g2, hs)
            H = [bytes(Hs[96 * k:96 * k + 96]) for k in range(n_inst)]
            counts, idx, scal, edits, kinds = _instances(n, t, n_inst, start, sks, hs, bad2)
            sg, st2 = ctx.g2_mul(g2, scal)  # sigma_i = sk_i * H_k = (sk_i h_k) G2
            assert not st2.any()
            sigs = [bytes(sg[96 * i:96 * i + 96]) for i in range(len(scal))]
            for pos, enc in edits:
                sigs[pos] = enc
            want, _ = ctx.g2_mul(g2, [poly[0] * h % R for h in hs])
            for master in (bytes(mpk), bytes(wrong_mpk)):
                ctx.keyset_set_master(ks, master)
                c2.keyset_set_master(ks2, master)
                ref = _reference(ctx, ks, H, counts, idx, sigs, t, master)
                st_g, out_g, par_g, coin_g = c2.coin_decide(ks2, H, counts, idx, sigs, t)
                print(n, t, n_inst, start, master == bytes(mpk), kinds, list(coin_g), ref[4])
                assert list(st_g) == list(ref[0]), kinds
                assert out_g == ref[1], kinds
                assert list(par_g) == list(ref[2]), kinds
                assert list(coin_g) == ref[4], (list(coin_g), ref[4], kinds)
                for k, kind in enumerate(kinds):
                    if master == bytes(mpk):
                        assert ref[4][k] == WANT_COIN[kind], (kind, ref[4][k])
                    else:  # every otherwise-ACCEPT instance fails the master check
                        assert ref[4][k] == (N.REJECT if WANT_COIN[kind] == N.ACCEPT else WANT_COIN[kind]), kind
                    if ref[3][k] == N.ACCEPT:
                        # the construction: t valid shares combine to (poly[0] h_k) G2
                        assert out_g[k] == bytes(want[96 * k:96 * k + 96]), kind
        ctx.keyset_free(ks)
    finally:
        if mode is not None:
            ctx.set_verify_mode(N.MODE_RLC)
        c2.close()


@pytest.mark.parametrize("n,t,n_inst", [(70, 65, 8), (70, 65, 3), (70, 64, 8), (140, 129, 4)])
def test_coin_decide_large_equals_separate_calls(ctx, n, t, n_inst):
    _run(ctx, n, t, n_inst)


def test_coin_decide_large_per_share(ctx):
    _run(ctx, 70, 65, 3, mode=N.MODE_PER_SHARE)


def test_coin_decide_large_on_generated_keyset(ctx):
    """A key set left loaded by hbtc_skg_generate carries its master key (the commitment's constant
    term) without hbtc_keyset_set_master: the large-t round runs on it, blocking and ticketed."""
    n, t, n_inst = 70, 66, 2
    rng = random.Random(4242)
    poly = [rng.randrange(1, R) for _ in range(t)]
    sks = [sum(c * pow(i + 1, e, R) for e, c in enumerate(poly)) % R for i in range(n)]
    g1 = B.g1_compress(B.G1_GEN)
    g2 = B.g2_compress(B.G2_GEN)
    row, st = ctx.g1_mul(g1, poly)  # one Part: its row 0 is the era's commitment
    assert not st.any()
    commit, _, _, ks, status = ctx.skg_generate(t - 1, bytes(row), None, n, load_keyset=True)
    assert status == N.ACCEPT and ks is not None
    try:
        hs = [rng.randrange(1, R) for _ in range(n_inst)]
        Hs, _ = ctx.g2_mul(g2, hs)
        H = [bytes(Hs[96 * k:96 * k + 96]) for k in range(n_inst)]
        sg, _ = ctx.g2_mul(g2, [sks[i] * h % R for h in hs for i in range(n)])
        sigs = [bytes(sg[96 * i:96 * i + 96]) for i in range(n * n_inst)]
        idx = list(range(n)) * n_inst
        want, _ = ctx.g2_mul(g2, [poly[0] * h % R for h in hs])
        got = ctx.coin_decide(ks, H, [n] * n_inst, idx, sigs, t)
        tick = ctx.coin_epoch_submit(ks, H, [0, n, 2 * n], idx, sigs, t).wait()
        for st_i, out, par, cst in (got, tick):
            assert not np.asarray(st_i)[:n * n_inst].any()
            assert [int(c) for c in cst[:n_inst]] == [N.ACCEPT] * n_inst
            assert [bytes(out[k]) for k in range(n_inst)] == [bytes(want[96 * k:96 * k + 96]) for k in range(n_inst)]
        assert list(got[2]) == list(tick[2][:n_inst])
    finally:
        ctx.keyset_free(ks)
