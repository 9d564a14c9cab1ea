"""hbtc_coin_epoch_submit (the coin round on a ticket: share checks, combine, master check and the
coin status merged on the device, collected by hbtc_wait) against hbtc_coin_decide on the same
inputs, at a threshold on each side of the one-workgroup combines' limit: (n, t, n_inst) =
(10, 4, 8) and (70, 65, 8).  Five tickets with different inputs are submitted back to back --
one more than the lanes, so the first lane's staging is reused -- and waited for out of order.
A key set without a master key and t = 0 are refused before anything is enqueued.
"""
import random

import numpy as np
import pytest

from hbbft_amd import _native as N
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu

R = B.R
G1 = B.g1_compress(B.G1_GEN)
G2 = B.g2_compress(B.G2_GEN)


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def _keys(ctx, rng, n, t):
    poly = [rng.randrange(1, R) for _ in range(t)]
    sks = [sum(c * pow(i + 1, e, R) for e, c in enumerate(poly)) % R for i in range(n)]
    pk, st = ctx.g1_mul(G1, sks)
    assert not st.any()
    mpk, _ = ctx.g1_mul(G1, [poly[0]])
    return poly, sks, pk, bytes(mpk)


def _round(ctx, rng, n, t, n_inst, sks):
    """One round's inputs: per instance a rotation of the senders, with a wrong share among the
    first t in some instances, too few valid ones in another and a repeated sender in another."""
    hs = [rng.randrange(1, R) for _ in range(n_inst)]
    Hs, _ = ctx.g2_mul(G2, hs)
    H = [bytes(Hs[96 * k:96 * k + 96]) for k in range(n_inst)]
    offsets, idx, scal = [0], [], []
    for k in range(n_inst):
        rot = rng.randrange(n)
        ids = [(rot + j) % n for j in range(n)]
        wrong = set()
        if k % 4 == 1:
            wrong = {rng.randrange(t)}
        elif k % 4 == 2:
            wrong = set(range(n - t + 1))
        elif k % 4 == 3:
            ids = ids[:1] + ids[:1] + ids[1:]
        for j, i in enumerate(ids):
            s = sks[i] * hs[k] % R
            scal.append((s + 1) % R if j in wrong else s)
        idx += ids
        offsets.append(len(idx))
    sg, st = ctx.g2_mul(G2, scal)
    assert not st.any()
    sigs = [bytes(sg[96 * i:96 * i + 96]) for i in range(len(scal))]
    return H, offsets, idx, sigs, hs


def _same(got, want, n_items, n_inst):
    st, sig, par, cst = got
    assert list(st[:n_items]) == list(want[0])
    assert [bytes(sig[k]) for k in range(n_inst)] == want[1]
    assert list(par[:n_inst]) == list(want[2])
    assert list(cst[:n_inst]) == list(want[3])


@pytest.mark.parametrize("n,t,n_inst", [(10, 4, 8), (70, 65, 8)])
def test_coin_epoch_submit_equals_coin_decide(ctx, n, t, n_inst):
    rng = random.Random(7 * n + t)
    poly, sks, pk, mpk = _keys(ctx, rng, n, t)
    ks, nbad = ctx.keyset_load(pk)
    assert nbad == 0
    try:
        wrong, _ = ctx.g1_mul(G1, [(poly[0] + 1) % R])
        for master in (mpk, bytes(wrong)):
            ctx.keyset_set_master(ks, master)
            H, off, idx, sigs, hs = _round(ctx, rng, n, t, n_inst, sks)
            want = ctx.coin_decide(ks, H, None, idx, sigs, t, offsets=off)
            got = ctx.coin_epoch_submit(ks, H, off, idx, sigs, t).wait()
            _same(got, want, off[-1], n_inst)
            codes = set(int(c) for c in want[3])
            assert N.NOT_ENOUGH_SHARES in codes and N.DUPLICATE_ENTRY in codes
            assert (N.ACCEPT if master == mpk else N.REJECT) in codes
            if master == mpk:  # the construction: an ACCEPTed coin's signature is (poly[0] h_k) G2
                sig, _ = ctx.g2_mul(G2, [poly[0] * h % R for h in hs])
                for k in range(n_inst):
                    if int(want[3][k]) == N.ACCEPT:
                        assert bytes(got[1][k]) == bytes(sig[96 * k:96 * k + 96])
    finally:
        ctx.keyset_free(ks)


@pytest.mark.parametrize("n,t,n_inst", [(10, 4, 8), (70, 65, 4)])
def test_coin_epoch_five_tickets_out_of_order(ctx, n, t, n_inst):
    rng = random.Random(99 + t)
    poly, sks, pk, mpk = _keys(ctx, rng, n, t)
    ks, _ = ctx.keyset_load(pk)
    try:
        ctx.keyset_set_master(ks, mpk)
        rounds = [_round(ctx, rng, n, t, n_inst, sks) for _ in range(5)]
        want = [ctx.coin_decide(ks, H, None, idx, sigs, t, offsets=off) for H, off, idx, sigs, _ in rounds]
        pend = [ctx.coin_epoch_submit(ks, H, off, idx, sigs, t) for H, off, idx, sigs, _ in rounds]
        for j in (3, 0, 4, 2, 1):
            _same(pend[j].wait(), want[j], rounds[j][1][-1], n_inst)
    finally:
        ctx.keyset_free(ks)


def test_coin_epoch_submit_refusals(ctx):
    rng = random.Random(5)
    poly, sks, pk, mpk = _keys(ctx, rng, 10, 4)
    ks, _ = ctx.keyset_load(pk)
    try:
        H, off, idx, sigs, _ = _round(ctx, rng, 10, 4, 2, sks)
        with pytest.raises(N.HbtcError):  # no master key
            ctx.coin_epoch_submit(ks, H, off, idx, sigs, 4)
        ctx.keyset_set_master(ks, mpk)
        with pytest.raises(N.HbtcError):  # t = 0
            ctx.coin_epoch_submit(ks, H, off, idx, sigs, 0)
        # nothing was enqueued by either: the next ticket is the context's next one, and works
        a = ctx.coin_epoch_submit(ks, H, off, idx, sigs, 4)
        b = ctx.coin_epoch_submit(ks, H, off, idx, sigs, 4)
        assert b.ticket == a.ticket + 1
        want = ctx.coin_decide(ks, H, None, idx, sigs, 4, offsets=off)
        _same(b.wait(), want, off[-1], 2)
        _same(a.wait(), want, off[-1], 2)
    finally:
        ctx.keyset_free(ks)
    assert np.int32(N.ACCEPT) == 0
