"""GPU checks of the lane-uniform bucket walk (msm_walk.h in k_msm_buckets and k_msm_buckets_g2p)
through the public API: hbtc_g1_msm / hbtc_g2_msm at the shapes where the walk takes another path
(lanes with nothing to do beside full walks, one lane leaving every rank at one position, windows
of a few terms, a crowded top window, cancelling and repeated points inside a bucket), and the
decryption and signature combines at the smallest t that goes through Pippenger over the
endomorphism split.

Expected values: [sum_i k_i a_i] G from hbtc_g1_mul / hbtc_g2_mul for points a_i G (the identity
tests/test_gpu_msm.py uses), the Python oracle for one small case of each group.  Bar:
byte-identical compressed points (integer arithmetic, no tolerance).
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
SIZE = {1: 48, 2: 96}


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


def _gen(ctx, group, vals):
    """[v] G compressed, via the library (checked against the oracle in test_gpu_parity); v = 0 mod r:
    the infinity encoding, written here"""
    size = SIZE[group]
    red = [v % R for v in vals]
    out, st = (ctx.g1_mul(G1, [v or 1 for v in red]) if group == 1 else ctx.g2_mul(G2, [v or 1 for v in red]))
    assert not st.any()
    inf = bytes([0xC0]) + bytes(size - 1)
    return [bytes(out[size * i:size * i + size]) if v else inf for i, v in enumerate(red)]


def _check_identity(ctx, group, n_msm, n, a, k):
    """msm of the points a_i G with the scalars k_i against [sum k_i a_i] G"""
    pts = _gen(ctx, group, a)
    msm = ctx.g1_msm if group == 1 else ctx.g2_msm
    out, st = msm(n_msm, n, pts, k)
    assert list(st) == [N.ACCEPT] * n_msm
    want = _gen(ctx, group, [sum(k[m * n + i] * a[m * n + i] for i in range(n)) for m in range(n_msm)])
    assert out == want


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 7, 9])
def test_few_terms(ctx, group, n):
    """Fewer terms than segments in most windows: slices with p0 == p1 beside slices of one term."""
    rng = random.Random(100 * group + n)
    n_msm = 3
    a = [rng.randrange(1, R) for _ in range(n_msm * n)]
    k = [rng.randrange(0, R) for _ in range(n_msm * n)]
    _check_identity(ctx, group, n_msm, n, a, k)


@pytest.mark.parametrize("group", [1, 2])
def test_all_scalars_and_points_equal(ctx, group):
    """n = 64, one point and one scalar: every window has one bucket, every mixed addition after the
    first is the doubling case or follows it."""
    rng = random.Random(200 + group)
    a, k = rng.randrange(1, R), rng.randrange(1, R)
    _check_identity(ctx, group, 1, 64, [a] * 64, [k] * 64)


@pytest.mark.parametrize("group", [1, 2])
def test_first_slice_leaves_every_rank(ctx, group):
    """n = 334.  For every window width c the library may choose, one MSM whose window 0 holds one
    digit of magnitude B = 2^(c-1) and 333 digits 1 (the first slice leaves B - 1 ranks at one
    position: the same snapshot again and again, a flush each time the slots are full), and whose
    window 1 holds only 8 nonzero digits spread over the ranks; the windows above are empty."""
    rng = random.Random(300 + group)
    n, widths = 334, list(range(4, 11))
    a = [rng.randrange(1, R) for _ in range(len(widths) * n)]
    k = []
    for c in widths:
        nb = 1 << (c - 1)
        d0 = [nb if i == 100 else 1 for i in range(n)]
        d1 = [0] * n
        for j in range(8):
            d1[3 + 41 * j] = max(1, nb * j // 8 + (j & 1))
        k += [d0[i] + (d1[i] << c) for i in range(n)]
    _check_identity(ctx, group, len(widths), n, a, k)


@pytest.mark.parametrize("group", [1, 2])
def test_cancelling_and_identity_terms_in_one_bucket(ctx, group):
    """P / -P pairs and infinity encodings under one scalar: `run` returns to the identity in
    mid-walk, and the whole MSM may cancel."""
    rng = random.Random(400 + group)
    inf = bytes([0xC0]) + bytes(SIZE[group] - 1)
    msm = ctx.g1_msm if group == 1 else ctx.g2_msm
    n = 40
    a = [rng.randrange(1, R) for _ in range(n // 4)]
    k0 = rng.randrange(1, R)
    av, ks = [], []
    for j, v in enumerate(a):  # P, -P, infinity, and one more point of its own scalar
        av += [v, R - v, 0, v]
        ks += [k0, k0, k0, rng.randrange(1, R) if j & 1 else k0]
    pts = _gen(ctx, group, av)
    assert pts[2] == inf
    out, st = msm(1, n, pts, ks)
    assert list(st) == [N.ACCEPT]
    assert out == _gen(ctx, group, [sum(x * y for x, y in zip(ks, av))])
    # everything cancels
    out, st = msm(1, n // 2, _gen(ctx, group, [v for x in a for v in (x, R - x)]), [k0] * (n // 2))
    assert list(st) == [N.ACCEPT] and out == [inf]


@pytest.mark.parametrize("group", [1, 2])
def test_idle_lanes_beside_full_walks(ctx, group):
    """n_msm = 9: one MSM of all-zero scalars and one with a single nonzero scalar between full
    ones, so a wave holds lanes with nothing to do beside lanes that walk a full slice."""
    rng = random.Random(500 + group)
    n_msm, n = 9, 334 if group == 1 else 120
    a = [rng.randrange(1, R) for _ in range(n_msm * n)]
    k = [rng.randrange(0, R) for _ in range(n_msm * n)]
    for i in range(n):
        k[2 * n + i] = 0
        k[5 * n + i] = 0
    k[5 * n + 77] = rng.randrange(1, R)
    pts = _gen(ctx, group, a)
    msm = ctx.g1_msm if group == 1 else ctx.g2_msm
    out, st = msm(n_msm, n, pts, k)
    assert list(st) == [N.ACCEPT] * n_msm
    inf = bytes([0xC0]) + bytes(SIZE[group] - 1)
    want = _gen(ctx, group, [sum(k[m * n + i] * a[m * n + i] for i in range(n)) for m in range(n_msm)])
    assert want[2] == inf
    assert out == want


@pytest.mark.parametrize("group", [1, 2])
def test_crowded_top_window(ctx, group):
    """Scalars r - 1 and 2^254 + 1: the top window has one or two buckets for all the terms."""
    rng = random.Random(600 + group)
    n = 200
    a = [rng.randrange(1, R) for _ in range(2 * n)]
    k = [R - 1] * n + [(1 << 254) + 1] * n
    _check_identity(ctx, group, 2, n, a, k)


@pytest.mark.parametrize("group", [1, 2])
def test_small_msm_against_the_oracle(ctx, group):
    rng = random.Random(700 + group)
    n_msm, n = 2, 5
    a = [rng.randrange(1, R) for _ in range(n_msm * n)]
    k = [rng.randrange(0, R) for _ in range(n_msm * n)]
    pts = _gen(ctx, group, a)
    out, st = (ctx.g1_msm if group == 1 else ctx.g2_msm)(n_msm, n, pts, k)
    assert not st.any()
    dec, mul, add, comp = ((B.g1_decompress, B.g1_mul, B.g1_add, B.g1_compress) if group == 1 else
                           (B.g2_decompress, B.g2_mul, B.g2_add, B.g2_compress))
    for m in range(n_msm):
        acc = None
        for i in range(n):
            term = mul(dec(pts[m * n + i]), k[m * n + i])
            acc = term if acc is None else add(acc, term)
        assert out[m] == comp(acc)


def _dev(ctx, arr):
    a = np.ascontiguousarray(arr)
    p = ctx.dev_alloc(max(a.nbytes, 16))
    if a.nbytes:
        ctx.dev_upload(p, a)
    return p


def test_decrypt_combine_past_the_small_threshold(ctx):
    """N = 100, t = 65 (the smallest t past the one-workgroup combines: Pippenger over the GLV
    halves), 3 ciphertexts.  One wrong share sits at a different index in each ciphertext, so the
    selected sets (the first t verified shares) differ; the combine must give master * r_k * G."""
    rng = random.Random(800)
    n, t, n_ct = 100, 65, 3
    coeffs = [rng.randrange(1, R) for _ in range(t)]
    sks = [sum(c * pow(i + 1, j, R) for j, c in enumerate(coeffs)) % R for i in range(n)]
    ks, nbad = ctx.keyset_load(_gen(ctx, 1, sks))
    assert nbad == 0
    rs = [rng.randrange(1, R) for _ in range(n_ct)]
    hs = [rng.randrange(1, R) for _ in range(n_ct)]
    H = _gen(ctx, 2, hs)
    w = _gen(ctx, 2, [r * h for r, h in zip(rs, hs)])
    wrong = {0: 0, 1: 31, 2: 64}
    scal = [(sks[i] * rs[k] + (1 if wrong[k] == i else 0)) % R for k in range(n_ct) for i in range(n)]
    shares = np.frombuffer(b"".join(_gen(ctx, 1, scal)), np.uint8).copy()
    idx = np.tile(np.arange(n, dtype=np.uint32), n_ct)
    off = np.arange(0, n * n_ct + 1, n, dtype=np.uint32)
    d_H = _dev(ctx, np.frombuffer(b"".join(H), np.uint8))
    d_w = _dev(ctx, np.frombuffer(b"".join(w), np.uint8))
    d_idx, d_sh = _dev(ctx, idx), _dev(ctx, shares)
    d_st = ctx.dev_alloc(4 * n * n_ct)
    d_g, d_cst = ctx.dev_alloc(48 * n_ct), ctx.dev_alloc(4 * n_ct)
    lib, h = ctx.lib, ctx.h
    offp = N._ptr(off)
    ctx._check(lib.hbtc_verify_dec_shares_dev(h, ks, n_ct, d_H, d_w, offp, d_idx, d_sh, d_st), "verify")
    ctx._check(lib.hbtc_combine_dec_verified_dev(h, n_ct, offp, d_idx, d_sh, d_st, t, d_g, d_cst),
               "combine verified")
    st = np.empty(n * n_ct, np.int32)
    ctx.dev_download(st, d_st)
    g = np.empty(48 * n_ct, np.uint8)
    ctx.dev_download(g, d_g)
    cst = np.empty(n_ct, np.int32)
    ctx.dev_download(cst, d_cst)
    assert list(st) == [N.REJECT if wrong[k] == i else N.ACCEPT for k in range(n_ct) for i in range(n)]
    assert list(cst) == [N.ACCEPT] * n_ct
    want = _gen(ctx, 1, [coeffs[0] * r for r in rs])
    assert [bytes(g[48 * k:48 * k + 48]) for k in range(n_ct)] == want


def test_sig_combine_past_the_small_threshold(ctx):
    """The same for the Coin's combine (k_msm_buckets_g2p over the four ψ parts of every share):
    N = 100, t = 65, 3 instances, one wrong share at a different index in each; the combined
    signature must be master * H_k."""
    rng = random.Random(900)
    n, t, n_inst = 100, 65, 3
    coeffs = [rng.randrange(1, R) for _ in range(t)]
    sks = [sum(c * pow(i + 1, j, R) for j, c in enumerate(coeffs)) % R for i in range(n)]
    ks, nbad = ctx.keyset_load(_gen(ctx, 1, sks))
    assert nbad == 0
    hs = [rng.randrange(1, R) for _ in range(n_inst)]
    H = _gen(ctx, 2, hs)
    wrong = {0: 1, 1: 40, 2: 64}
    scal = [(sks[i] * hs[k] + (1 if wrong[k] == i else 0)) % R for k in range(n_inst) for i in range(n)]
    sigs = np.frombuffer(b"".join(_gen(ctx, 2, scal)), np.uint8).copy()
    idx = np.tile(np.arange(n, dtype=np.uint32), n_inst)
    off = np.arange(0, n * n_inst + 1, n, dtype=np.uint32)
    d_H = _dev(ctx, np.frombuffer(b"".join(H), np.uint8))
    d_idx, d_sig = _dev(ctx, idx), _dev(ctx, sigs)
    d_st = ctx.dev_alloc(4 * n * n_inst)
    d_out, d_par, d_cst = ctx.dev_alloc(96 * n_inst), ctx.dev_alloc(16), ctx.dev_alloc(4 * n_inst)
    lib, h = ctx.lib, ctx.h
    offp = N._ptr(off)
    ctx._check(lib.hbtc_verify_sig_shares_dev(h, ks, n_inst, d_H, offp, d_idx, d_sig, d_st), "verify")
    ctx._check(lib.hbtc_combine_sigs_verified_dev(h, n_inst, offp, d_idx, d_sig, d_st, t, d_out, d_par, d_cst),
               "combine verified")
    st = np.empty(n * n_inst, np.int32)
    ctx.dev_download(st, d_st)
    out = np.empty(96 * n_inst, np.uint8)
    ctx.dev_download(out, d_out)
    cst = np.empty(n_inst, np.int32)
    ctx.dev_download(cst, d_cst)
    assert list(st) == [N.REJECT if wrong[k] == i else N.ACCEPT for k in range(n_inst) for i in range(n)]
    assert list(cst) == [N.ACCEPT] * n_inst
    want = _gen(ctx, 2, [coeffs[0] * hv for hv in hs])
    assert [bytes(out[96 * k:96 * k + 96]) for k in range(n_inst)] == want
