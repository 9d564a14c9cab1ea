"""The DecryptionShare tile sums as a lane-dense tree kernel (hbtc_rlc.hip k_rlc_tree, rlc_tree.h).

Device test: on 40 tiles of every count and mask kind the tree's TileSums must equal, byte for
byte, what rlc_common.h rlc_reduce_sp (one wave per tile, the form k_rlc_items ended with before)
writes for the same inputs.

Public API tests: decisions equal the construction's and the per-share mode's at 128 and 64 bits
under every check schedule, with a wrong share at every position of a tile (every weight of the
tree locates), in the last position of ragged tiles, two wrong shares under every split level, and
lanes outside the sums beside summed ones.  The number of exact leaf checks of every call is the
one the in-kernel tree gave (recorded from a build with HBTC_RLC_TREE=0).
Reference: threshold_crypto's PublicKeyShare::verify_decryption_share, once per share."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from hbbft_amd import _native as N
from tests.test_gpu_parity import R, _keyset
from tests.test_gpu_rlc_sender_scalars import Batch, N_KEYS, SCHEDULES, _senders

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libhbtc_tree_devtest.so")
COUNTS = [1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64]
BAD_KEY = 21
AUTO, PLAIN, SUBS, LEAVES = SCHEDULES


# ------------------------------------------------------------------------------- device harness
@pytest.fixture(scope="module")
def td():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/libhbtc_tree_devtest.so"])
    lib = ctypes.CDLL(LIB)
    lib.td_group_tiles.restype = lib.td_sums_bytes.restype = ctypes.c_uint32
    assert lib.td_devices() >= 1
    return lib


def all_of(count):
    return (1 << count) - 1


def test_tree_bytes_equal_the_one_wave_reduction(td):
    """40 tiles (more than two groups, not a multiple of the group): every count with the masks
    all / none / one lane / alternating / only the last lane in turn, the rest random masks; lanes
    inside a mask carry random points, a few of them an identity S beside their P."""
    G = td.td_group_tiles()
    n_tiles = 40 if 40 % G else 41
    assert n_tiles > 2 * G and n_tiles % G
    rng = random.Random(830)
    n_pk = 70
    counts, masks, s_scal, idx = [], [], [], []
    for t in range(n_tiles):
        c = COUNTS[t % len(COUNTS)] if t < 33 else rng.choice((64, 64, 40, 5))
        kinds = [all_of(c), 0, 1 << (c // 2), all_of(c) & 0x5555555555555555, 1 << (c - 1)]
        m = kinds[(t // len(COUNTS) + t) % 5] if t < 33 else rng.getrandbits(64) & all_of(c)
        counts.append(c)
        masks.append(m)
        for i in range(c):
            inside = (m >> i) & 1
            s_scal.append(rng.randrange(1, 1 << 64) if inside and rng.random() > 0.05 else 0)
            idx.append(rng.randrange(n_pk))
    p_scal = [rng.randrange(1, 1 << 64) for _ in range(n_pk)]
    p_scal[3] = 0  # a sender whose table entry is the identity
    size = td.td_sums_bytes()
    ref = ctypes.create_string_buffer(n_tiles * size)
    got = ctypes.create_string_buffer(n_tiles * size)
    rc = td.td_tile_sums(n_tiles, (ctypes.c_uint32 * n_tiles)(*counts), (ctypes.c_uint64 * n_tiles)(*masks),
                         (ctypes.c_uint64 * len(s_scal))(*s_scal), (ctypes.c_uint32 * len(idx))(*idx), n_pk,
                         (ctypes.c_uint64 * n_pk)(*p_scal), ref, got)
    assert rc == 0, rc
    assert any(ref.raw[k] for k in range(0, len(ref.raw), 997))
    for t in range(n_tiles):
        a, b_ = ref.raw[t * size:(t + 1) * size], got.raw[t * size:(t + 1) * size]
        assert a == b_, (t, counts[t], hex(masks[t]), [j for j in range(size // 144) if a[144 * j:144 * j + 144] != b_[144 * j:144 * j + 144]])


# ----------------------------------------------------------------------------------- public API
@pytest.fixture(scope="module")
def env():
    ctx = N.Context(0)
    ctx.set_exact_below(0)
    ctx.set_sender_tracking(False)
    rng = random.Random(808)
    f, coeffs, sks, pk = _keyset(ctx, rng, N_KEYS)
    ks, bad = ctx.keyset_load(pk)
    assert bad == 0
    yield ctx, rng, sks, pk, ks
    ctx.set_rlc_bits(128)
    ctx.close()


def _run_all(ctx, ks, args, exp, leaves, name):
    """Per-share mode, then the RLC mode at both scalar widths under every check schedule; the
    exact leaf checks of every RLC call are leaves[schedule]."""
    ctx.set_verify_mode(N.MODE_PER_SHARE)
    st_ref = ctx.verify_dec_shares(ks, *args)
    assert (st_ref == exp).all(), (name, "per-share", np.nonzero(st_ref != exp))
    ctx.set_verify_mode(N.MODE_RLC)
    seen = {}
    try:
        for bits in (128, 64):
            ctx.set_rlc_bits(bits)
            for sched in SCHEDULES:
                ctx.set_check_schedule(sched)
                st = ctx.verify_dec_shares(ks, *args)
                assert (st == exp).all(), (name, bits, sched, np.nonzero(st != exp)[0], st[st != exp])
                seen[(bits, sched)] = ctx.rlc_last_leaves()
    finally:
        ctx.set_rlc_bits(128)
        ctx.set_check_schedule(N.CHECK_AUTO)
    print("leaves", name, seen)
    for (bits, sched), n in seen.items():
        assert n == leaves[sched], (name, bits, sched, seen)


def test_single_wrong_share_at_every_position(env):
    """64 instances of 64 shares, instance k wrong at position k only: the weighted sums of the
    tile locate every one of them, no exact check runs."""
    ctx, rng, sks, pk, ks = env
    bt = Batch(rng, sks)
    for k in range(64):
        bt.add("p%d" % k, _senders(rng, 64), delta={k: rng.randrange(1, R)})
    H, w, counts, idx, shares, exp = bt.build(ctx)
    assert int((exp == N.REJECT).sum()) == 64
    _run_all(ctx, ks, (H, w, counts, idx, shares), exp, {s: 0 for s in SCHEDULES}, "every-position")


def test_ragged_instances(env):
    """Instances of 1, 2, 63, 65, 70 and 129 shares, each with its one wrong share in the last
    position of its ragged tile; all located."""
    ctx, rng, sks, pk, ks = env
    bt = Batch(rng, sks)
    for n in (1, 2, 63, 65, 70, 129):
        senders = []
        for lo in range(0, n, 64):
            senders += _senders(rng, min(64, n - lo))
        bt.add("n%d" % n, senders, delta={n - 1: rng.randrange(1, R)})
    H, w, counts, idx, shares, exp = bt.build(ctx)
    assert counts == [1, 2, 63, 65, 70, 129] and int((exp == N.REJECT).sum()) == 6
    _run_all(ctx, ks, (H, w, counts, idx, shares), exp, {s: 0 for s in SCHEDULES}, "ragged")


# two wrong shares of one 64-share tile: positions, and the exact checks each schedule ends with
# (a located single share needs none; an eighth with two wrong shares lists its 8 shares; the
# paired schedule without sub-tiles lists the whole tile, and a call of two tiles takes it by itself)
TWO_WRONG = {
    "one-eighth": ((9, 14), {AUTO: 64, PLAIN: 8, SUBS: 8, LEAVES: 64}),
    "two-eighths-of-a-quarter": ((3, 12), {AUTO: 64, PLAIN: 0, SUBS: 0, LEAVES: 64}),
    "two-quarters-of-a-half": ((5, 20), {AUTO: 64, PLAIN: 0, SUBS: 0, LEAVES: 64}),
    "both-halves": ((7, 40), {AUTO: 64, PLAIN: 0, SUBS: 0, LEAVES: 64}),
}


@pytest.mark.parametrize("case", sorted(TWO_WRONG))
def test_two_wrong_shares_under_the_split_levels(env, case):
    ctx, rng, sks, pk, ks = env
    (p, q), leaves = TWO_WRONG[case]
    bt = Batch(rng, sks)
    bt.add(case, _senders(rng, 64), delta={p: rng.randrange(1, R), q: rng.randrange(1, R)})
    bt.add("clean", _senders(rng, 64))
    H, w, counts, idx, shares, exp = bt.build(ctx)
    _run_all(ctx, ks, (H, w, counts, idx, shares), exp, leaves, case)


def _mixed_tile(rng, exclude=()):
    """A 64-share tile: a wrong share at 20 beside a broken encoding at 19, an unknown sender at 21,
    sender 13 twice (22 and 45: the later copy takes the exact path)."""
    senders = _senders(rng, 64, exclude=(13,) + tuple(exclude))
    senders[21] = N_KEYS + 5
    senders[22] = senders[45] = 13
    return senders


def test_mask_lanes_beside_summed_lanes(env):
    ctx, rng, sks, pk, ks = env
    bt = Batch(rng, sks)
    bt.add("mixed", _mixed_tile(rng), delta={20: rng.randrange(1, R)}, broken=(19,),
           expect={19: N.DECODE_ERR, 21: N.UNKNOWN_SENDER})
    H, w, counts, idx, shares, exp = bt.build(ctx)
    # the duplicate's later copy is the one leaf: the tile's one wrong summed share is located
    _run_all(ctx, ks, (H, w, counts, idx, shares), exp, {s: 1 for s in SCHEDULES}, "mixed")


def test_key_that_failed_to_load_beside_summed_lanes(env):
    ctx, rng, sks, pk, ks = env
    pk2 = np.array(pk, dtype=np.uint8).reshape(N_KEYS, 48).copy()
    pk2[BAD_KEY, 0] &= 0x7F
    ks2, bad = ctx.keyset_load(pk2.reshape(-1))
    assert bad == 1
    try:
        senders = _mixed_tile(rng, exclude=(BAD_KEY,))
        senders[18] = senders[63] = BAD_KEY
        bt = Batch(rng, sks)
        bt.add("badkey", senders, delta={20: rng.randrange(1, R)}, broken=(19,),
               expect={19: N.DECODE_ERR, 21: N.UNKNOWN_SENDER, 18: N.DECODE_ERR, 63: N.DECODE_ERR})
        H, w, counts, idx, shares, exp = bt.build(ctx)
        _run_all(ctx, ks2, (H, w, counts, idx, shares), exp, {s: 1 for s in SCHEDULES}, "badkey")
    finally:
        ctx.keyset_free(ks2)


def test_tracked_sender_beside_summed_lanes(env):
    """With tracking on: sender 31 lies in every instance of a first call and is tracked; in the
    second call its share (a wrong one) sits in the mixed tile and is checked exactly, outside
    the sums, beside the tile's other wrong share.  That share's sender is tracked from its first
    REJECT on, so the repeats of the call check it exactly as well."""
    ctx, rng, sks, pk, ks2 = env
    ks, bad = ctx.keyset_load(pk)  # a key set of its own: the tracking state stays out of the others
    assert bad == 0
    liar = 31
    ctx.set_sender_tracking(True)
    ctx.set_verify_mode(N.MODE_RLC)
    try:
        bt = Batch(rng, sks)
        for k in range(8):
            senders = _senders(rng, 64, exclude=(liar,))
            senders[(5 * k + 2) % 64] = liar
            bt.add("l%d" % k, senders, delta={(5 * k + 2) % 64: rng.randrange(1, R)})
        H, w, counts, idx, shares, exp = bt.build(ctx)
        st = ctx.verify_dec_shares(ks, H, w, counts, idx, shares)
        assert (st == exp).all()
        bt = Batch(rng, sks)
        senders = _mixed_tile(rng, exclude=(liar,))
        senders[33] = liar
        bt.add("tracked", senders, delta={20: rng.randrange(1, R), 33: rng.randrange(1, R)}, broken=(19,),
               expect={19: N.DECODE_ERR, 21: N.UNKNOWN_SENDER})
        H, w, counts, idx, shares, exp = bt.build(ctx)
        first = True
        for bits in (128, 64):
            ctx.set_rlc_bits(bits)
            for sched in SCHEDULES:
                ctx.set_check_schedule(sched)
                st = ctx.verify_dec_shares(ks, H, w, counts, idx, shares)
                assert (st == exp).all(), (bits, sched, np.nonzero(st != exp)[0], st[st != exp])
                # the tracked sender's share and the duplicate's later copy; from the second call
                # on also the share at 20
                print("leaves tracked", bits, sched, ctx.rlc_last_leaves())
                assert ctx.rlc_last_leaves() == (2 if first else 3), (bits, sched, ctx.rlc_last_leaves())
                first = False
        ctx.set_verify_mode(N.MODE_PER_SHARE)
        st = ctx.verify_dec_shares(ks, H, w, counts, idx, shares)
        assert (st == exp).all()
    finally:
        ctx.set_verify_mode(N.MODE_RLC)
        ctx.set_rlc_bits(128)
        ctx.set_check_schedule(N.CHECK_AUTO)
        ctx.set_sender_tracking(False)
        ctx.keyset_free(ks)
