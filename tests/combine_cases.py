"""Case tables and the Python-integer reference of the Lagrange combines (PublicKeySet::
combine_signatures, src/coin.rs:185-191; PublicKeySet::decrypt, src/threshold_decryption.rs:
181-185), shared by tests/test_combine_cases.py (CPU) and tests/test_gpu_combine_paths.py (gfx950).

On the device "the first t accepted shares, lambda_i at 0 over x = idx + 1" is four routes, picked
by the data of the call: the small combine (hbtc_comb.hip), k_select, the factorial tables
(k_lagrange_fact) and the generic k_lagrange_x / _den / _inv.  The tables here put one instance on
every side of every switch between them; route_of() restates the switch conditions so that the CPU
test can assert that each case sits where its name says.

An item is (idx, status, s): the node index, the verifier's status of the share and the share's
scalar (the share is [s] G); s = None stands for an undecodable encoding (tests/golden/codec.json).
The s are independent random non-zero scalars, NOT evaluations of one polynomial: any single wrong
lambda_i moves sum lambda_i s_i, and no other route reaches the same value by accident.
"""
import collections
import functools
import math
import random

from oracle import bls12_381 as B
from oracle import threshold_crypto as TC

R = B.R

# Statuses of include/hbtc.h (hbbft_amd/_native.py restates them too).
ACCEPT, REJECT, DECODE_ERR, NOT_ENOUGH_SHARES, DUPLICATE_ENTRY = 0, 1, 2, 5, 6

# The constants this module mirrors, all in one place.  hbtc_msm.hip: k_select ballots BALLOT items
# at a time; k_lagrange_fact takes t <= LG_FACT_TMAX (its xs[] LDS array) and M - t <=
# LG_FACT_RMAX gaps (its rs[] LDS array); k_lagrange_inv walks ceil(t / LG_BS) terms per thread of
# its LG_BS threads.  hbtc_api.hip / hbtc_kernels.h: combines of t <= COMB_SMALL_T go to
# hbtc_comb.hip, and the factorial tables hold 0! .. FACT_N!.
BALLOT = 64
COMB_SMALL_T = 64
LG_FACT_RMAX = 256
LG_FACT_TMAX = 4096
LG_BS = 256
FACT_N = 65535

T_IDX = 70  # the index and the selection cases: just past COMB_SMALL_T
CHUNK_TS = (65, 255, 256, 257, 511, 512, 513, 769)
SMALL_TS = (8, 64)

Case = collections.namedtuple("Case", "name t items verified route status")
# verified: the first t ACCEPTed items are selected (hbtc_combine_*_verified_dev); else the first t
# route: "fact" / "generic" with the tables on (None: the coefficients are never used)
# status: the instance status the reference must give


# ------------------------------------------------------------------------------------ reference
def select(case):
    """The selected items: the first t (verified: the first t whose status is ACCEPT)."""
    its = [it for it in case.items if not case.verified or it[1] == ACCEPT]
    return its[:case.t]


def lagrange(xs):
    """lambda_i at 0 over the distinct integers xs, mod r: prod_{j != i} x_j / (x_j - x_i).  Every
    denominator is a product over chunks of 32 differences, reduced mod r per chunk."""
    P = 1
    for x in xs:
        P = P * x % R
    out = []
    for i, xi in enumerate(xs):
        diffs = [xj - xi for j, xj in enumerate(xs) if j != i]
        q = xi % R
        for c in range(0, len(diffs), 32):
            q = q * (math.prod(diffs[c:c + 32]) % R) % R
        out.append(P * pow(q, -1, R) % R)
    return out


Ref = collections.namedtuple("Ref", "status xs lam k")


@functools.lru_cache(maxsize=None)
def _reference(case):
    sel = select(case)
    xs = [idx + 1 for idx, _, _ in sel]  # integers: no 32-bit wrap
    if len(sel) < case.t:
        return Ref(NOT_ENOUGH_SHARES, xs, None, None)
    if any(s is None for _, _, s in sel):  # the share never decodes: nothing to interpolate
        return Ref(DECODE_ERR, xs, None, None)
    if len(set(xs)) < len(xs):
        return Ref(DUPLICATE_ENTRY, xs, None, None)
    lam = lagrange(xs)
    return Ref(ACCEPT, xs, lam, sum(l * s for l, (_, _, s) in zip(lam, sel)) % R)


def reference(case):
    """Ref(status, selected x, lambda, sum lambda_i s_i mod r) of one instance, in threshold_crypto's
    order: NOT_ENOUGH_SHARES, then (a selected share that does not decode: DECODE_ERR, as
    k_msm_final), then DUPLICATE_ENTRY, then ACCEPT."""
    return _reference(case)


@functools.lru_cache(maxsize=None)
def expected(case, group):
    """(compressed point, parity bit, status) of the instance in G1 (group 1) / G2 (group 2): one
    oracle multiplication; zero bytes and parity 0 for a failed instance."""
    ref = reference(case)
    if ref.status != ACCEPT:
        return bytes(48 if group == 1 else 96), 0, ref.status
    if group == 1:
        return B.g1_compress(B.g1_mul(B.G1_GEN, ref.k)), 0, ACCEPT
    p = B.g2_mul(B.G2_GEN, ref.k)
    return B.g2_compress(p), int(TC.signature_parity(p)), ACCEPT


# ------------------------------------------------------------------------------- route conditions
def route_of(case):
    """The Lagrange route of an instance with the factorial tables on, restated from k_select /
    k_lagrange_fact: None when fewer than t are selected (done[k] = 1, nothing computed), "fact"
    when the selected x, as 32-bit words, are non-zero and strictly increasing with t <=
    LG_FACT_TMAX, M - t <= LG_FACT_RMAX and M <= FACT_N (M = the largest x), else "generic"."""
    sel = select(case)
    if len(sel) < case.t:
        return None
    x32 = [(idx + 1) & 0xffffffff for idx, _, _ in sel]
    inc = all(a != 0 and a < b for a, b in zip(x32, x32[1:])) and x32[0] != 0
    M = x32[-1]
    if inc and case.t <= LG_FACT_TMAX and M - case.t <= LG_FACT_RMAX and M <= FACT_N:
        return "fact"
    return "generic"


def inv_chunk(t):
    """Terms per thread of k_lagrange_inv."""
    return (t + LG_BS - 1) // LG_BS


# ------------------------------------------------------------------------------------ the tables
def _rng(name):
    return random.Random("combine_cases:" + name)


def _plain(name, t, xs, route, status, filler=()):
    """An instance in the plain form: the items at x = xs (all selected when len(xs) == t), then the
    filler x (never selected)."""
    rng = _rng(name)
    items = tuple((x - 1, ACCEPT, rng.randrange(1, R)) for x in list(xs) + list(filler))
    return Case(name, t, items, False, route, status)


def _filler(xs, n=2):
    """n small x outside xs."""
    out, used, x = [], set(xs), 3
    while len(out) < n:
        if x not in used:
            out.append(x)
        x += 7
    return out


def _scatter(name, t, M):
    """t increasing x in [1, M] with the largest M, seeded."""
    return sorted(_rng(name + ":x").sample(range(1, M), t - 1)) + [M]


LARGE_IDX = (65534, 65535, 10 ** 6, 2 ** 32 - 2, 2 ** 32 - 1)


def _index_shapes(t):
    """name -> (selected x, route with the tables on, status, filler x or None for the default)."""
    dense = list(range(1, t + 1))
    swap = list(dense)
    swap[t // 2], swap[t // 2 + 1] = swap[t // 2 + 1], swap[t // 2]
    shuf = list(dense)
    _rng("shuffle%d" % t).shuffle(shuf)
    assert shuf != dense
    large = list(range(1, t - len(LARGE_IDX) + 1)) + [i + 1 for i in LARGE_IDX]
    dup_adj = list(dense)
    dup_adj[t // 4 + 1] = dup_adj[t // 4]
    dup_ends = list(dense)
    dup_ends[-1] = dup_ends[0]
    short = list(range(1, t))
    if t > 2:
        short[-1] = short[1]
    return {
        "dense": (dense, "fact", ACCEPT, None),
        "first_x_2": (list(range(2, t + 2)), "fact", ACCEPT, None),
        "gaps256_block": (list(range(1, t)) + [t + 256], "fact", ACCEPT, None),
        "gaps256_scattered": (_scatter("g256", t, t + 256), "fact", ACCEPT, None),
        "gaps257_scattered": (_scatter("g257", t, t + 257), "generic", ACCEPT, None),
        "gaps257_front": (list(range(258, t + 258)), "generic", ACCEPT, None),
        "large": (large, "generic", ACCEPT, None),
        "decreasing": (dense[::-1], "generic", ACCEPT, None),
        "swap": (swap, "generic", ACCEPT, None),
        "shuffle": (shuf, "generic", ACCEPT, None),
        "dup_adjacent": (dup_adj, "generic", DUPLICATE_ENTRY, None),
        "dup_first_last": (dup_ends, "generic", DUPLICATE_ENTRY, None),
        # the repeat sits at position t + 1: it is not selected
        "dup_past_t": (dense, "fact", ACCEPT, [dense[t // 3], t + 9]),
        # t - 1 items holding a repeat: NotEnoughShares comes first
        "short_dup": (short, None, NOT_ENOUGH_SHARES, []),
    }


def _index_case(prefix, t, name):
    xs, route, status, fill = _index_shapes(t)[name]
    return _plain("%s%s" % (prefix, name), t, xs, route, status,
                  _filler(xs) if fill is None else fill)


INDEX_NAMES = ("dense", "first_x_2", "gaps256_block", "gaps256_scattered", "gaps257_scattered",
               "gaps257_front", "large", "decreasing", "swap", "shuffle", "dup_adjacent",
               "dup_first_last", "dup_past_t", "short_dup")
BOUNDARY_NAMES = ("dense", "gaps256_block", "gaps256_scattered", "gaps257_scattered",
                  "gaps257_front", "decreasing")


@functools.lru_cache(maxsize=None)
def index_cases():
    """The index cases, every one at t = T_IDX."""
    return tuple(_index_case("idx_", T_IDX, n) for n in INDEX_NAMES)


@functools.lru_cache(maxsize=None)
def chunk_cases():
    """{t: (sparse[, dense])}: sparse increasing x with M - t > LG_FACT_RMAX (generic under either
    setting: k_lagrange_inv at chunk 1, 2, 3 and 4 with empty and ragged last chunks), and beside
    it a dense instance the factorial kernel takes, so done[] is mixed at every chunk size.  (No
    dense one at t = 255, 256, 257: the oracle's lagrange_at_zero inverts per pair of x, which
    takes the CPU test several seconds per instance of that size.)"""
    out = {}
    for t in CHUNK_TS:
        xs = _scatter("chunk%d" % t, t, 3 * t + 400)
        out[t] = (_plain("chunk_%d_sparse" % t, t, xs, "generic", ACCEPT, _filler(xs)),)
        if t not in (255, 256, 257):
            out[t] += (_plain("chunk_%d_dense" % t, t, range(1, t + 1), "fact", ACCEPT, [t + 5]),)
    return out


@functools.lru_cache(maxsize=None)
def limit_cases():
    """The t limit of the factorial kernel (G1 only, one instance each): t = 4096 over x = 1..4352
    with 256 scattered gaps, the factorial route at its real table top; t = 4097 dense, the generic
    route at chunk 17."""
    t = LG_FACT_TMAX
    return (_plain("limit_4096_fact", t, _scatter("limit", t, t + LG_FACT_RMAX), "fact", ACCEPT),
            _plain("limit_4097_generic", t + 1, range(1, t + 2), "generic", ACCEPT))


def _verified(name, t, statuses, route, status, idx=None, bad=()):
    """An instance in the verified form: item p has idx[p] (default p), statuses[p] and a valid
    share, but for the positions in `bad`, whose encoding does not decode."""
    rng = _rng(name)
    idx = list(range(len(statuses))) if idx is None else idx
    items = tuple((i, st, None if p in bad else rng.randrange(1, R))
                  for p, (i, st) in enumerate(zip(idx, statuses)))
    for p in bad:
        assert statuses[p] != ACCEPT  # the combine trusts ACCEPT: such a share must be valid
    return Case(name, t, items, True, route, status)


def _statuses(name, n, t, tth, lo=0):
    """n statuses whose t-th ACCEPT sits at position tth, none before position lo; the others are
    REJECT or DECODE_ERR before it and any of the three behind it."""
    rng = _rng(name + ":st")
    acc = set(rng.sample(range(lo, tth), t - 1)) | {tth}
    st = [ACCEPT if p in acc else rng.choice((REJECT, DECODE_ERR)) for p in range(tth + 1)]
    st += [rng.choice((ACCEPT, REJECT, DECODE_ERR)) for _ in range(n - tth - 1)]
    assert len(st) == n and st[:tth + 1].count(ACCEPT) == t and st[tth] == ACCEPT
    return st


def tth_position(case):
    """Position (0-based, within the instance) of the t-th selected item, or None."""
    pos = [p for p, it in enumerate(case.items) if not case.verified or it[1] == ACCEPT]
    return pos[case.t - 1] if len(pos) >= case.t else None


@functools.lru_cache(maxsize=None)
def selection_cases():
    """The selection cases of k_select: the verified form at t = T_IDX (but for the last one).  A
    t-th accepted item at position p needs t <= p + 1, so positions 63 and 64 cannot be met at
    t = 70: they are in small_cases() at t = 8 and t = 64, which HBTC_COMB_SMALL=0 sends through
    k_select as well."""
    t = T_IDX
    A = ACCEPT
    out = [
        # item counts: fewer than t items in one ballot / one item into the second
        _verified("sel_n64", t, [A] * 64, None, NOT_ENOUGH_SHARES),
        _verified("sel_n65", t, [A] * 65, None, NOT_ENOUGH_SHARES),
        # the t-th accepted item last of the second ballot / first of the third
        _verified("sel_n128_tth127", t, _statuses("n128", 128, t, 127), "fact", ACCEPT),
        _verified("sel_n129_tth128", t, _statuses("n129", 129, t, 128), "fact", ACCEPT),
        _verified("sel_n200_tth128", t, _statuses("n200", 200, t, 128), "fact", ACCEPT),
        _verified("sel_n200_tth127", t, _statuses("n200b", 200, t, 127), "fact", ACCEPT),
        # a whole ballot rejected
        _verified("sel_first64_rejected", t, _statuses("f64", 200, t, 150, lo=64), "fact", ACCEPT),
        # exactly t accepted, the last item being the t-th
        _verified("sel_exact_last", t, _statuses("exact", 100, t, 99), "fact", ACCEPT),
        # t - 1 accepted
        _verified("sel_t_minus_1", t, _statuses("tm1", 121, t - 1, 120) + [REJECT] * 7, None,
                  NOT_ENOUGH_SHARES),
    ]
    # a repeat whose first copy is REJECT: only the second one is selected
    st = [A] * 80
    st[5] = REJECT
    idx = list(range(80))
    idx[40] = idx[5]
    out.append(_verified("sel_dup_first_rejected", t, st, "generic", ACCEPT, idx=idx))
    # an undecodable encoding under a non-ACCEPT status in front of the selection, another behind
    st = [DECODE_ERR] + [A] * t + [REJECT, A]
    out.append(_verified("sel_bad_around", t, st, "fact", ACCEPT, bad=(0, t + 1)))
    # the same encoding selected, in the plain form
    c = _plain("sel_bad_selected_plain", t, range(1, t + 1), "fact", DECODE_ERR, [t + 3])
    items = list(c.items)
    items[7] = (items[7][0], ACCEPT, None)
    out.append(c._replace(items=tuple(items)))
    return tuple(out)


SMALL_INDEX_NAMES = ("dense", "decreasing", "shuffle", "large", "dup_first_last", "dup_past_t",
                     "short_dup")


@functools.lru_cache(maxsize=None)
def small_cases():
    """{t: cases} for t = 8 and t = 64 (hbtc_comb.hip: its own selection and its own lambda loop;
    the same cases run through k_select and the Lagrange kernels under HBTC_COMB_SMALL=0): the index
    cases that do not need t > 64, in the plain form, and selection cases in the verified form with
    64, 65 and 129 items and the t-th accepted item at positions 63, 64 and 128."""
    out = {}
    for t in SMALL_TS:
        p = "small%d_" % t
        cs = [_index_case(p, t, n) for n in SMALL_INDEX_NAMES]
        cs += [
            _verified(p + "sel_n64_tth63", t, _statuses(p + "n64", 64, t, 63), "fact", ACCEPT),
            _verified(p + "sel_n65_tth64", t, _statuses(p + "n65", 65, t, 64), "fact", ACCEPT),
            _verified(p + "sel_n129_tth128", t, _statuses(p + "n129", 129, t, 128, lo=64), "fact",
                      ACCEPT),
            _verified(p + "sel_t_minus_1", t, _statuses(p + "tm1", 65, t - 1, 64), None,
                      NOT_ENOUGH_SHARES),
        ]
        st = [REJECT] + [ACCEPT] * t
        idx = list(range(t + 1))
        idx[t] = idx[0]
        cs.append(_verified(p + "sel_dup_first_rejected", t, st, "generic", ACCEPT, idx=idx))
        out[t] = tuple(cs)
    return out


def all_cases():
    out = list(index_cases())
    for pair in chunk_cases().values():
        out += pair
    out += limit_cases() + selection_cases()
    for cs in small_cases().values():
        out += cs
    return out
