"""Case tables and the Python-integer reference of the redundant 13 x 30 form (field.h FqW, curve.h
jacw_*), shared by tests/test_rrw_host.py (host build, both bounds asserted at every operation) and
tests/test_gpu_rrw.py (gfx950).  A value is the integer its 13 limbs spell (limbs may pass 2^30 - 1,
the value may pass p); sums, differences and normalisations are compared as exact integers, products
as the exact Montgomery quotient, points as affine points against oracle/bls12_381.py."""
import ctypes
import functools
import random

from oracle import bls12_381 as B
import devarith_cases as D
import rr_cases as RC

P = B.P
W, NL = 30, 13
M30 = (1 << W) - 1
RP = 1 << (W * NL)
RPI = pow(RP, -1, P)
SLACK = 3
ENTRY_V = 12                           # tools/rr_bounds.py ENTRY_V: the loop invariant, in units of p
X_ABS = 0xd201000000010000
(RW_ADD, RW_SUB, RW_NEG, RW_DBL, RW_NORM, RW_MUL, RW_SQR, RW_ZERO_SQR, RW_ZERO_ONE, RW_PT_DBL, RW_PT_ADD_AFF,
 RW_PT_ADD, RW_PT_EQ_AFF) = range(13)
OP_NAMES = ["add", "sub", "neg", "dbl", "norm", "mul", "sqr", "zero_sqr", "zero_one", "pt_dbl", "pt_add_aff",
            "pt_add", "pt_eq_aff"]
Z13 = [0] * NL


def spell(v):
    """canonical limbs (the top limb takes what is left)"""
    assert 0 <= v < 1 << (W * (NL - 1) + 32)
    return [(v >> (W * i)) & M30 for i in range(NL - 1)] + [v >> (W * (NL - 1))]


def val(ws):
    return sum(w << (W * i) for i, w in enumerate(ws))


def respell(ws, j, units=1):
    """the same integer with `units` of 2^30 moved from limb j + 1 down into limb j"""
    ws = list(ws)
    assert ws[j + 1] >= units
    ws[j + 1] -= units
    ws[j] += units << W
    return ws


def limb_max(vmax):
    """every limb below the top at the entry bound 2^30 + 2, the value as close below vmax as that allows"""
    low = [M30 + SLACK] * (NL - 1)
    return low + [(vmax - val(low + [0])) >> (W * (NL - 1))]


# ------------------------------------------------------------------------------- field cases
def field_table():
    rng = random.Random(0x3A)
    vmax = ENTRY_V * P
    ev = [0, 1, P - 1, P, P + 1, 2 * P - 1, vmax - 1, vmax] + [rng.randrange(vmax) for _ in range(4)]
    e = [spell(v) for v in ev] + [limb_max(vmax)]
    t = []
    for op in (RW_ADD, RW_SUB, RW_MUL):
        t += [(op, [a, b]) for a in e for b in e]
    t += [(op, [a]) for op in (RW_DBL, RW_SQR) for a in e]
    t += [(RW_NEG, [spell(v)]) for v in (0, 1, P - 1, P, 2 * P, 3 * P - 1, 3 * P, rng.randrange(3 * P))]
    # normalise: every limb below the top at 2^32 - 1, borrowed spellings of values up to 12p
    full = [0xFFFFFFFF] * (NL - 1)
    t.append((RW_NORM, [full + [(vmax - val(full + [0])) >> (W * (NL - 1))]]))
    t.append((RW_NORM, [full + [0]]))
    for v in ev[1:]:
        ws = spell(v)
        for j in range(NL - 1):
            if ws[j + 1] >= 3:
                ws = respell(ws, j, 3)
        t.append((RW_NORM, [ws]))
    # zero tests: k p and k p +- 1 for every k up to the value bound, canonical and with a borrow moved
    for k in range(ENTRY_V + 1):
        for dlt in (-1, 0, 1):
            v = k * P + dlt
            if not 0 <= v <= vmax:
                continue
            ws = spell(v)
            forms = [ws] + [respell(ws, j) for j in (0, 5, 11) if ws[j + 1] >= 1]
            for f in forms:
                t.append((RW_ZERO_SQR, [f]))
                t.append((RW_ZERO_ONE, [f]))
    return t


def field_ref(op, ins):
    """(exact integer or None, flag)"""
    a = val(ins[0])
    b = val(ins[1]) if len(ins) > 1 else 0
    if op == RW_ADD:
        return a + b, 0
    if op == RW_SUB:
        return a + 14 * P - b, 0
    if op == RW_NEG:
        return 4 * P - a, 0
    if op == RW_DBL:
        return 2 * a, 0
    if op == RW_NORM:
        return a, 0
    if op == RW_MUL:
        return RC.mont30(a * b), 0
    if op == RW_SQR:
        return RC.mont30(a * a), 0
    if op in (RW_ZERO_SQR, RW_ZERO_ONE):
        return None, int(a % P == 0)
    raise ValueError(op)


# ------------------------------------------------------------------------------- point cases
def jac_of(rng, pt, zval=None):
    """entry-bound Jacobian limbs of an affine point (None: infinity), each coordinate lifted by a
    random multiple of p below the value bound"""
    lift = lambda v: spell(v % P + P * rng.randrange(ENTRY_V))
    if pt is None:
        z = 0 if zval is None else zval
        return [lift(rng.randrange(P)), lift(rng.randrange(P)), spell(z)]
    z = rng.randrange(1, P)
    return [lift(pt[0] * z * z * RP), lift(pt[1] * z * z * z * RP), lift(z * RP)]


def aff_of(pt):
    return [spell(pt[0] * RP % P), spell(pt[1] * RP % P)]


def to_affine(out):
    x, y, z = [val(c) * RPI % P for c in out]
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


@functools.lru_cache(maxsize=None)
def points():
    rng = random.Random(0x9A)
    g = [B.g1_mul(B.G1_GEN, rng.randrange(1, B.R)) for _ in range(3)]
    t3 = (0, 2)
    t11 = RC._torsion_point(rng, 11)
    while True:
        out = B.g1_point_from_x(rng.randrange(P), False)
        if out and not B.g1_in_subgroup(out):
            break
    return g + [t3, t11, out]


def point_table():
    rng = random.Random(0x9B)
    pts = points()
    t = []
    infs = [jac_of(rng, None, z) for z in (0, P, 5 * P, ENTRY_V * P)]
    for p in pts:
        t.append((RW_PT_DBL, jac_of(rng, p), B.g1_add(p, p), None))
    for j in infs:
        t.append((RW_PT_DBL, j, None, None))
    for p in pts:
        for q in pts:
            # q == p: the doubling exit; q == -p: the infinity exit
            for qq in (q, B.g1_neg(q)) if q == p else (q,):
                want = B.g1_add(p, qq)
                t.append((RW_PT_ADD_AFF, jac_of(rng, p) + aff_of(qq), want, None))
                t.append((RW_PT_ADD, jac_of(rng, p) + jac_of(rng, qq), want, None))
    for p in pts[:3] + pts[3:4]:
        for j in infs[:3]:
            t.append((RW_PT_ADD_AFF, j + aff_of(p), p, None))          # addition into infinity
            t.append((RW_PT_ADD, j + jac_of(rng, p), p, None))
            t.append((RW_PT_ADD, jac_of(rng, p) + j, p, None))         # addition of infinity
    t.append((RW_PT_ADD, infs[1] + infs[2], None, None))
    for p in pts:
        ny = spell(4 * P - p[1] * RP % P)                               # fw_neg's spelling of -y
        t.append((RW_PT_EQ_AFF, jac_of(rng, p) + aff_of(p), None, 1))
        t.append((RW_PT_EQ_AFF, jac_of(rng, B.g1_neg(p)) + [aff_of(p)[0], ny], None, 1))
        t.append((RW_PT_EQ_AFF, jac_of(rng, p) + [aff_of(p)[0], ny], None, 0))
        t.append((RW_PT_EQ_AFF, jac_of(rng, B.g1_add(p, p)) + aff_of(p), None, 0))
    return t


@functools.lru_cache(maxsize=None)
def cases():
    ft = field_table()
    pt = point_table()
    return ft, [field_ref(op, ins) for op, ins in ft], pt


def run(fn, items):
    """fn(n, ops, in, out, flag) over [(op, [13-limb lists])] -> [(three 13-limb outputs, flag)]"""
    n = len(items)
    flat = []
    for _, ins in items:
        ins = list(ins) + [Z13] * (6 - len(ins))
        flat += [w for slot in ins for w in slot]
    out, flag = (ctypes.c_uint32 * (39 * n))(), (ctypes.c_uint32 * n)()
    rc = fn(n, D.u32([op for op, _ in items]), D.u32(flat), out, flag)
    assert rc == 0, "harness status %d" % rc
    o = list(out)
    return [([o[39 * i + 13 * k:39 * i + 13 * (k + 1)] for k in range(3)], flag[i]) for i in range(n)]


def check_fields(table, want, got):
    bad = []
    for (op, ins), (wi, wf), (outs, f) in zip(table, want, got):
        g = val(outs[0])
        ok = f == wf and (wi is None or g == wi)
        if op == RW_NORM:
            ok = ok and all(w <= M30 + SLACK for w in outs[0][:NL - 1])
        if op in (RW_MUL, RW_SQR):
            ok = ok and all(w <= M30 for w in outs[0][:NL - 1]) and g % P == val(ins[0]) * val(ins[-1]) * RPI % P
        if not ok:
            bad.append((OP_NAMES[op], [hex(val(x)) for x in ins], hex(g), f, wf))
    return bad


def check_points(table, got):
    """affine results against the oracle; every coordinate inside the entry bound again (closure)"""
    bad = []
    for (op, ins, want, wflag), (outs, f) in zip(table, got):
        if op == RW_PT_EQ_AFF:
            ok = f == wflag
        else:
            ok = to_affine(outs) == want
            ok = ok and all(max(c[:NL - 1]) <= M30 + SLACK and val(c) <= ENTRY_V * P for c in outs)
        if not ok:
            bad.append((OP_NAMES[op], to_affine(ins[:3]), want, f))
    return bad


# ------------------------------------------------------------------------------- the subgroup test
def walk(q):
    """An integer walk of [|x|] q, MSB first, as jacw_mul_x runs it: how often the accumulator is
    infinity at a doubling, infinity at an addition, equal to q (the addition's doubling exit) and
    equal to -q (its infinity exit)."""
    acc, n = None, dict(dbl_inf=0, add_inf=0, eq=0, neg=0)
    for b in range(63, -1, -1):
        if acc is None:
            n["dbl_inf"] += 1
        acc = B.g1_add(acc, acc) if acc is not None else None
        if (X_ABS >> b) & 1:
            if acc is None:
                n["add_inf"] += 1
            elif acc == q:
                n["eq"] += 1
            elif acc == B.g1_neg(q):
                n["neg"] += 1
            acc = B.g1_add(acc, q)
    return acc, n


@functools.lru_cache(maxsize=None)
def subgroup_cases():
    """[(tag, affine point)]: G1 points of both y signs, (0, +-2), a point of each prime order dividing
    the cofactor, one of order 33, P + T with P in G1 and T of order 3, an on-curve point outside G1"""
    rng = random.Random(0x5B)
    out = []
    for i in range(3):
        pt = B.g1_mul(B.G1_GEN, rng.randrange(1, B.R))
        out += [("G1 %d" % i, pt), ("G1 %d negated" % i, B.g1_neg(pt))]
    assert len({B.g1_compress(p)[0] & 0x20 for _, p in out}) == 2
    out += [("(0, 2)", (0, 2)), ("(0, -2)", (0, P - 2))]
    tors = {}
    for prime in (3, 11, 10177, 859267, 52437899):
        tors[prime] = RC._torsion_point(rng, prime)
        out.append(("order %d" % prime, tors[prime]))
    out.append(("order 33", B.g1_add(tors[3], tors[11])))
    out.append(("P + T", B.g1_add(out[0][1], tors[3])))
    while True:
        pt = B.g1_point_from_x(rng.randrange(P), False)
        if pt and not B.g1_in_subgroup(pt):
            break
    out.append(("outside G1", pt))
    return out


def run_subgroup(fn):
    """-> [(flags, t1 of the redundant form as an affine point or None, t1 of 12 x 32 likewise)]"""
    cs = subgroup_cases()
    n = len(cs)
    out, flags = (ctypes.c_uint32 * (72 * n))(), (ctypes.c_uint32 * n)()
    rc = fn(n, b"".join(B.g1_compress(p) for _, p in cs), out, flags)
    assert rc == 0, "harness status %d" % rc
    o = list(out)
    got = []
    for i in range(n):
        pts = []
        for h in range(2):
            x, y, z = [D.from_m(sum(w << (32 * k) for k, w in enumerate(o[72 * i + 36 * h + 12 * c:][:12])))
                       for c in range(3)]
            if z == 0:
                pts.append(None)
            else:
                zi = pow(z, -1, P)
                pts.append((x * zi * zi % P, y * zi * zi * zi % P))
        got.append((flags[i], pts[0], pts[1]))
    return got


def check_subgroup(got):
    bad = []
    for (tag, pt), (f, tw, tr) in zip(subgroup_cases(), got):
        want_t1 = B.g1_mul(pt, X_ABS)
        verdict = int(B.g1_in_subgroup(pt))
        if f != (1 | 4 * verdict | 8 * verdict | 16) or tw != want_t1 or tr != want_t1:
            bad.append((tag, f))
    return bad
