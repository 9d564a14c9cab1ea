"""Edge cases of the GPU hash-to-G2 path (hbtc_hash.hip: k_hash_cand, k_g2_clear_cofactor), built on
the CPU from oracle/rand04.py and oracle/threshold_crypto.py; nothing here imports the library
under test.

trace() restates G2::rand's draw loop over a ChaChaRng that counts its words and returns the
oracle hash together with a profile of the data-dependent branches the draw took: the fq_rand
rejections, the non-square redraws, the `greatest` bit against the root's order, and where in a
ChaCha block every next_u64 and the `greatest` word fell.  CLASSES names the branch classes the
GPU tests must reach; G2_COUNTERS / G1G2_COUNTERS are the messages b"hc<counter>" that
`python -m tests.hash_cases` (from the repository's root) found to populate every class (stored,
so that no run repeats the search and the set cannot drift).  tests/test_hash_cases.py holds the
conditions that keep tests/test_gpu_hash_edges.py from being vacuous: every class populated,
trace() == the oracle."""
import random

from oracle import bls12_381 as B
from oracle import threshold_crypto as TC
from oracle.rand04 import ChaChaRng

P = B.P


class _CountingRng(ChaChaRng):
    """oracle.rand04.ChaChaRng with a count of the words handed out (next_u64 draws through it)."""

    def __init__(self, seed_words):
        super().__init__(seed_words)
        self.words = 0

    def next_u32(self):
        self.words += 1
        return super().next_u32()


def _kernel_root(a):
    """The root fq2_sqrt (field.h) returns for a square a, in plain integers: (root, swapped).
    swapped: delta = (a0 + s) / 2 was a non-square, the root is (-a1 t / 2, x0)."""
    a0, a1 = a
    s = pow((a0 * a0 + a1 * a1) % P, (P + 1) // 4, P)
    half = B.fq_inv(2)
    d = (a0 + s) * half % P
    if d == 0:
        d = (a0 - s) * half % P
    t = pow(d, (P - 3) // 4, P)
    x0 = t * d % P
    if t * x0 % P == 1:
        return (x0, a1 * t * half % P), False
    return ((-a1 * t * half) % P, x0), True


def _lex_largest(y):
    """pairing 0.14 Ord for Fq2 (c1, then c0): y > -y."""
    return B.f2_lt(B.f2_neg(y), y)


def trace(seed_msg, with_hash=True):
    """(hash_g2(seed_msg) or None, profile) by G2::rand's loop written out once more.

    profile: attempts (non-square redraws + 1); rej[a] = (c0, c1) fq_rand rejections of attempt a;
    greatest; negated (the oracle's root was replaced by its negative); kernel_swapped /
    kernel_negated (the same for the root field.h's fq2_sqrt returns, and which of its two forms
    it took); hi_words (the stream index of the high word of every next_u64), greatest_words (of
    every `greatest` draw); words, blocks (ChaCha blocks generated).  with_hash False skips [h2]."""
    rng = _CountingRng(TC._seed_words(TC.sha3_256(seed_msg)))
    prof = {"attempts": 0, "rej": [], "hi_words": [], "greatest_words": []}
    while True:
        prof["attempts"] += 1
        x, rej = [], []
        for _ in range(2):
            r = 0
            while True:
                limbs = []
                for _ in range(6):
                    prof["hi_words"].append(rng.words)
                    limbs.append(rng.next_u64())
                limbs[5] &= 0xFFFFFFFFFFFFFFFF >> 3
                rep = sum(l << (64 * i) for i, l in enumerate(limbs))
                if rep < P:
                    break
                r += 1
            rej.append(r)
            x.append(rep * TC.R_MONT_INV % P)
        prof["rej"].append(tuple(rej))
        prof["greatest_words"].append(rng.words)
        greatest = rng.gen_bool()
        x = tuple(x)
        rhs = B.f2_add(B.f2_mul(B.f2_sqr(x), x), (4, 4))
        y = B.f2_sqrt(rhs)
        if y is None:
            continue
        negated = _lex_largest(y) != greatest
        if negated:
            y = B.f2_neg(y)
        ky, swapped = _kernel_root(rhs)
        assert B.f2_sqr(ky) == rhs and ky in (y, B.f2_neg(y))
        prof.update(greatest=greatest, negated=negated, kernel_swapped=swapped,
                    kernel_negated=_lex_largest(ky) != greatest, words=rng.words,
                    blocks=(rng.words + 15) // 16)
        if not with_hash:
            return None, prof
        q = B.g2_mul((x, y), B.H2)
        if q is not None:
            return q, prof


def _any_call(comp, pred):
    return lambda p: any(pred(r[comp]) for r in p["rej"])


CLASSES = {
    "attempts = 1": lambda p: p["attempts"] == 1,
    "attempts = 2": lambda p: p["attempts"] == 2,
    "attempts = 3": lambda p: p["attempts"] == 3,
    "attempts >= 6": lambda p: p["attempts"] >= 6,
    "rejection in an attempt that fails the square test": lambda p: any(sum(r) for r in p["rej"][:-1]),
    "u64 high word at word 15": lambda p: any(w % 16 == 15 for w in p["hi_words"]),
    "greatest word at word 15": lambda p: any(w % 16 == 15 for w in p["greatest_words"]),
    "greatest word at word 0": lambda p: any(w % 16 == 0 for w in p["greatest_words"]),
    "blocks >= 8": lambda p: p["blocks"] >= 8,
    # the two forms of fq2_sqrt's root (field.h) on the accepted draw
    "kernel root from a square delta": lambda p: not p["kernel_swapped"],
    "kernel root from a non-square delta": lambda p: p["kernel_swapped"],
}
for _c, _name in ((0, "c0"), (1, "c1")):
    CLASSES["%s rejections = 0" % _name] = _any_call(_c, lambda r: r == 0)
    CLASSES["%s rejections = 1" % _name] = _any_call(_c, lambda r: r == 1)
    CLASSES["%s rejections = 2" % _name] = _any_call(_c, lambda r: r == 2)
    CLASSES["%s rejections >= 3" % _name] = _any_call(_c, lambda r: r >= 3)
for _g in (False, True):
    for _n in (False, True):
        CLASSES["greatest = %d, y negated = %d" % (_g, _n)] = \
            lambda p, g=_g, n=_n: p["greatest"] == g and p["negated"] == n
        CLASSES["greatest = %d, kernel's y negated = %d" % (_g, _n)] = \
            lambda p, g=_g, n=_n: p["greatest"] == g and p["kernel_negated"] == n


def is_light(p):
    """Finishes on the first draw with no rejection: the lanes beside a heavy one."""
    return p["attempts"] == 1 and p["rej"] == [(0, 0)]


def is_heavy(p):
    return p["attempts"] >= 6


N_LIGHT = 4  # distinct light messages kept for the batch layouts

# ------------------------------------------------------------------ the stored counters
U_MULTIPLES = 7  # hash_g1_g2's u for counter c: [1 + c % 7] G1


def g2_msg(counter):
    return b"hc%d" % counter


def g1g2_input(counter):
    """(compressed u, v) of counter."""
    return B.g1_compress(B.g1_mul(B.G1_GEN, 1 + counter % U_MULTIPLES)), b"hc%d" % counter


def g1g2_seed_msg(u_c48, v):
    """The message hash_g1_g2 hands to hash_g2."""
    return (TC.sha3_256(v) if len(v) > 64 else bytes(v)) + bytes(u_c48)


# found by mine() below: greedy, in counter order, a counter kept when it is the first of a class
# or one of the first N_LIGHT light ones
G2_COUNTERS = [0, 1, 2, 3, 4, 5, 6, 8, 9, 15, 17, 18, 19, 41, 352]
G1G2_COUNTERS = [0, 1, 2, 3, 5, 6, 8, 9, 12, 33, 39, 73, 119]


def mine(seed_msg_of, limit=200000):
    """The counters, in order, that first populate a class of CLASSES or are among the first
    N_LIGHT light draws; stops when every class has one."""
    missing, light, keep = set(CLASSES), 0, []
    for c in range(limit):
        _, p = trace(seed_msg_of(c), with_hash=False)
        hit = {k for k in missing if CLASSES[k](p)}
        take_light = is_light(p) and light < N_LIGHT
        if hit or take_light:
            keep.append(c)
            missing -= hit
            light += is_light(p)
        if not missing and light >= N_LIGHT:
            return keep
    raise RuntimeError("classes left: %s" % sorted(missing))


# ------------------------------------------------------------------ the cases
G2_LENGTHS = [0, 1, 7, 8, 9, 135, 136, 137, 271, 272, 273, 408, 1000]
G1G2_LENGTHS = [0, 1, 63, 64, 65, 66, 135, 136, 137, 272, 273]


def _bytes(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def g2_cases():
    """[(name, msg)]: the mined draws, then the length cases."""
    rng = random.Random(0x6832)
    return [("hc%d" % c, g2_msg(c)) for c in G2_COUNTERS] + \
           [("len %d" % n, _bytes(rng, n)) for n in G2_LENGTHS]


def g1g2_cases():
    """[(name, compressed u, v)]: the mined draws, then the |v| cases."""
    rng = random.Random(0x6731)
    out = [("hc%d" % c,) + g1g2_input(c) for c in G1G2_COUNTERS]
    for k, n in enumerate(G1G2_LENGTHS):
        out.append(("|v| %d" % n, B.g1_compress(B.g1_mul(B.G1_GEN, 11 + k)), _bytes(rng, n)))
    return out


_memo = {}


def g2_point(msg):
    """oracle hash_g2(msg) as a point, computed once per process."""
    msg = bytes(msg)
    if msg not in _memo:
        _memo[msg] = TC.hash_g2(msg)
    return _memo[msg]


def want_g2(msg):
    """compressed oracle hash_g2(msg)."""
    return B.g2_compress(g2_point(msg))


def want_g1g2(u_c48, v):
    """compressed oracle hash_g1_g2(u, v); TC.hash_g1_g2 is this on the decoded u
    (tests/test_hash_cases.py asserts it on every case)."""
    return want_g2(g1g2_seed_msg(u_c48, v))


BATCH_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 129]
HEAVY_SIZES = [33, 65, 129]


def layouts(profiles, empty):
    """{name: [case index]} for cases whose draw profiles are `profiles` (one per case, in order)
    and whose empty message is case `empty`.

    n = 1 .. 64: the cases in rotation, started at a different one per size, so every case sits in
    several batches at different lanes.  n = 33, 65, 129 (one item past k_g2_clear_cofactor's
    32-candidate and k_hash_cand's 64-message workgroups): light cases in rotation with the
    heaviest draw at item 0, at the last item and at lane 32 of the last full block (item 16 of
    33), so one lane loops many times beside lanes that finish on the first draw.  Two batches of
    empty messages: first, last and adjacent among others; and nothing else."""
    n_cases = len(profiles)
    light = [i for i, p in enumerate(profiles) if is_light(p)]
    heavy = max(range(n_cases), key=lambda i: profiles[i]["attempts"])
    assert len(light) >= N_LIGHT and is_heavy(profiles[heavy])
    out = {}
    for k, n in enumerate(BATCH_SIZES):
        if n in HEAVY_SIZES:
            idx = [light[i % len(light)] for i in range(n)]
            mid = (n - 1) // 64 * 64 - 32 if n > 64 else n // 2
            for at in (0, mid, n - 1):
                idx[at] = heavy
        else:
            idx = [(7 * k + i) % n_cases for i in range(n)]
            if n <= 2:
                idx[0] = heavy
        out["n = %d" % n] = idx
    others = [i for i in range(n_cases) if i != empty]
    out["empty first, last and adjacent"] = [empty, empty, others[0], others[1], empty, empty, empty,
                                             others[2], empty]
    out["only empty"] = [empty] * 33
    return out


if __name__ == "__main__":
    print("G2_COUNTERS =", mine(g2_msg))
    print("G1G2_COUNTERS =", mine(lambda c: g1g2_seed_msg(*g1g2_input(c))))
