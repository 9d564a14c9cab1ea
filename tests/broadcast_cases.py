"""Edge cases of the Reliable Broadcast kernels (hbtc_bcast.hip: k_gf_apply, k_merkle_tree,
k_merkle_validate) and of the device-pointer forms' ordering, built on the CPU from seeded
random / numpy.  Every expected byte and verdict comes from hashlib.sha3_256, from
oracle/broadcast.py (merkle_levels, merkle_proof, proof_validate, rs_encode, rs_reconstruct) or
from the Reed-Solomon round trip; nothing here imports the library under test.
tests/test_broadcast_cases.py holds the conditions that keep the GPU tests
(tests/test_gpu_broadcast_edges.py) from being vacuous."""
import hashlib
import itertools
import random

import numpy as np

from oracle import broadcast as B

RATE = 136          # SHA3-256 rate in bytes
SLACK = 64          # bytes kept free on both sides of every device buffer
GUARD = 0xA5
ALIGNS = (0, 1, 2, 3)
ACCEPT, REJECT, NOT_ENOUGH = 0, 1, 5  # HBTC_ACCEPT / HBTC_REJECT / HBTC_NOT_ENOUGH_SHARES (include/hbtc.h)


def _bytes(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


# ------------------------------------------------------------------ A / B: k_merkle_tree
# A: leaf lengths by SHA3 padding class.  rem = len % 136: rem == 0 is the empty last block and the
# `while (len - off >= RATE)` boundary; rem in 128..135 puts the 0x06 into the last rate word (at
# 135 onto the byte of the 0x80); 1..9 and 63..65 are the partial-word masks of load_block; 271..273
# and 407..409 the same boundaries after one and two full blocks.
LEAF_LENS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127] + list(range(128, 138)) + \
            [143, 144, 145, 271, 272, 273, 407, 408, 409]
LEAF_N_LEAVES, LEAF_N_INST = 5, 3  # 5 -> 3 -> 2 -> 1: an odd digest is carried up on two levels

# B: tree shapes.  One workgroup has 128 lane pairs: 129 .. 256 leaves take the second trip of the
# leaf loop (partial at 129 and 255, full at 256), 257 the third and the second trip of level 1.
TREE_N_LEAVES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 33, 127, 128, 129, 255, 256, 257]
TREE_LEAF_LEN, TREE_N_INST = 3, 2


def tree_digests(values):
    """Every digest of MerkleTree::from_vec in the library's layout: level 0 (the leaves), level
    1, ..., the root last; an odd last digest is carried up unhashed (merkle.rs:19-32)."""
    levels, root = B.merkle_levels(values)
    return [d for lvl in levels for d in lvl] + [root]


def tree_case(n_leaves, leaf_len, n_inst, seed):
    """(leaves uint8[n_inst, n_leaves, leaf_len], digests uint8[n_inst, n_dig, 32])."""
    rng = np.random.default_rng(seed)
    leaves = rng.integers(0, 256, (n_inst, n_leaves, leaf_len), dtype=np.uint8)
    dig = [tree_digests([bytes(v) for v in inst]) for inst in leaves]
    return leaves, np.frombuffer(b"".join(b"".join(d) for d in dig), np.uint8).reshape(n_inst, -1, 32).copy()


def leaf_case(leaf_len):
    return tree_case(LEAF_N_LEAVES, leaf_len, LEAF_N_INST, 1000 + leaf_len)


def shape_case(n_leaves):
    return tree_case(n_leaves, TREE_LEAF_LEN, TREE_N_INST, 2000 + n_leaves)


# ------------------------------------------------------------------ C: k_merkle_validate
PROOF_N_NODES = [1, 2, 3, 5, 6, 7, 9, 13, 17, 33, 100, 255, 256]
VALUE_LENS = [0, 1, 135, 136, 137, 272, 300]  # cycled over the leaves: their sum is 981 = 1 mod 4
BATCH_SIZES = [1, 31, 32, 33, 65]             # 32 proofs per workgroup
# a digest bit at an even position of its 64-bit word lives in lane 0 of the pair, at an odd
# position in lane 1: (byte, bit) of the first and last word's bits 0 and 1
HALF_BITS = {"w0_even": (0, 0), "w0_odd": (0, 1), "w3_even": (24, 0), "w3_odd": (24, 1)}
TAMPER_CLASSES = (["value_first", "value_last", "value_135", "value_136", "value_short", "value_long",
                   "index_xor1", "index_plus_pow2", "index_n_nodes", "digests_swapped", "digest_bit",
                   "digest_dropped", "digest_appended"] +
                  ["root_" + k for k in HALF_BITS] + ["sibling_" + k for k in HALF_BITS])


def _flip(b, pos, mask=1):
    return b[:pos] + bytes([b[pos] ^ mask]) + b[pos + 1:]


def tampers(proof, n_nodes, rng):
    """[(class, proof)] of one valid proof; a tamper the proof has no room for is left out."""
    v, i, d, r = proof
    out = []
    if v:
        out.append(("value_first", (_flip(v, 0, 0x80), i, d, r)))
        out.append(("value_last", (_flip(v, len(v) - 1), i, d, r)))
        out.append(("value_short", (v[:-1], i, d, r)))
    if len(v) > 135:
        out.append(("value_135", (_flip(v, 135, 0x10), i, d, r)))
    if len(v) > 136:
        out.append(("value_136", (_flip(v, 136, 0x04), i, d, r)))
    out.append(("value_long", (v + b"\0", i, d, r)))
    out.append(("index_xor1", (v, i ^ 1, d, r)))
    for lvl in range(32):
        if i + (1 << lvl) < 1 << 32:
            out.append(("index_plus_pow2", (v, i + (1 << lvl), d, r)))
    out.append(("index_n_nodes", (v, n_nodes, d, r)))
    if len(d) >= 2:
        out.append(("digests_swapped", (v, i, [d[1], d[0]] + d[2:], r)))
    for lvl in range(len(d)):
        bit = rng.randrange(256)
        out.append(("digest_bit", (v, i, d[:lvl] + [_flip(d[lvl], bit // 8, 1 << (bit % 8))] + d[lvl + 1:], r)))
    if d:
        out.append(("digest_dropped", (v, i, d[:-1], r)))
    out.append(("digest_appended", (v, i, d + [_bytes(rng, 32)], r)))
    for name, (byte, bit) in HALF_BITS.items():
        out.append(("root_" + name, (v, i, d, _flip(r, byte, 1 << bit))))
        if d:
            s = rng.randrange(len(d))
            out.append(("sibling_" + name, (v, i, d[:s] + [_flip(d[s], byte, 1 << bit)] + d[s + 1:], r)))
    return out


_PROOF_CACHE = {}


def proof_case(n_nodes):
    """One tree of n_nodes values (lengths cycling VALUE_LENS): every index's valid proof, then the
    tampers of every fifth index and of the last one.  Returns [(class, proof, verdict)] with
    class "valid" for the untampered ones and verdict = Proof::validate by the oracle."""
    if n_nodes not in _PROOF_CACHE:
        rng = random.Random(3000 + n_nodes)
        values = [_bytes(rng, VALUE_LENS[i % len(VALUE_LENS)]) for i in range(n_nodes)]
        levels, root = B.merkle_levels(values)
        valid = [B.merkle_proof(levels, root, values, i) for i in range(n_nodes)]
        items = [("valid", pr) for pr in valid]
        for i in sorted(set(range(0, n_nodes, 5)) | {n_nodes - 1}):
            items += tampers(valid[i], n_nodes, rng)
        _PROOF_CACHE[n_nodes] = [(c, pr, bool(B.proof_validate(pr, n_nodes))) for c, pr in items]
    return _PROOF_CACHE[n_nodes]


def last_leaf_at_n_nodes(n_nodes):
    """The proof of the last leaf submitted with index = n_nodes, and the oracle's verdict."""
    items = proof_case(n_nodes)
    last = items[n_nodes - 1][1]
    got = [(pr, ok) for c, pr, ok in items if c == "index_n_nodes" and pr[0] == last[0] and pr[2] == last[2]]
    return got[-1]


def batch_case(size):
    """`size` proofs drawn from the n_nodes = 13 case, valid and tampered mixed."""
    items = proof_case(13)
    rng = random.Random(4000 + size)
    pick = rng.sample(range(len(items)), size - 1) if size > 1 else []
    return 13, [items[rng.randrange(13)]] + [items[j] for j in pick]  # at least one ACCEPT


def pack_proofs(proofs):
    """The flat arrays of hbtc_merkle_validate: value_off u64[n + 1], values u8, index u32[n],
    digest_off u32[n + 1], digests u8, roots u8[32 n]."""
    n = len(proofs)
    voff = np.zeros(n + 1, np.uint64)
    voff[1:] = np.cumsum([len(p[0]) for p in proofs])
    doff = np.zeros(n + 1, np.uint32)
    doff[1:] = np.cumsum([len(p[2]) for p in proofs])
    values = np.frombuffer(b"".join(p[0] for p in proofs), np.uint8).copy()
    idx = np.array([p[1] for p in proofs], np.uint32)
    digests = np.frombuffer(b"".join(x for p in proofs for x in p[2]), np.uint8).copy()
    roots = np.frombuffer(b"".join(p[3] for p in proofs), np.uint8).copy()
    return voff, values, idx, doff, digests, roots


# ------------------------------------------------------------------ D: k_gf_apply, encode
# k crosses the input groups of 8 (GF_J), p the row blocks of 8 (GF_R), len the block sizes
# (64 words per step up to 256) and the strided loop past 256 words.
ENC_K = [1, 2, 7, 8, 9, 16, 17]
ENC_P = [1, 2, 7, 8, 9, 17]
ENC_LEN = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 260, 261, 1023, 1025]
ENC_TRIPLES = [(1, 1, 1), (2, 2, 2), (7, 7, 3), (8, 8, 4), (9, 9, 5), (16, 17, 7), (17, 1, 8),
               (1, 17, 255), (2, 9, 256), (7, 8, 257), (8, 7, 260), (9, 2, 261), (16, 1, 1023),
               (17, 17, 1025), (8, 9, 1025), (9, 8, 255), (17, 7, 257), (1, 8, 261), (16, 2, 3),
               (2, 1, 1023)]
ENC_N_INST = 3


def encode_case(k, p, ln):
    """(submitted uint8[n_inst, k + p, ln] with junk in the parity rows, expected: the same data
    rows with ReedSolomon::encode's parity)."""
    rng = np.random.default_rng(5000 + 10000 * k + 100 * p + ln)
    sub = rng.integers(0, 256, (ENC_N_INST, k + p, ln), dtype=np.uint8)
    exp = sub.copy()
    for i in range(ENC_N_INST):
        enc = B.rs_encode([bytes(r) for r in sub[i]], k, p)
        exp[i] = np.frombuffer(b"".join(enc), np.uint8).reshape(k + p, ln)
    return sub, exp


def guarded(payload, shift):
    """payload (uint8, flat) at SLACK + shift inside a buffer of GUARD bytes with at least SLACK
    of them on both sides; the buffer's size is a multiple of 8."""
    n = SLACK + shift + payload.size + SLACK
    buf = np.full((n + 7) // 8 * 8, GUARD, np.uint8)
    buf[SLACK + shift:SLACK + shift + payload.size] = payload
    return buf


# ------------------------------------------------------------------ E: reconstruct patterns
RECON_ALL = {"E1": (3, 4, 5), "E2": (4, 6, 3)}  # (k, p, len): one instance per presence pattern
MULTIPLICITIES = (1, 3, 17)


class ReconCase:
    """submitted / expected uint8[n_inst, k + p, len], present uint8[n_inst, k + p], status
    int32[n_inst], patterns: the presence string of each instance ('1' = present)."""

    def __init__(self, k, p, ln, patterns, seed):
        rng = np.random.default_rng(seed)
        n = k + p
        self.k, self.p, self.len, self.patterns = k, p, ln, list(patterns)
        ni = len(self.patterns)
        self.encoded = np.zeros((ni, n, ln), np.uint8)
        self.encoded[:, :k] = rng.integers(0, 256, (ni, k, ln), dtype=np.uint8)
        for i in range(ni):
            enc = B.rs_encode([bytes(r) for r in self.encoded[i]], k, p)
            self.encoded[i] = np.frombuffer(b"".join(enc), np.uint8).reshape(n, ln)
        self.present = np.array([[c == "1" for c in pat] for pat in self.patterns], np.uint8)
        self.submitted = self.encoded.copy()
        self.submitted[self.present == 0] = 0  # missing rows are zeroed
        enough = self.present.sum(axis=1) >= k
        self.status = np.where(enough, ACCEPT, NOT_ENOUGH).astype(np.int32)
        # too few shards: the bytes stay as submitted; otherwise the whole encoding comes back
        self.expected = np.where(enough[:, None, None], self.encoded, self.submitted)

    def oracle_rows(self, i):
        """ReedSolomon::reconstruct_shards of instance i by the oracle (None: too few shards)."""
        rows = [bytes(r) if f else None for r, f in zip(self.submitted[i], self.present[i])]
        try:
            return B.rs_reconstruct(rows, self.k, self.p)
        except B.ReconstructError:
            return None

    def groups(self):
        """The library's launch groups: instances that miss a shard and have enough, by pattern,
        in the pattern string's sort order (std::map) -> [(pattern, size)]."""
        cnt = {}
        for pat, st in zip(self.patterns, self.status):
            if st == ACCEPT and "0" in pat:
                cnt[pat] = cnt.get(pat, 0) + 1
        return sorted(cnt.items())


_RECON_CACHE = {}


def recon_case(name):
    """E1 / E2: every presence pattern once.  E3: 60 of E2's patterns with multiplicities cycling
    1, 3, 17 in sort order (so groups of 3 and 17 come after smaller ones), instances shuffled."""
    if name not in _RECON_CACHE:
        if name in RECON_ALL:
            k, p, ln = RECON_ALL[name]
            pats = ["".join(b) for b in itertools.product("01", repeat=k + p)]
            _RECON_CACHE[name] = ReconCase(k, p, ln, pats, 6000 + k)
        else:
            k, p, ln = RECON_ALL["E2"]
            rng = random.Random(6100)
            every = ["".join(b) for b in itertools.product("01", repeat=k + p)]
            chosen = sorted(rng.sample([x for x in every if x.count("1") >= k and "0" in x], 54))
            pats = [x for j, x in enumerate(chosen) for _ in range(MULTIPLICITIES[j % 3])]
            pats += rng.sample([x for x in every if x.count("1") < k], 5) + ["1" * (k + p)]
            rng.shuffle(pats)
            _RECON_CACHE[name] = ReconCase(k, p, ln, pats, 6200)
    return _RECON_CACHE[name]


# ------------------------------------------------------------------ F: ordering of the *_dev forms
def raw_chain(region):
    """F-RAW: the last 192 bytes of `region` (uint8) are one instance of (k, p, len) = (1, 2, 64)
    with the data row in place.  Returns (shards after encode, root of their tree): what calls
    2 - 4 of the chain must see."""
    tail = bytes(region[-192:])
    shards = B.rs_encode([tail[0:64], tail[64:128], tail[128:192]], 1, 2)
    return shards, B.merkle_levels(shards)[1]


def sha3(b):
    return hashlib.sha3_256(bytes(b)).digest()
