"""The cases of tests/broadcast_cases.py against hashlib and the oracle: the conditions under which
tests/test_gpu_broadcast_edges.py says something about the kernels.  No GPU and no library."""
import hashlib

import numpy as np
import pytest

import broadcast_cases as BC
from oracle import broadcast as B


def _h(b):
    return hashlib.sha3_256(bytes(b)).digest()


def _tree_by_hand(values):
    """merkle.rs:19-32 written out once more over hashlib alone."""
    out, cur = [], [_h(v) for v in values]
    while len(cur) > 1:
        out += cur
        cur = [_h(cur[i] + cur[i + 1]) if i + 1 < len(cur) else cur[i] for i in range(0, len(cur), 2)]
    return out + cur


# ------------------------------------------------------------------ A / B
def test_leaf_lengths_hit_every_padding_class():
    want = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127} | set(range(128, 138)) | \
           {143, 144, 145, 271, 272, 273, 407, 408, 409}
    assert set(BC.LEAF_LENS) == want and len(BC.LEAF_LENS) == len(want)
    rem = {n % BC.RATE for n in BC.LEAF_LENS}
    assert 0 in rem and set(range(128, 136)) <= rem          # `rem == 0`, `rem >= 128`
    assert {n // BC.RATE for n in BC.LEAF_LENS if n % BC.RATE == 0} == {1, 2, 3}
    assert any(n >= 2 * BC.RATE for n in BC.LEAF_LENS)        # the absorb loop runs more than once
    assert (BC.LEAF_N_LEAVES, BC.LEAF_N_INST) == (5, 3)


@pytest.mark.parametrize("leaf_len", [1, 135, 136, 137, 272, 409])
def test_leaf_case_digests_are_hashlib(leaf_len):
    leaves, dig = BC.leaf_case(leaf_len)
    assert leaves.shape == (3, 5, leaf_len) and dig.shape == (3, 5 + 3 + 2 + 1, 32)
    for inst in range(3):
        assert [bytes(d) for d in dig[inst]] == _tree_by_hand([bytes(v) for v in leaves[inst]])
        # 5 -> 3 -> 2 -> 1: the odd digest is carried up unhashed on two levels
        assert bytes(dig[inst][7]) == bytes(dig[inst][4]) and bytes(dig[inst][9]) == bytes(dig[inst][7])
    assert len({bytes(v) for v in leaves.reshape(-1, leaf_len)}) > 1


def test_tree_shapes_cross_the_pair_loop():
    assert BC.TREE_N_LEAVES == [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 33, 127, 128, 129, 255, 256, 257]
    assert (BC.TREE_LEAF_LEN, BC.TREE_N_INST) == (3, 2)
    for n in BC.TREE_N_LEAVES:
        leaves, dig = BC.shape_case(n)
        count, m = n, n
        while m > 1:
            m = (m + 1) // 2
            count += m
        assert dig.shape == (2, count, 32)
        if n in (1, 6, 129, 257):
            for inst in range(2):
                assert [bytes(d) for d in dig[inst]] == _tree_by_hand([bytes(v) for v in leaves[inst]])


# ------------------------------------------------------------------ C
def test_proof_cases_accepts_and_rejects():
    assert BC.PROOF_N_NODES == [1, 2, 3, 5, 6, 7, 9, 13, 17, 33, 100, 255, 256]
    assert BC.VALUE_LENS == [0, 1, 135, 136, 137, 272, 300]
    rejected = {c: 0 for c in BC.TAMPER_CLASSES}
    starts = set()
    for n in BC.PROOF_N_NODES:
        items = BC.proof_case(n)
        valid = [(pr, ok) for c, pr, ok in items if c == "valid"]
        assert len(valid) == n and [pr[1] for pr, _ in valid] == list(range(n))
        assert sum(ok for _, ok in valid) == n                 # exactly n_nodes ACCEPTs untampered
        classes = {c for c, _, _ in items}
        assert {"root_w0_even", "root_w0_odd", "root_w3_even", "root_w3_odd"} <= classes
        for c, pr, ok in items:
            if c != "valid" and not ok:
                rejected[c] += 1
        voff = BC.pack_proofs([pr for _, pr, _ in items])[0]
        starts |= {(int(o) % 4, len(pr[0])) for o, (_, pr, _) in zip(voff, items)}
    assert all(rejected[c] > 0 for c in BC.TAMPER_CLASSES), rejected
    # the concatenated values start at every byte alignment, at every length that has a full block
    for ln in (135, 136, 137, 272, 300):
        assert {a for a, n in starts if n == ln} == {0, 1, 2, 3}, ln
    assert any(n == 0 for _, n in starts)


def test_half_bit_tampers_differ_in_one_lane_only():
    """Each root_* / sibling_* tamper differs from the valid proof in one bit, at an even position
    of its 64-bit word (lane 0 of the pair) or at an odd one (lane 1), and the oracle rejects it."""
    items = BC.proof_case(13)
    valid = {pr[1]: pr for c, pr, _ in items if c == "valid"}
    seen = set()
    for c, pr, ok in items:
        kind, _, name = c.partition("_")
        if name not in BC.HALF_BITS:
            continue
        ref = valid[pr[1]]
        a = b"".join(ref[2]) + ref[3]
        b = b"".join(pr[2]) + pr[3]
        diff = int.from_bytes(a, "little") ^ int.from_bytes(b, "little")
        assert bin(diff).count("1") == 1 and not ok
        pos = diff.bit_length() - 1
        assert (pos % 64) % 2 == (1 if name.endswith("odd") else 0)
        assert (pos < 256 * len(ref[2])) == (kind == "sibling")
        seen.add(c)
    assert seen == {k + "_" + n for k in ("root", "sibling") for n in BC.HALF_BITS}


def test_last_leaf_with_index_n_nodes():
    """The oracle's verdicts, not an assumption: index = n_nodes with the last leaf's proof walks
    the same siblings as the last leaf for n_nodes = 1 and 6, and is valid there."""
    got = {n: BC.last_leaf_at_n_nodes(n)[1] for n in BC.PROOF_N_NODES}
    assert got == {n: n in (1, 6) for n in BC.PROOF_N_NODES}
    for n in BC.PROOF_N_NODES:
        pr, ok = BC.last_leaf_at_n_nodes(n)
        assert pr[1] == n and B.proof_validate(pr, n) == ok


def test_batch_cases():
    assert BC.BATCH_SIZES == [1, 31, 32, 33, 65]
    for size in BC.BATCH_SIZES:
        n_nodes, items = BC.batch_case(size)
        assert len(items) == size and n_nodes == 13
        verdicts = {ok for _, _, ok in items}
        assert True in verdicts and (size == 1 or False in verdicts)


# ------------------------------------------------------------------ D
def test_encode_triples_cover_the_tiling():
    assert {t[0] for t in BC.ENC_TRIPLES} == set(BC.ENC_K) == {1, 2, 7, 8, 9, 16, 17}
    assert {t[1] for t in BC.ENC_TRIPLES} == set(BC.ENC_P) == {1, 2, 7, 8, 9, 17}
    assert {t[2] for t in BC.ENC_TRIPLES} == set(BC.ENC_LEN) == \
        {1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 260, 261, 1023, 1025}
    assert 15 <= len(BC.ENC_TRIPLES) <= 25 and len(set(BC.ENC_TRIPLES)) == len(BC.ENC_TRIPLES)


@pytest.mark.parametrize("k,p,ln", BC.ENC_TRIPLES)
def test_encode_case_round_trip(k, p, ln):
    """The expected parity decodes back to the data from the LAST k shards (the parity rows first
    in line), and the submitted parity rows hold something else."""
    sub, exp = BC.encode_case(k, p, ln)
    assert np.array_equal(sub[:, :k], exp[:, :k])
    assert all(not np.array_equal(sub[i, k:], exp[i, k:]) for i in range(BC.ENC_N_INST))
    for i in range(BC.ENC_N_INST):
        rows = [bytes(r) for r in exp[i]]
        kept = [r if j >= p else None for j, r in enumerate(rows)]  # the last k of the k + p shards
        assert B.rs_reconstruct(kept, k, p) == rows


def test_guarded_layout():
    for shift in BC.ALIGNS:
        buf = BC.guarded(np.arange(10, dtype=np.uint8), shift)
        assert buf.size % 8 == 0 and buf.size >= 2 * BC.SLACK + 10 + shift
        assert bytes(buf[BC.SLACK + shift:BC.SLACK + shift + 10]) == bytes(range(10))
        assert (buf[:BC.SLACK + shift] == BC.GUARD).all() and (buf[BC.SLACK + shift + 10:] == BC.GUARD).all()
        assert buf.size - (BC.SLACK + shift + 10) >= BC.SLACK


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("name,accepted,refused", [("E1", 99, 29), ("E2", 848, 176)])
def test_recon_all_patterns(name, accepted, refused):
    c = BC.recon_case(name)
    assert (c.k, c.p, c.len) == BC.RECON_ALL[name]
    assert len(set(c.patterns)) == len(c.patterns) == 2 ** (c.k + c.p)
    assert int((c.status == BC.ACCEPT).sum()) == accepted
    assert int((c.status == BC.NOT_ENOUGH).sum()) == refused
    for i, st in enumerate(c.status):
        rows = c.oracle_rows(i)
        if st == BC.ACCEPT:  # the oracle's reconstruct_shards reproduces the encoding
            assert b"".join(rows) == c.encoded[i].tobytes() == c.expected[i].tobytes()
        else:
            assert rows is None and c.expected[i].tobytes() == c.submitted[i].tobytes()
            assert (c.submitted[i][c.present[i] == 0] == 0).all()
    assert len({c.encoded[i].tobytes() for i in range(len(c.patterns))}) == len(c.patterns)
    assert len(c.groups()) == accepted - 1 and all(size == 1 for _, size in c.groups())


def test_recon_e2_flushes_the_plan_cache():
    """One plan per set of missing data shards given the pattern, one per set of missing parity
    shards: E2 needs far more than the cache's 256, so it is emptied several times in the call."""
    c = BC.recon_case("E2")
    keys = set()
    for pat, _ in c.groups():
        if "0" in pat[:c.k]:
            keys.add("dec/" + pat)
        if "0" in pat[c.k:]:
            keys.add("par/" + pat[c.k:])
    assert len(keys) > 3 * 256


def test_recon_e3_groups_grow_inside_the_call():
    c = BC.recon_case("E3")
    sizes = [size for _, size in c.groups()]
    assert set(sizes) == set(BC.MULTIPLICITIES) == {1, 3, 17}
    # in the order the library visits them, a group of 3 follows a smaller one and a group of 17
    # follows those: the job list outgrows its buffer twice inside the call
    assert sizes.index(1) < sizes.index(3) < sizes.index(17)
    assert sizes[:3] == [1, 3, 17]
    order = [p for p in c.patterns if "0" in p and p.count("1") >= c.k]
    assert order != sorted(order)                               # the instances are shuffled
    assert (c.status == BC.NOT_ENOUGH).sum() == 5 and "1" * 10 in c.patterns
    for i, st in enumerate(c.status):
        if st == BC.ACCEPT:
            assert b"".join(c.oracle_rows(i)) == c.expected[i].tobytes()


# ------------------------------------------------------------------ F
def test_raw_chain_expectation():
    rng = np.random.default_rng(1)
    region = rng.integers(0, 256, 1000, dtype=np.uint8)
    shards, root = BC.raw_chain(region)
    data = bytes(region[-192:-128])
    assert shards == [data, data, data]  # k = 1: every parity shard repeats the data shard
    assert bytes(region[-128:-64]) != data and bytes(region[-64:]) != data
    pair = _h(_h(data) + _h(data))
    assert root == _h(pair + _h(data))
    assert B.proof_validate((data, 2, [pair], root), 3)
    assert not B.proof_validate((bytes(region[-64:]), 2, [pair], root), 3)
    assert not B.proof_validate((data, 2, [bytes(32)], root), 3)
