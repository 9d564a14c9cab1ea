"""The cases of tests/hash_cases.py against the oracle, hashlib and the host C path: the
conditions under which tests/test_gpu_hash_edges.py says something about k_hash_cand and
k_g2_clear_cofactor.  No GPU.  The host path (hbtc_hash_g2_batch / hbtc_hash_g1_g2_batch) is the
kernels' own HASH_HD code compiled for the CPU, so a mistake in the shared code fails here first."""
import hashlib

import pytest

import hash_cases as HC
from hbbft_amd import _native as N
from oracle import bls12_381 as B
from oracle import threshold_crypto as TC


@pytest.fixture(scope="module")
def g2():
    """[(name, msg, traced hash, profile)]"""
    return [(name, m) + HC.trace(m) for name, m in HC.g2_cases()]


@pytest.fixture(scope="module")
def g1g2():
    """[(name, u, v, traced hash, profile)]"""
    return [(name, u, v) + HC.trace(HC.g1g2_seed_msg(u, v)) for name, u, v in HC.g1g2_cases()]


def _row(name, p):
    return "%-8s att %d  rej %-40s g %d neg %d kneg %d swap %d  hi15 %d  gw %-22s blocks %d" % (
        name, p["attempts"], " ".join("%d/%d" % r for r in p["rej"]), p["greatest"], p["negated"],
        p["kernel_negated"], p["kernel_swapped"], sum(w % 16 == 15 for w in p["hi_words"]),
        ",".join(str(w % 16) for w in p["greatest_words"]), p["blocks"])


def _mined_classes(rows, n_mined):
    """{class: [names of the mined cases in it]}; the table is printed on the way."""
    for r in rows:
        print(_row(r[0], r[-1]))
    mined = rows[:n_mined]
    got = {k: [r[0] for r in mined if f(r[-1])] for k, f in HC.CLASSES.items()}
    for k, names in got.items():
        print("%-52s %s" % (k, " ".join(names)))
    return got


def test_class_list_is_the_one_to_pin():
    want = {"attempts = 1", "attempts = 2", "attempts = 3", "attempts >= 6",
            "rejection in an attempt that fails the square test", "u64 high word at word 15",
            "greatest word at word 15", "greatest word at word 0", "blocks >= 8",
            "kernel root from a square delta", "kernel root from a non-square delta"}
    want |= {"%s rejections %s" % (c, r) for c in ("c0", "c1") for r in ("= 0", "= 1", "= 2", ">= 3")}
    want |= {"greatest = %d, %s negated = %d" % (g, y, n) for g in (0, 1) for n in (0, 1)
             for y in ("y", "kernel's y")}
    assert set(HC.CLASSES) == want
    assert HC.G2_LENGTHS == [0, 1, 7, 8, 9, 135, 136, 137, 271, 272, 273, 408, 1000]
    assert HC.G1G2_LENGTHS == [0, 1, 63, 64, 65, 66, 135, 136, 137, 272, 273]
    assert HC.BATCH_SIZES == [1, 2, 31, 32, 33, 63, 64, 65, 129]


def test_every_draw_class_has_a_hash_g2_message(g2):
    got = _mined_classes(g2, len(HC.G2_COUNTERS))
    assert not [k for k, names in got.items() if not names]
    assert sum(HC.is_light(r[-1]) for r in g2[:len(HC.G2_COUNTERS)]) >= HC.N_LIGHT


def test_every_draw_class_has_a_hash_g1_g2_input(g1g2):
    got = _mined_classes(g1g2, len(HC.G1G2_COUNTERS))
    assert not [k for k, names in got.items() if not names]
    assert sum(HC.is_light(r[-1]) for r in g1g2[:len(HC.G1G2_COUNTERS)]) >= HC.N_LIGHT
    assert len({u for _, u, _, _, _ in g1g2}) > HC.U_MULTIPLES  # u varies, in the seed's last block


def test_stored_counters_are_what_the_search_finds():
    assert HC.mine(HC.g2_msg) == HC.G2_COUNTERS
    assert HC.mine(lambda c: HC.g1g2_seed_msg(*HC.g1g2_input(c))) == HC.G1G2_COUNTERS


def test_profile_counts_are_consistent(g2, g1g2):
    for row in g2 + g1g2:
        p = row[-1]
        calls = sum(2 + a + b for a, b in p["rej"])
        assert len(p["rej"]) == len(p["greatest_words"]) == p["attempts"]
        assert len(p["hi_words"]) == 6 * calls and p["words"] == 12 * calls + p["attempts"]
        assert p["blocks"] == -(-p["words"] // 16)
        # a high word at 15 needs an odd stream position: only after a `greatest` draw
        assert all(w % 2 == 0 for w in p["hi_words"][:6 * (2 + sum(p["rej"][0]))])


def test_trace_is_the_oracle_hash_g2(g2):
    for name, m, h, _ in g2:
        assert h == TC.hash_g2(m), name
        assert HC.want_g2(m) == B.g2_compress(h), name


def test_trace_is_the_oracle_hash_g1_g2(g1g2):
    for name, u, v, h, _ in g1g2:
        assert h == TC.hash_g1_g2(B.g1_decompress(u), v), name
        assert HC.want_g1g2(u, v) == B.g2_compress(h), name
    # |v| = 65 .. take the inner digest, |v| <= 64 do not
    lens = {len(v): len(HC.g1g2_seed_msg(u, v)) for _, u, v, _, _ in g1g2}
    assert lens[64] == 112 and lens[65] == lens[66] == lens[273] == 80 and lens[0] == 48


def test_sha3_at_every_length_used(g2, g1g2):
    msgs = [m for _, m, _, _ in g2] + [v for _, _, v, _, _ in g1g2] + \
           [HC.g1g2_seed_msg(u, v) for _, u, v, _, _ in g1g2]
    assert {0, 1, 135, 136, 137, 271, 272, 273, 408, 1000} <= {len(m) for m in msgs}
    for m in msgs:
        want = hashlib.sha3_256(m).digest()
        assert TC.sha3_256(m) == want and N.sha3_256(m) == want, len(m)


def test_host_path_equals_the_oracle_on_every_case(g2, g1g2):
    got = N.hash_g2_batch([m for _, m, _, _ in g2])
    assert [n for (n, m, _, _), h in zip(g2, got) if h != HC.want_g2(m)] == []
    got = N.hash_g1_g2_batch([u for _, u, _, _, _ in g1g2], [v for _, _, v, _, _ in g1g2])
    assert [n for (n, u, v, _, _), h in zip(g1g2, got) if h != HC.want_g1g2(u, v)] == []


def test_layouts_place_the_heavy_draw_and_the_empty_messages(g2, g1g2):
    for rows, n_case_fields in ((g2, 1), (g1g2, 2)):
        profs = [r[-1] for r in rows]
        empty = [i for i, r in enumerate(rows) if r[n_case_fields] == b""]
        assert len(empty) == 1
        lay = HC.layouts(profs, empty[0])
        assert [len(lay["n = %d" % n]) for n in HC.BATCH_SIZES] == HC.BATCH_SIZES
        heavy = lay["n = 1"][0]
        assert profs[heavy]["attempts"] >= 6 and profs[heavy]["attempts"] == max(p["attempts"] for p in profs)
        for n, mid in ((33, 16), (65, 32), (129, 96)):
            idx = lay["n = %d" % n]
            assert [i for i, c in enumerate(idx) if c == heavy] == [0, mid, n - 1]
            assert all(HC.is_light(profs[c]) for c in idx if c != heavy)
            assert len({c for c in idx if c != heavy}) >= HC.N_LIGHT
        # every case is in a batch, at more than one lane
        for c in range(len(rows)):
            lanes = {i % 64 for n in (31, 32, 63, 64) for i, x in enumerate(lay["n = %d" % n]) if x == c}
            assert len(lanes) >= 2, rows[c][0]
        e = lay["empty first, last and adjacent"]
        assert e[0] == e[1] == e[-1] == empty[0] and e[4:7] == empty * 3 and set(e) != set(empty)
        assert lay["only empty"] == empty * 33
