"""The Reliable Broadcast kernels (hbtc_bcast.hip) at their byte-level edges, and the ordering of
the device-pointer forms, through hbtc_rs_encode_dev / hbtc_rs_reconstruct_dev /
hbtc_merkle_trees_dev / hbtc_merkle_validate_dev on buffers of their own.

Reference: tests/broadcast_cases.py (hashlib.sha3_256 and oracle/broadcast.py; held against
hashlib and the round trips by tests/test_broadcast_cases.py).  Bar: identical bytes and statuses,
every buffer compared whole, with 64 bytes of 0xA5 on both sides of every payload.

Kernel branches reached, by family:
  A  sha3_mem2 / load_block in k_merkle_tree: `rem == 0` (136, 272, 408: the empty last block, the
     absorb loop's `>=`), `rem >= 128` (the 0x06 in the last rate word, at 135 on the byte of the
     0x80), the partial-word masks, and `s != 0` (d_leaves at every byte alignment)
  B  k_merkle_tree's level loop: carried digests, the second and third trip of the 128-pair loop
  C  k_merkle_validate: the multi-block absorb at every alignment, empty values, the level walk
     under index tampers, `it >= end` / `it != end`, and a mismatch that only ONE lane of the pair
     sees (root / sibling bits at even and at odd positions)
  D  k_gf_apply: partial and several input groups (k), partial and several row blocks (p), block
     sizes 64 .. 256 and the strided loop (len), `sh != 0` on loads and the byte-wise stores
  E  hbtc_rs_reconstruct_dev: every presence pattern, the plan cache emptied inside a call (E2),
     the job list outgrowing its buffer inside a call (E3), refused instances left alone
  F  begin_verify's ranges: a validate that reads what an earlier *_dev call on another lane still
     writes (RAW), and a *_dev call that writes what a pending validate still reads (WAR)
"""
import ctypes
import time

import numpy as np
import pytest

import broadcast_cases as BC
from hbbft_amd import _native as N

pytestmark = pytest.mark.gpu

SLACK = BC.SLACK
# F: the slow call hashes ONE string of F_BYTES bytes on one lane pair.  Measured on an MI355X
# (the "merkle" / "merkle_validate" timing families of that single call, two runs each):
#   1 MiB  merkle 56.5 - 57.8 ms   merkle_validate 67.1 - 68.4 ms
#   2 MiB        123 - 141 ms                      117 - 127 ms
#   8 MiB        468 - 543 ms                      489 - 512 ms
# A launch plus an event wait is tens of microseconds, so 1 MiB already leaves three orders of
# magnitude; before merkle_validate_dev declared d_values / d_digests both tests below reported
# REJECT at this size.
F_BYTES = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


class Dev:
    """Device allocations of one test: each a guarded buffer uploaded whole, freed at the end."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, payload, shift=0, fill=None):
        """payload (any dtype) at SLACK + shift of a new allocation -> (pointer to it, handle)."""
        flat = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
        host = BC.guarded(flat, shift)
        if fill is not None:
            host[SLACK + shift:SLACK + shift + flat.size] = fill
        p = self.ctx.dev_alloc(host.size)
        self.ptrs.append(p)
        self.ctx.dev_upload(p, host)
        return ctypes.c_void_p(p.value + SLACK + shift), (p, host.size)

    def get(self, handle):
        out = np.empty(handle[1], np.uint8)
        self.ctx.dev_download(out, handle[0])
        return out

    def close(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def _at(p, off):
    return ctypes.c_void_p(p.value + off)


def _trees_dev(ctx, dev, leaves, want, shift):
    """hbtc_merkle_trees_dev with d_leaves at byte alignment `shift`: every digest of every level,
    the guards of the digest buffer, and the leaf buffer unchanged."""
    n_inst, n_leaves, leaf_len = leaves.shape
    d_leaves, h_leaves = dev.put(leaves, shift)
    d_dig, h_dig = dev.put(want, 0, fill=BC.GUARD)
    ctx._check(ctx.lib.hbtc_merkle_trees_dev(ctx.h, n_leaves, leaf_len, n_inst, d_leaves, d_dig), "trees_dev")
    got = dev.get(h_dig)
    exp = BC.guarded(want.reshape(-1), 0)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero((got != exp)) // 32
        raise AssertionError("leaf_len %d, n_leaves %d, shift %d: digest buffer differs in 32-byte cells %s"
                             % (leaf_len, n_leaves, shift, sorted(set(bad.tolist()))[:12]))
    assert np.array_equal(dev.get(h_leaves), BC.guarded(leaves.reshape(-1), shift))


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("leaf_len", BC.LEAF_LENS)
def test_leaf_hash_padding_and_alignment(ctx, dev, leaf_len):
    leaves, want = BC.leaf_case(leaf_len)
    for shift in BC.ALIGNS:
        _trees_dev(ctx, dev, leaves, want, shift)
    assert np.array_equal(ctx.merkle_trees(BC.LEAF_N_LEAVES, leaf_len, leaves), want)  # the host form


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("n_leaves", BC.TREE_N_LEAVES)
def test_tree_shapes(ctx, dev, n_leaves):
    leaves, want = BC.shape_case(n_leaves)
    assert ctx.lib.hbtc_merkle_digest_count(n_leaves) == want.shape[1]
    _trees_dev(ctx, dev, leaves, want, n_leaves % 4)


# ------------------------------------------------------------------ C
def _validate_dev(ctx, dev, n_nodes, items, shift):
    proofs = [pr for _, pr, _ in items]
    voff, values, idx, doff, digests, roots = BC.pack_proofs(proofs)
    n = len(proofs)
    d_voff, _ = dev.put(voff)
    d_val, _ = dev.put(values, shift)
    d_idx, _ = dev.put(idx)
    d_doff, _ = dev.put(doff)
    d_dig, _ = dev.put(digests)
    d_roots, _ = dev.put(roots)
    d_st, h_st = dev.put(np.zeros(n, np.int32), 0, fill=BC.GUARD)
    ctx._check(ctx.lib.hbtc_merkle_validate_dev(ctx.h, n, n_nodes, d_voff, d_val, d_idx, d_doff, d_dig,
                                                d_roots, d_st), "validate_dev")
    want = np.array([BC.ACCEPT if ok else BC.REJECT for _, _, ok in items], np.int32)
    got = dev.get(h_st)
    st = got[SLACK:SLACK + 4 * n].view(np.int32)
    wrong = [(j, items[j][0], len(items[j][1][0]), int(voff[j]) % 4, int(st[j]))
             for j in np.flatnonzero(st != want)]
    assert not wrong, "n_nodes %d: (proof, class, value bytes, value alignment, status) %s" % (n_nodes, wrong[:10])
    assert np.array_equal(got, BC.guarded(want.view(np.uint8), 0))
    return proofs, want


@pytest.mark.parametrize("n_nodes", BC.PROOF_N_NODES)
def test_proof_validation(ctx, dev, n_nodes):
    items = BC.proof_case(n_nodes)
    proofs, want = _validate_dev(ctx, dev, n_nodes, items, n_nodes % 4)
    assert int((want[:n_nodes] == BC.ACCEPT).sum()) == n_nodes
    host = ctx.merkle_validate(n_nodes, [p[0] for p in proofs], [p[1] for p in proofs],
                               [p[2] for p in proofs], [p[3] for p in proofs])
    assert np.array_equal(host, want)                                                  # the host form


@pytest.mark.parametrize("size", BC.BATCH_SIZES)
def test_proof_batch_sizes(ctx, dev, size):
    n_nodes, items = BC.batch_case(size)
    _validate_dev(ctx, dev, n_nodes, items, size % 4)


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("k,p,ln", BC.ENC_TRIPLES)
def test_encode_tiling(ctx, dev, k, p, ln):
    sub, exp = BC.encode_case(k, p, ln)
    for shift in BC.ALIGNS:
        d_sh, h_sh = dev.put(sub, shift)
        ctx._check(ctx.lib.hbtc_rs_encode_dev(ctx.h, k, p, ln, BC.ENC_N_INST, d_sh), "rs_encode_dev")
        got = dev.get(h_sh)
        want = BC.guarded(exp.reshape(-1), shift)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "(k, p, len) = %s, shift %d: %d bytes differ, first at buffer offset %d" % (
            (k, p, ln), shift, bad.size, bad[0])


# ------------------------------------------------------------------ E
def _reconstruct_dev(ctx, dev, case, shift):
    d_sh, h_sh = dev.put(case.submitted, shift)
    present = np.ascontiguousarray(case.present).reshape(-1)
    status = np.full(len(case.patterns), -1, np.int32)
    t0 = time.perf_counter()
    ctx._check(ctx.lib.hbtc_rs_reconstruct_dev(ctx.h, case.k, case.p, case.len, len(case.patterns), d_sh,
                                               N._ptr(present), N._ptr(status)), "rs_reconstruct_dev")
    got = dev.get(h_sh)
    dt = time.perf_counter() - t0
    assert np.array_equal(status, case.status)
    want = BC.guarded(case.expected.reshape(-1), shift)
    if not np.array_equal(got, want):
        per = (case.k + case.p) * case.len
        body = got[SLACK + shift:SLACK + shift + per * len(case.patterns)].reshape(-1, per)
        bad = [case.patterns[i] for i in np.flatnonzero((body != case.expected.reshape(-1, per)).any(axis=1))]
        raise AssertionError("%d instances differ (patterns %s), guards intact: %s" % (
            len(bad), bad[:8], bool((got[:SLACK + shift] == BC.GUARD).all() and
                                    (got[SLACK + shift + body.size:] == BC.GUARD).all())))
    return dt


def test_reconstruct_every_pattern_k3_p4(ctx, dev):
    """E1: 128 instances, one per presence pattern; 29 have fewer than 3 shards and stay as
    submitted, 99 come back whole."""
    _reconstruct_dev(ctx, dev, BC.recon_case("E1"), 1)


def test_reconstruct_every_pattern_k4_p6_flushes_plans(ctx, dev):
    """E2: 1024 instances, one per pattern, 847 launch groups and over 768 plans in one call: the
    256-plan cache is emptied several times inside it.  The longest test here: 0.10 s on an
    MI355X."""
    dt = _reconstruct_dev(ctx, dev, BC.recon_case("E2"), 3)
    print("E2: hbtc_rs_reconstruct_dev + download %.3f s" % dt)


def test_reconstruct_groups_grow_inside_the_call(ctx, dev):
    """E3: shuffled instances, groups of 1, 3 and 17 in the order the call visits them: the job
    list is restaged per group and outgrows its device buffer twice inside the call."""
    _reconstruct_dev(ctx, dev, BC.recon_case("E3"), 2)
    _reconstruct_dev(ctx, dev, BC.recon_case("E3"), 0)  # and with every buffer and plan in place


# ------------------------------------------------------------------ F
def test_order_raw(ctx, dev):
    """F-RAW.  No sync between the four calls; every upload is before the first.
      1  hbtc_merkle_trees_dev over ONE leaf of F_BYTES = 1 MiB (one lane pair: 57 ms measured)
      2  hbtc_rs_encode_dev (1, 2, 64) on the leaf's last 192 bytes: waits for 1 (declared)
      3  hbtc_merkle_trees_dev of those 3 shards into d_tree (zeros before): waits for 2
      4  hbtc_merkle_validate_dev of shard 2 (through a device value_off of [128, 192]) with the
         level-1 digest at d_tree + 96 and the root in a buffer of its own
    Call 4 is ordered after 2 and 3 only through d_values and d_digests, whose sizes are in device
    memory: it must ACCEPT.  Call 1's digest is that of the leaf as uploaded (the declared WAR).
    """
    S = F_BYTES
    rng = np.random.default_rng(7001)
    leaf = rng.integers(0, 256, S, dtype=np.uint8)
    shards, root = BC.raw_chain(leaf)
    tree = BC.tree_digests(shards)
    assert len(tree) == 6
    lib, h = ctx.lib, ctx.h
    d_leaf, h_leaf = dev.put(leaf)
    d_one, h_one = dev.put(np.zeros(32, np.uint8))
    d_tree, h_tree = dev.put(np.zeros(6 * 32, np.uint8))
    d_voff, _ = dev.put(np.array([128, 192], np.uint64))
    d_idx, _ = dev.put(np.array([2], np.uint32))
    d_doff, _ = dev.put(np.array([0, 1], np.uint32))
    d_root, _ = dev.put(np.frombuffer(root, np.uint8))
    d_st, h_st = dev.put(np.full(1, -1, np.int32))
    d_shards = _at(d_leaf, S - 192)
    ctx._check(lib.hbtc_merkle_trees_dev(h, 1, S, 1, d_leaf, d_one), "1 trees_dev")
    ctx._check(lib.hbtc_rs_encode_dev(h, 1, 2, 64, 1, d_shards), "2 rs_encode_dev")
    ctx._check(lib.hbtc_merkle_trees_dev(h, 3, 64, 1, d_shards, d_tree), "3 trees_dev")
    ctx._check(lib.hbtc_merkle_validate_dev(h, 1, 3, d_voff, d_shards, d_idx, d_doff, _at(d_tree, 96), d_root,
                                            d_st), "4 validate_dev")
    status = int(dev.get(h_st)[SLACK:SLACK + 4].view(np.int32)[0])
    assert bytes(dev.get(h_one)[SLACK:SLACK + 32]) == BC.sha3(leaf)
    assert bytes(dev.get(h_leaf)[SLACK + S - 192:SLACK + S]) == b"".join(shards)
    assert bytes(dev.get(h_tree)[SLACK:SLACK + 192]) == b"".join(tree)
    assert status == BC.ACCEPT


def test_order_war(ctx, dev):
    """F-WAR.  No sync between the two calls.
      1  hbtc_merkle_validate_dev of ONE proof (n_nodes = 1, no digests) whose value is a region
         of F_BYTES = 1 MiB and whose root is its SHA3-256 by hashlib (one lane pair: 67 ms
         measured)
      2  hbtc_rs_encode_dev (1, 1, 64) on the region's last 128 bytes: the parity row, which held
         other bytes when the region was hashed, becomes a copy of the data row
    Call 2 writes what call 1 still reads: it has to wait, and call 1 must ACCEPT."""
    S = F_BYTES
    rng = np.random.default_rng(7002)
    value = rng.integers(0, 256, S, dtype=np.uint8)
    assert bytes(value[S - 64:]) != bytes(value[S - 128:S - 64])
    lib, h = ctx.lib, ctx.h
    d_val, h_val = dev.put(value)
    d_voff, _ = dev.put(np.array([0, S], np.uint64))
    d_idx, _ = dev.put(np.array([0], np.uint32))
    d_doff, _ = dev.put(np.array([0, 0], np.uint32))
    d_dig, _ = dev.put(np.zeros(32, np.uint8))
    d_root, _ = dev.put(np.frombuffer(BC.sha3(value), np.uint8))
    d_st, h_st = dev.put(np.full(1, -1, np.int32))
    ctx._check(lib.hbtc_merkle_validate_dev(h, 1, 1, d_voff, d_val, d_idx, d_doff, d_dig, d_root, d_st),
               "1 validate_dev")
    ctx._check(lib.hbtc_rs_encode_dev(h, 1, 1, 64, 1, _at(d_val, S - 128)), "2 rs_encode_dev")
    status = int(dev.get(h_st)[SLACK:SLACK + 4].view(np.int32)[0])
    after = dev.get(h_val)[SLACK:SLACK + S]
    assert bytes(after[S - 64:]) == bytes(value[S - 128:S - 64])  # the encode ran
    assert np.array_equal(after[:S - 64], value[:S - 64])
    assert status == BC.ACCEPT
