"""Cases for BLAKE3 as the context's digest (MS_FLAG_DIGEST_BLAKE3), shared by the emulation suite (tests/test_blake3_emu.py) and the GPU suite
(tests/test_blake3_gpu.py): the matrix of tests/digest_cases.py (BLAKE2s) plus the messages that cross BLAKE3's 1024-byte chunk.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set.
Expected digests come from tests/pyref_blake3.py, which is pinned by tests/golden/blake3_kats.json."""
import hashlib

import numpy as np
import pytest

import digest_cases as dc
import parity_cases as pc
import pyref
import pyref_blake3 as pb
import pyref_digest as pd
from common import MODULUS, EXT, fibonacci_trace_fast

ZAE, LATENCY, B2, B3 = 1, 4, 8, 0x10   # MS_FLAG_ZERO_DISPLAY_EMPTY, MS_FLAG_LATENCY, MS_FLAG_DIGEST_BLAKE2S, MS_FLAG_DIGEST_BLAKE3
ERR_ARG = -5
ROOT_0_15_SHA256 = dc.ROOT_0_15_SHA256
MERKLE_SHAPES = dc.MERKLE_SHAPES + [(4096, 1, 1, 64),      # inner nodes of 2048 bytes: two chunks and a parent
                                    (512, 1, 1, 512),      # one inner node of 16 KiB: 16 chunks, the longest message supported
                                    (128 * 8, 1, 128, 2),  # the wide AIR's leaf group: up to 2560 bytes (Goldilocks), three chunks
                                    (800 * 2, 1, 800, 2)]  # up to 16 000 bytes: a chaining-value stack of depth 4
EDGE_LENGTHS = dc.EDGE_LENGTHS
CHUNK_EDGES = [1023, 1024, 1025]
TREE_EDGES = [0, 1, 64, 1023, 1024, 1025, 1088, 1089, 2047, 2048, 2049, 3071, 3072, 3073, 4096, 4097]   # through a leaf kernel with a chunk tree: 16 groups


def case_flag_selects_blake3(make):
    import mini_stark_amd as ms
    ctx = make(0, ZAE | B3)
    assert hasattr(ctx.L, "ms_digest") and ctx.L.ms_digest(ctx.h) == 2 and ctx.digest == 2
    assert ms.FLAG_DIGEST_BLAKE3 == B3 and ms.DIGEST_BLAKE3 == 2
    leafs = np.arange(16, dtype=np.uint64)
    rc, _, root = ctx.merkle_commit(leafs, 1, 2, 2)
    with pb.as_blake3():   # pyref's own tree over the scalar BLAKE3
        want = pyref.merkle_nodes([(i,) for i in range(16)], 2, 2, True)[-1]
    assert rc == 0 and root == want and root == pb.tree_nodes(leafs, 1, 2, 2, True)[-1].tobytes()
    for flags, digest, start in ((ZAE, 0, ROOT_0_15_SHA256), (ZAE | B2, 1, dc.ROOT_0_15_BLAKE2S)):
        other = make(0, flags)
        assert other.L.ms_digest(other.h) == digest and other.digest == digest
        rc, _, r = other.merkle_commit(leafs, 1, 2, 2)
        assert rc == 0 and r.hex().startswith(start) and r != root
    with pytest.raises(ms.MsError) as e:   # a context has one D
        make(0, ZAE | B2 | B3)
    assert e.value.code == ERR_ARG


def case_every_node(ctx, field, leaf_num, ext, lpn, ic, zae):
    e = ext or EXT[field]
    leafs = dc._special_leafs(field, leaf_num * e, seed=leaf_num + lpn)
    rc, nodes, root = ctx.merkle_commit(leafs, e, lpn, ic)
    n = leaf_num // lpn
    m = n
    while m > 1 and m % ic == 0:
        m //= ic
    if leaf_num % lpn or n == 0 or m != 1:   # merkle.rs:93-104 panics
        assert rc == pc.ERR_SHAPE
        return
    assert rc == 0, ctx.last_error()
    want = pb.tree_nodes(leafs, e, lpn, ic, zae)
    assert nodes.shape == want.shape
    bad = np.nonzero((nodes != want).any(axis=1))[0]
    assert bad.size == 0, f"first wrong node {bad[0]} of {len(want)}"
    assert root == want[-1].tobytes()


def case_too_long_is_refused(ctx, field):
    """Above 16 KiB per message the call fails with MS_ERR_ARG and says why; the context stays usable."""
    maxd = len(str(MODULUS[field] - 1))
    lpn = 16384 // maxd + 1
    rc, _, _ = ctx.merkle_commit(np.ones(2 * lpn, dtype=np.uint64), 1, lpn, 2)
    assert rc == ERR_ARG and "BLAKE3" in ctx.last_error() and "16384" in ctx.last_error()
    rc, _, _ = ctx.merkle_commit(np.ones(1024, dtype=np.uint64), 1, 1, 1024)
    assert rc == ERR_ARG and "BLAKE3" in ctx.last_error()
    leafs = np.arange(16, dtype=np.uint64)
    rc, _, root = ctx.merkle_commit(leafs, 1, 2, 2)
    assert rc == 0 and root == pb.tree_nodes(leafs, 1, 2, 2, True)[-1].tobytes()


def case_every_height(ctx, field, max_log, zae):
    for h in range(1, max_log + 1):
        leafs = dc._special_leafs(field, 2 << h, seed=h)
        rc, nodes, root = ctx.merkle_commit(leafs, 1, 2, 2)
        assert rc == 0, ctx.last_error()
        want = pb.tree_nodes(leafs, 1, 2, 2, zae)
        assert (nodes == want).all() and root == want[-1].tobytes(), f"2^{h} leaf groups"


def case_merkle_prove(ctx, field, leaf_num=64):
    """ms_merkle_prove on a BLAKE3 context: the path of a leaf found by value holds the siblings of the expected tree (extension-field leaves, lpn 2)"""
    e = EXT[field]
    leafs = pc.rand_field(field, (leaf_num, e), seed=leaf_num + e)
    nodes = pb.tree_nodes(leafs, e, 2, 2, True)
    for idx in (0, 3, leaf_num - 1):
        rc, path = ctx.merkle_prove(leafs.reshape(-1), leafs[idx], e, 2)
        assert rc == 0, ctx.last_error()
        head = 8 + 2 * e * 8 + 8
        got_idx, nlev = int.from_bytes(path[:8], "little"), int.from_bytes(path[head - 8:head], "little")
        assert got_idx == idx and len(path) == head + 64 * nlev
        assert [path[head + 64 * l:head + 64 * l + 64] for l in range(nlev)] == pb.expected_path(nodes, leaf_num // 2, idx)


def groups_of_lengths(field, lpn, lengths):
    """Leaf groups (lpn base elements each, zero printed empty) whose messages have exactly the given lengths (digest_cases.edge_groups' filling)"""
    p = MODULUS[field]
    maxd = len(str(p - 1))
    leafs = np.zeros(len(lengths) * lpn, dtype=np.uint64)
    for g, total in enumerate(lengths):
        assert total <= lpn * maxd
        digs = [0] * lpn
        left, k = total, g
        while left > 0:
            add = min(maxd - digs[k % lpn], left)
            digs[k % lpn] += add
            left -= add
            k += 1
        for j, d in enumerate(digs):
            leafs[g * lpn + j] = 0 if d == 0 else 10 ** (d - 1) + (g * 31 + j) % 9
    assert int(leafs.max()) < p
    return leafs


def _check_groups(ctx, leafs, lpn, lengths, what):
    msgs = pb.leaf_messages(leafs, 1, lpn, True)
    assert [len(m) for m in msgs] == list(lengths)
    rc, nodes, root = ctx.merkle_commit(leafs, 1, lpn, 2)
    assert rc == 0, ctx.last_error()
    want = pb.tree_nodes(leafs, 1, lpn, 2, True)
    bad = np.nonzero((nodes != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: first wrong node {bad[0]}" + (f" (message of {lengths[bad[0]]} bytes)" if bad[0] < len(lengths) else "")
    assert root == want[-1].tobytes()


def case_length_edges(make, field, lpns, lazy):
    """lazy: MS_LEAF_LAZY_MIN at ms_create forces the two-block (True) or the plain (False) leaf kernel.  `lpns`: groups of at most one chunk (the single-chunk
    kernels); then the smallest lpn whose longest message exceeds 1024 bytes - every length 0 ... 1024 + through the multi-chunk instance - and a set of lengths
    around the chunk and subtree boundaries up to 4097 bytes."""
    ctx = make(field, ZAE | B3, env={"MS_LEAF_LAZY_MIN": "1" if lazy else "1000000"})
    maxd = len(str(MODULUS[field] - 1))
    assert all(lpn * maxd <= 1024 for lpn in lpns)
    multi_lpn = 1024 // maxd + 2
    sets = [(lpn,) + dc.edge_groups(field, lpn) for lpn in tuple(lpns) + (multi_lpn,)]
    single, multi = set(), set()
    for lpn, leafs, lengths in sets:
        (multi if lpn == multi_lpn else single).update(lengths)
    for t in EDGE_LENGTHS:
        assert t in single and t in multi, f"no message of {t} bytes in the input"
    for t in CHUNK_EDGES:
        assert t in multi, f"no message of {t} bytes in the input"
    for lpn, leafs, lengths in sets:
        _check_groups(ctx, leafs, lpn, lengths, f"lpn {lpn}")
    lpn = 4097 // maxd + 1
    _check_groups(ctx, groups_of_lengths(field, lpn, TREE_EDGES), lpn, TREE_EDGES, f"lpn {lpn}")


def check_proof_outputs(field, trace, nq, out, trees=None):
    """digest_cases.check_proof_outputs with the trees of pyref_blake3: every root of `out` is the root of the expected tree over the values read back, every Merkle
    path of the MSFP blob holds that tree's siblings."""
    o, e = dict(out), EXT[field]
    w = trace.shape[1]
    rounds = sum(1 for k in o if k.startswith("round_info"))
    if trees is None:
        trees = {"trace": pb.tree_nodes(trace, 1, 2 * w, 2, True), "lde": pb.tree_nodes(o["lde"], 1, 2 * w, 2, True)}
        for i in range(rounds):
            trees[i] = pb.tree_nodes(o[f"round_cw{i}"], e, 2, 2, True)
    assert o["trace_root"] == trees["trace"][-1].tobytes()
    assert o["lde_root"] == trees["lde"][-1].tobytes()
    for i in range(rounds):
        assert o[f"fri_root{i}"] == trees[i][-1].tobytes(), f"root of FRI round {i}"
    _, paths = pb.fri_paths(o["fri_proof"], e, rounds - 1, nq)
    for win, idx, levels in paths:
        D = o[f"round_info{win}"][1]
        assert levels == pb.expected_path(trees[win], D // 2, idx), f"Merkle path of window {win}, leaf {idx}"
    return trees


def case_whole_proof(make, field, log_n, blowup, variants=(("default", ZAE | B3, None),), seed=77, against_pyprover=False):
    """parity_cases.drive on a SHA-256 context and on BLAKE3 contexts (`variants`: (name, flags, env)) with the same (trace, seed): whatever is not a digest equals the
    SHA-256 proof's, every digest is pyref_blake3's."""
    trace = fibonacci_trace_fast(field, 1 << log_n)
    nq_fri = 2
    nq = nq_fri + 2   # drive adds two fixed betas
    e = EXT[field]
    sha = pc.drive(dc.NumpySession(make(field, ZAE)), field, trace, blowup, nq_fri, seed)
    trees, first = None, None
    for name, flags, env in variants:
        ctx = make(field, flags, env=env)
        assert ctx.digest == 2
        b3 = pc.drive(dc.NumpySession(ctx), field, trace, blowup, nq_fri, seed)
        ctx.close()
        assert [k for k, _ in b3] == [k for k, _ in sha]
        for (k, vs), (_, vb) in zip(sha, b3):
            if not dc._is_digest_output(k):   # the challenges are inputs: whatever is not a digest does not depend on D
                assert dc._same(vs, vb), f"{name}: stage output {k} differs between the digests"
        rounds = sum(1 for k, _ in b3 if k.startswith("round_info"))
        ps, _ = pb.fri_paths(dict(sha)["fri_proof"], e, rounds - 1, nq)
        p3, _ = pb.fri_paths(dict(b3)["fri_proof"], e, rounds - 1, nq)
        assert ps == p3, f"{name}: points / quotients / opened leaves of the FRI proof differ between the digests"
        trees = check_proof_outputs(field, trace, nq, b3, trees)
        if first is None:
            first = b3
        else:
            for (k, v0), (_, v1) in zip(first, b3):
                assert dc._same(v0, v1), f"{name}: stage output {k} differs from the first variant's"
    if against_pyprover:
        with pb.as_blake3():
            dc._against_pyprover(field, trace, blowup, nq_fri, seed, first)


def case_roundtrip_and_cross_rejection(make, field, steps, blowup):
    """prove -> verify through the C++ mirror and the Python mirror with each of the three digests; a proof made under one digest is rejected under each of the other
    two; a flipped byte in a Merkle path is rejected."""
    from mini_stark_amd.host import HostStark
    from mini_stark_amd.stark import Stark, StarkConfig, fibonacci_air
    ctxs = {0: make(field, ZAE), 1: make(field, ZAE | B2), 2: make(field, ZAE | B3)}
    hs, wire, pyproof, cons = {}, {}, {}, None
    for d, ctx in ctxs.items():
        assert ctx.digest == d
        tt = fibonacci_air(ctx, steps)
        hs[d] = HostStark(ctx, 20, blowup, steps, tt.constrain_number())
        if cons is None:
            cons = hs[d].derive_constrains(tt)   # (polynomials: the same for every digest)
        proof = hs[d].prove(tt)
        wire[d] = hs[d].proof_bytes()
        py = Stark(StarkConfig(ctx, 20, blowup, steps, tt.constrain_number())).prove(tt)   # the Python mirror draws the same challenges from the same chain
        pyproof[d] = py
        assert py.to_bytes() == wire[d] and proof.arthur == py.arthur
        assert hs[d].verify_bytes(cons, wire[d]), hs[d].last_verify_error
        assert hs[d].verify(cons, py), hs[d].last_verify_error
    assert len({wire[0], wire[1], wire[2]}) == 3
    for d in (0, 1, 2):
        for o in (0, 1, 2):
            if o != d:
                assert not hs[d].verify_bytes(cons, wire[o]) and hs[d].last_verify_error, f"verifier over digest {d} accepted a proof made under digest {o}"
                assert not hs[d].verify(cons, pyproof[o]), f"verifier over digest {d} accepted the Python mirror's proof made under digest {o}"
    bad = bytearray(wire[2]); bad[-1] ^= 1   # a byte of the LAST Merkle path's top level
    assert not hs[2].verify_bytes(cons, bytes(bad)) and "Merkle" in hs[2].last_verify_error


def case_shard_fails_closed(make, field=0):
    import ctypes as C
    from mini_stark_amd._native import EXCHANGE_FN
    ctx = make(field, ZAE | B3)
    calls = []
    cb = EXCHANGE_FN(lambda user, op, nbytes: calls.append((op, nbytes)) or 0)
    buf = (C.c_uint8 * 8192)()
    ctx.L.ms_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, EXCHANGE_FN, C.c_void_p]
    rc = ctx.L.ms_set_shard(ctx.h, 0, 2, C.addressof(buf), C.addressof(buf) + 4096, 4096, cb, None)
    assert rc == ERR_ARG and "SHA-256 only" in ctx.last_error()
    ctx.L.ms_set_shard_rccl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    assert ctx.L.ms_set_shard_rccl(ctx.h, 0, 2, bytes(128), 1 << 20) == ERR_ARG and "SHA-256 only" in ctx.last_error()
    # the context is unsharded and whole: a commitment goes through without a single exchange
    leafs = np.arange(16, dtype=np.uint64)
    rc, _, root = ctx.merkle_commit(leafs, 1, 2, 2)
    assert rc == 0 and root == pb.tree_nodes(leafs, 1, 2, 2, True)[-1].tobytes() and calls == []


def case_msh_hash():
    """msh_hash of the host mirror: ids 0 / 1 against hashlib, id 2 against the KAT file, on the KAT inputs; an unknown id is refused; stark.py's wrapper"""
    from mini_stark_amd.host import hash_bytes
    from mini_stark_amd.stark import DIGEST_HASH
    import mini_stark_amd as ms
    kats = pb.load_kats()
    assert len(kats) > 200 and kats[0] == (b"", bytes.fromhex("af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"))
    for data, want in kats:
        assert hash_bytes(2, data) == want, f"BLAKE3 of {len(data)} bytes"
        assert hash_bytes(0, data) == hashlib.sha256(data).digest()
        assert hash_bytes(1, data) == hashlib.blake2s(data, digest_size=32).digest()
        for d in (0, 1, 2):
            assert DIGEST_HASH[d](data).digest() == hash_bytes(d, data)
    h = DIGEST_HASH[2](b"ab"); h.update(b"c")
    assert h.hexdigest() == "6437b3ac38465133ffb63b75273a8db548c558465d79db03fd359c6cd5bd9d85"
    with pytest.raises(ms.MsError):
        hash_bytes(3, b"")


def case_pyref_pinned():
    """tests/pyref_blake3.py itself: scalar and batched against the KAT file, batched against scalar on random messages"""
    kats = pb.load_kats()
    for data, want in kats:
        assert pb.blake3(data) == want, f"scalar BLAKE3 of {len(data)} bytes"
    got = pb.hash_many([d for d, _ in kats])
    for i, (data, want) in enumerate(kats):
        assert got[i].tobytes() == want, f"batched BLAKE3 of {len(data)} bytes"
    rng = np.random.default_rng(3)
    msgs = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 1100, 300)]
    got = pb.hash_many(msgs)
    assert all(got[i].tobytes() == pb.blake3(m) for i, m in enumerate(msgs))
    rows = rng.integers(0, 256, (40, 512), dtype=np.uint8)
    assert all(r.tobytes() == pb.blake3(rows[i].tobytes()) for i, r in enumerate(pb.hash_rows(rows)))
