"""Cases for Keccak-256 (MS_FLAG_DIGEST_KECCAK256, ms_digest 4) and SHA3-256 (MS_FLAG_DIGEST_SHA3_256, ms_digest 5) as the context's digest, shared by the emulation
suite (tests/test_keccak_emu.py) and the GPU suite (tests/test_keccak_gpu.py): the matrix of tests/blake3_cases.py plus the messages around the 136-byte rate.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set; `d` is the ms_digest_id.
Expected digests: SHA3-256 from hashlib.sha3_256 directly, Keccak-256 from tests/pyref_keccak.py, which case_pyref_pinned holds to hashlib (suffix 0x06) and to
published Keccak-256 digests (suffix 0x01)."""
import hashlib
import itertools

import numpy as np
import pytest

import digest_cases as dc
import parity_cases as pc
import pyref
import pyref_keccak as pk
from common import EXT, fibonacci_trace_fast

ZAE, LATENCY, B2, B3, KECCAK, SHA3 = 1, 4, 8, 0x10, 0x20, 0x40   # MS_FLAG_ZERO_DISPLAY_EMPTY, MS_FLAG_LATENCY, MS_FLAG_DIGEST_*
ERR_ARG = -5
FLAG = {pk.KECCAK256: KECCAK, pk.SHA3_256: SHA3}
DIGESTS = (pk.KECCAK256, pk.SHA3_256)
MERKLE_SHAPES = dc.MERKLE_SHAPES + [(4096, 1, 1, 64),      # inner nodes of 2048 bytes = 15 rate blocks + 8 bytes: 16 blocks
                                    (68, 1, 1, 17),        # a child count that is no power of two: MS_ERR_SHAPE
                                    (64, 1, 1, 32),        # 64 leaf groups are no power of 32: MS_ERR_SHAPE
                                    (1024, 1, 1, 32),      # inner nodes of 1024 bytes = 7 rate blocks + 72 bytes
                                    (128 * 8, 1, 128, 2)]  # the wide AIR's leaf group: up to 2560 bytes (Goldilocks), about 19 blocks
RATE_EDGES = [0, 1, 134, 135, 136, 137, 271, 272, 273]   # the one-byte pad (135), the padding-only block (0, 136) and its second occurrence (272)
KECCAK256_VECTORS = [(b"", "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"),
                     (b"abc", "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"),
                     (b"The quick brown fox jumps over the lazy dog", "4d741b6f1eb29cb2a9b9911c82f56fa8d73b04959d3d9d222895df6c0b28aa15"),
                     (bytes(range(135)), "cbdfd9dee5faad3818d6b06f95a219fd290b0e1706f6a82e5a595b9ce9faca62"),
                     (bytes(range(136)), "7ce759f1ab7f9ce437719970c26b0a66ff11fe3e38e17df89cf5d29c7d7f807e")]


def tree(d, values, ext, lpn, ic, zae=True):
    """every node of the expected tree: hashlib for SHA3-256, the numpy sponge of pyref_keccak for Keccak-256"""
    if d == pk.SHA3_256:
        return pk.tree_nodes_hashlib(values, ext, lpn, ic, zae)
    return pk.tree_nodes(values, ext, lpn, ic, zae, pk.SUFFIX[d])


def case_pyref_pinned():
    """tests/pyref_keccak.py itself: suffix 0x06 is hashlib.sha3_256 on every length 0 ... 300, on 407 / 408 / 409 and on random messages, scalar and batched;
    suffix 0x01 gives the Keccak-256 digests written here; the batched Keccak-256 equals the scalar one"""
    rng = np.random.default_rng(5)
    msgs = [bytes((7 * i + n) % 256 for i in range(n)) for n in list(range(301)) + [407, 408, 409]]
    msgs += [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 1500, 60)]
    want = [hashlib.sha3_256(m).digest() for m in msgs]
    for m, w in zip(msgs, want):
        assert pk.keccak(m, 0x06) == w, f"scalar SHA3-256 of {len(m)} bytes"
    got = pk.hash_many(msgs, 0x06)
    for i, m in enumerate(msgs):
        assert got[i].tobytes() == want[i], f"batched SHA3-256 of {len(m)} bytes"
    for m, hexd in KECCAK256_VECTORS:
        assert pk.keccak(m, 0x01).hex() == hexd, f"scalar Keccak-256 of {len(m)} bytes"
    got = pk.hash_many([m for m, _ in KECCAK256_VECTORS], 0x01)
    assert [g.tobytes().hex() for g in got] == [h for _, h in KECCAK256_VECTORS]
    got = pk.hash_many(msgs, 0x01)
    assert all(got[i].tobytes() == pk.keccak(m, 0x01) for i, m in enumerate(msgs))
    rows = rng.integers(0, 256, (40, 544), dtype=np.uint8)   # 4 * 136: the padding-only block of hash_rows
    assert all(r.tobytes() == hashlib.sha3_256(rows[i].tobytes()).digest() for i, r in enumerate(pk.hash_rows(rows, 0x06)))
    assert all(r.tobytes() == pk.keccak(rows[i].tobytes(), 0x01) for i, r in enumerate(pk.hash_rows(rows, 0x01)))
    vals = np.arange(64, dtype=np.uint64)
    assert (pk.tree_nodes(vals, 1, 2, 2, True, 0x06) == pk.tree_nodes_hashlib(vals, 1, 2, 2, True)).all()
    assert pk.Keccak256(b"abc").hexdigest() == KECCAK256_VECTORS[1][1] and pk.Sha3_256(b"abc").digest() == hashlib.sha3_256(b"abc").digest()


def case_flag_selects(make):
    import mini_stark_amd as ms
    assert (ms.FLAG_DIGEST_KECCAK256, ms.FLAG_DIGEST_SHA3_256, ms.DIGEST_KECCAK256, ms.DIGEST_SHA3_256) == (KECCAK, SHA3, 4, 5)
    leafs = np.arange(16, dtype=np.uint64)
    roots = {}
    for d in DIGESTS:
        ctx = make(0, ZAE | FLAG[d])
        assert hasattr(ctx.L, "ms_digest") and ctx.L.ms_digest(ctx.h) == d and ctx.digest == d
        rc, _, root = ctx.merkle_commit(leafs, 1, 2, 2)
        with pk.as_keccak(pk.SUFFIX[d]):   # pyref's own tree over the scalar sponge
            want = pyref.merkle_nodes([(i,) for i in range(16)], 2, 2, True)[-1]
        assert rc == 0 and root == want and root == tree(d, leafs, 1, 2, 2)[-1].tobytes()
        roots[d] = root
    for flags, digest in ((ZAE, 0), (ZAE | B2, 1), (ZAE | B3, 2)):
        other = make(0, flags)
        assert other.L.ms_digest(other.h) == digest and other.digest == digest
        rc, _, r = other.merkle_commit(leafs, 1, 2, 2)
        assert rc == 0
        roots[digest] = r
    assert roots[0].hex().startswith(dc.ROOT_0_15_SHA256) and roots[1].hex() == dc.ROOT_0_15_BLAKE2S
    assert len(set(roots.values())) == 5
    for a, b in itertools.combinations((B2, B3, KECCAK, SHA3), 2):   # a context has one D
        with pytest.raises(ms.MsError) as e:
            make(0, ZAE | a | b)
        assert e.value.code == ERR_ARG
    with pytest.raises(ms.MsError) as e:
        make(0, ZAE | B2 | B3 | KECCAK | SHA3)
    assert e.value.code == ERR_ARG


def case_every_node(ctx, d, field, leaf_num, ext, lpn, ic, zae):
    e = ext or EXT[field]
    leafs = dc._special_leafs(field, leaf_num * e, seed=leaf_num + lpn)
    rc, nodes, root = ctx.merkle_commit(leafs, e, lpn, ic)
    n = leaf_num // lpn
    m = n
    while m > 1 and m % ic == 0:
        m //= ic
    if leaf_num % lpn or n == 0 or m != 1 or ic & (ic - 1):   # merkle.rs:93-104 panics
        assert rc == pc.ERR_SHAPE
        return
    assert rc == 0, ctx.last_error()
    want = tree(d, leafs, e, lpn, ic, zae)
    assert nodes.shape == want.shape
    bad = np.nonzero((nodes != want).any(axis=1))[0]
    assert bad.size == 0, f"first wrong node {bad[0]} of {len(want)}"
    assert root == want[-1].tobytes()


def case_every_height(ctx, d, field, max_log, zae):
    for h in range(1, max_log + 1):
        leafs = dc._special_leafs(field, 2 << h, seed=h)
        rc, nodes, root = ctx.merkle_commit(leafs, 1, 2, 2)
        assert rc == 0, ctx.last_error()
        want = tree(d, leafs, 1, 2, 2, zae)
        assert (nodes == want).all() and root == want[-1].tobytes(), f"2^{h} leaf groups"


def case_merkle_prove(ctx, d, field, leaf_num=64):
    """ms_merkle_prove: the path of a leaf found by value holds the siblings of the expected tree (extension-field leaves, lpn 2)"""
    e = EXT[field]
    leafs = pc.rand_field(field, (leaf_num, e), seed=leaf_num + e)
    nodes = tree(d, leafs, e, 2, 2)
    for idx in (0, 3, leaf_num - 1):
        rc, path = ctx.merkle_prove(leafs.reshape(-1), leafs[idx], e, 2)
        assert rc == 0, ctx.last_error()
        head = 8 + 2 * e * 8 + 8
        got_idx, nlev = int.from_bytes(path[:8], "little"), int.from_bytes(path[head - 8:head], "little")
        assert got_idx == idx and len(path) == head + 64 * nlev
        assert [path[head + 64 * l:head + 64 * l + 64] for l in range(nlev)] == pk.expected_path(nodes, leaf_num // 2, idx)


def case_length_edges(make, d, field, lpns, lazy):
    """lazy: MS_LEAF_LAZY_MIN at ms_create forces the LAZY (True) or the plain (False) leaf kernel.  Every message length from 0 to lpn * max digits for each lpn
    (digest_cases.edge_groups); the lengths around one and two rate blocks must be among them."""
    ctx = make(field, ZAE | FLAG[d], env={"MS_LEAF_LAZY_MIN": "1" if lazy else "1000000"})
    sets = [(lpn,) + dc.edge_groups(field, lpn) for lpn in lpns]
    present = set()
    for lpn, leafs, _ in sets:
        present |= {len(m) for m in pk.leaf_messages(leafs, 1, lpn, True)}
    for t in RATE_EDGES:
        assert t in present, f"no message of {t} bytes in the input"
    for lpn, leafs, lengths in sets:
        msgs = pk.leaf_messages(leafs, 1, lpn, True)
        assert [len(m) for m in msgs] == lengths
        rc, nodes, root = ctx.merkle_commit(leafs, 1, lpn, 2)
        assert rc == 0, ctx.last_error()
        want = tree(d, leafs, 1, lpn, 2)
        bad = np.nonzero((nodes != want).any(axis=1))[0]
        assert bad.size == 0, f"lpn {lpn}: first wrong node {bad[0]}" + (f" (message of {lengths[bad[0]]} bytes)" if bad[0] < len(lengths) else "")
        assert root == want[-1].tobytes()


def check_proof_outputs(d, field, trace, nq, out, trees=None):
    """digest_cases.check_proof_outputs with the expected trees of `tree`: every root of `out` is the root of the expected tree over the values read back, every
    Merkle path of the MSFP blob holds that tree's siblings."""
    o, e = dict(out), EXT[field]
    w = trace.shape[1]
    rounds = sum(1 for k in o if k.startswith("round_info"))
    if trees is None:
        trees = {"trace": tree(d, trace, 1, 2 * w, 2), "lde": tree(d, o["lde"], 1, 2 * w, 2)}
        for i in range(rounds):
            trees[i] = tree(d, o[f"round_cw{i}"], e, 2, 2)
    assert o["trace_root"] == trees["trace"][-1].tobytes()
    assert o["lde_root"] == trees["lde"][-1].tobytes()
    for i in range(rounds):
        assert o[f"fri_root{i}"] == trees[i][-1].tobytes(), f"root of FRI round {i}"
    _, paths = pk.fri_paths(o["fri_proof"], e, rounds - 1, nq)
    for win, idx, levels in paths:
        D = o[f"round_info{win}"][1]
        assert levels == pk.expected_path(trees[win], D // 2, idx), f"Merkle path of window {win}, leaf {idx}"
    return trees


def tail_variants(d):
    f = ZAE | FLAG[d]
    return [("fused tail", f, {"MS_FRI_TAIL_MAX": "65536"}), ("launch per step", f, {"MS_FRI_TAIL_MAX": "0"}), ("latency", f | LATENCY, None)]


def case_whole_proof(make, d, field, log_n, blowup, variants=None, seed=77):
    """parity_cases.drive on a SHA-256 context and on contexts of digest `d` (`variants`: (name, flags, env)) with the same (trace, seed): whatever is not a digest
    equals the SHA-256 proof's, every digest is the expected tree's."""
    variants = variants or [("default", ZAE | FLAG[d], None)]
    trace = fibonacci_trace_fast(field, 1 << log_n)
    nq_fri = 2
    nq = nq_fri + 2   # drive adds two fixed betas
    e = EXT[field]
    sha = pc.drive(dc.NumpySession(make(field, ZAE)), field, trace, blowup, nq_fri, seed)
    trees, first = None, None
    for name, flags, env in variants:
        ctx = make(field, flags, env=env)
        assert ctx.digest == d
        kk = pc.drive(dc.NumpySession(ctx), field, trace, blowup, nq_fri, seed)
        ctx.close()
        assert [k for k, _ in kk] == [k for k, _ in sha]
        for (k, vs), (_, vk) in zip(sha, kk):
            if not dc._is_digest_output(k):   # the challenges are inputs: whatever is not a digest does not depend on D
                assert dc._same(vs, vk), f"{name}: stage output {k} differs between the digests"
            else:
                assert not dc._same(vs, vk), f"{name}: {k} equals the SHA-256 proof's"
        rounds = sum(1 for k, _ in kk if k.startswith("round_info"))
        ps, _ = pk.fri_paths(dict(sha)["fri_proof"], e, rounds - 1, nq)
        pq, _ = pk.fri_paths(dict(kk)["fri_proof"], e, rounds - 1, nq)
        assert ps == pq, f"{name}: points / quotients / opened leaves of the FRI proof differ between the digests"
        trees = check_proof_outputs(d, field, trace, nq, kk, trees)
        if first is None:
            first = kk
        else:
            for (k, v0), (_, v1) in zip(first, kk):
                assert dc._same(v0, v1), f"{name}: stage output {k} differs from the first variant's"


def case_roundtrip_and_cross_rejection(make, field, steps, blowup):
    """prove -> MSSP -> verify through the C++ mirror and the Python mirror with each of the five digests; a proof made under one digest is rejected under each of
    the other four; a flipped byte in the last Merkle path is rejected."""
    from mini_stark_amd.host import HostStark
    from mini_stark_amd.stark import Stark, StarkConfig, fibonacci_air
    ctxs = {0: make(field, ZAE), 1: make(field, ZAE | B2), 2: make(field, ZAE | B3), 4: make(field, ZAE | KECCAK), 5: make(field, ZAE | SHA3)}
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
    assert len(set(wire.values())) == 5
    for d in ctxs:
        for o in ctxs:
            if o != d:
                assert not hs[d].verify_bytes(cons, wire[o]) and hs[d].last_verify_error, f"verifier over digest {d} accepted a proof made under digest {o}"
                assert not hs[d].verify(cons, pyproof[o]), f"verifier over digest {d} accepted the Python mirror's proof made under digest {o}"
    for d in DIGESTS:
        bad = bytearray(wire[d]); bad[-1] ^= 1   # a byte of the LAST Merkle path's top level
        assert not hs[d].verify_bytes(cons, bytes(bad)) and "Merkle" in hs[d].last_verify_error


def case_shard_fails_closed(make, d, field=0):
    import ctypes as C
    from mini_stark_amd._native import EXCHANGE_FN
    ctx = make(field, ZAE | FLAG[d])
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
    assert rc == 0 and root == tree(d, leafs, 1, 2, 2)[-1].tobytes() and calls == []


def case_msh_hash():
    """msh_hash of the host mirror: id 5 against hashlib, id 4 against pyref_keccak, lengths 0 ... 300 and a few above 1000; stark.py's wrappers, incremental update
    included; the unassigned id 3 and id 6 are refused"""
    from mini_stark_amd.host import hash_bytes
    from mini_stark_amd.stark import DIGEST_HASH
    import mini_stark_amd as ms
    msgs = [bytes((11 * i + n) % 256 for i in range(n)) for n in list(range(301)) + [1087, 1088, 1089, 4000]]
    want4 = pk.hash_many(msgs, 0x01)
    for i, m in enumerate(msgs):
        assert hash_bytes(5, m) == hashlib.sha3_256(m).digest(), f"SHA3-256 of {len(m)} bytes"
        assert hash_bytes(4, m) == want4[i].tobytes(), f"Keccak-256 of {len(m)} bytes"
    for m, hexd in KECCAK256_VECTORS:
        assert hash_bytes(4, m).hex() == hexd and DIGEST_HASH[4](m).hexdigest() == hexd
    assert DIGEST_HASH[5] is hashlib.sha3_256
    for d in DIGESTS:
        for m in msgs[::37]:
            assert DIGEST_HASH[d](m).digest() == hash_bytes(d, m)
        h = DIGEST_HASH[d](b"ab"); h.update(b"c")
        assert h.digest() == hash_bytes(d, b"abc") and h.copy().hexdigest() == h.hexdigest()
    assert DIGEST_HASH[4](b"abc").hexdigest() == KECCAK256_VECTORS[1][1]
    for bad in (3, 6):
        with pytest.raises(ms.MsError):
            hash_bytes(bad, b"")
