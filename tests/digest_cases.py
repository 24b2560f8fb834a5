"""Cases for BLAKE2s-256 as the context's digest (MS_FLAG_DIGEST_BLAKE2S), shared by the emulation suite (tests/test_digest_emu.py) and the GPU suite
(tests/test_digest_gpu.py).  `make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set.
Expected digests come from hashlib (tests/pyref_digest.py)."""
import numpy as np

import parity_cases as pc
import pyref
import pyref_digest as pd
from common import MODULUS, EXT, SplitMix64, fibonacci_trace_fast

ZAE, LATENCY, B2 = 1, 4, 8   # MS_FLAG_ZERO_DISPLAY_EMPTY, MS_FLAG_LATENCY, MS_FLAG_DIGEST_BLAKE2S
ROOT_0_15_SHA256 = "2dde637a"
ROOT_0_15_BLAKE2S = "0e7ab796eed0c16d63a49ede406024c3679f2a435ed60ce1ef51a93ea0b522b6"
MERKLE_SHAPES = [(16, 1, 2, 2), (16, 1, 4, 2), (16, 1, 4, 4), (16, 1, 16, 16), (2, 1, 2, 2), (3, 1, 2, 2), (4096, 1, 2, 2), (6144, 1, 6, 2), (24, 1, 6, 2),
                 (1 << 13, 0, 2, 2), (64, 0, 2, 2)]   # (leaf_num, ext (0: the field's extension degree), lpn, ic) of test_emu_parity.py::test_merkle
EDGE_LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 192]


def case_flag_selects_blake2s(make):
    ctx = make(0, ZAE | B2)
    assert hasattr(ctx.L, "ms_digest") and ctx.L.ms_digest(ctx.h) == 1 and ctx.digest == 1
    rc, _, root = ctx.merkle_commit(np.arange(16, dtype=np.uint64), 1, 2, 2)
    assert rc == 0 and root.hex() == ROOT_0_15_BLAKE2S
    sha = make(0, ZAE)
    assert sha.L.ms_digest(sha.h) == 0 and sha.digest == 0
    rc, _, root = sha.merkle_commit(np.arange(16, dtype=np.uint64), 1, 2, 2)
    assert rc == 0 and root.hex().startswith(ROOT_0_15_SHA256)
    with pd.as_blake2s():   # the stand-in namespace gives pyref's own tree the same root
        assert pyref.merkle_nodes([(i,) for i in range(16)], 2, 2, True)[-1].hex() == ROOT_0_15_BLAKE2S


def _special_leafs(field, n, seed):
    """random canonical values with the directed values of parity_cases.directed_values (zeros, small values, p - 1, every digit-count boundary, the chunk
    fix-up grid) sprinkled in"""
    leafs = pc.rand_field(field, (n,), seed=seed)
    for i, v in enumerate(pc.directed_values(field)):
        leafs[(i * 5) % n] = v
    return leafs


def case_every_node(ctx, field, leaf_num, ext, lpn, ic, zae):
    e = ext or EXT[field]
    leafs = _special_leafs(field, leaf_num * e, seed=leaf_num + lpn)
    rc, nodes, root = ctx.merkle_commit(leafs, e, lpn, ic)
    n = leaf_num // lpn
    m = n
    while m > 1 and m % ic == 0:
        m //= ic
    if leaf_num % lpn or n == 0 or m != 1:   # merkle.rs:93-104 panics
        assert rc == pc.ERR_SHAPE
        return
    assert rc == 0, ctx.last_error()
    want = pd.tree_nodes(leafs, e, lpn, ic, zae)
    assert nodes.shape == want.shape and (nodes == want).all()
    assert root == want[-1].tobytes()


def case_every_height(ctx, field, max_log, zae):
    for h in range(1, max_log + 1):
        leafs = _special_leafs(field, 2 << h, seed=h)
        rc, nodes, root = ctx.merkle_commit(leafs, 1, 2, 2)
        assert rc == 0, ctx.last_error()
        want = pd.tree_nodes(leafs, 1, 2, 2, zae)
        assert (nodes == want).all() and root == want[-1].tobytes(), f"2^{h} leaf groups"


def case_merkle_prove(ctx, field, leaf_num=64):
    """ms_merkle_prove on a BLAKE2s context: the path of a leaf found by value holds the siblings of the hashlib tree (extension-field leaves, lpn 2)"""
    e = EXT[field]
    leafs = pc.rand_field(field, (leaf_num, e), seed=leaf_num + e)
    nodes = pd.tree_nodes(leafs, e, 2, 2, True)
    for idx in (0, 3, leaf_num - 1):
        rc, path = ctx.merkle_prove(leafs.reshape(-1), leafs[idx], e, 2)
        assert rc == 0, ctx.last_error()
        head = 8 + 2 * e * 8 + 8
        got_idx, nlev = int.from_bytes(path[:8], "little"), int.from_bytes(path[head - 8:head], "little")
        assert got_idx == idx and len(path) == head + 64 * nlev
        assert [path[head + 64 * l:head + 64 * l + 64] for l in range(nlev)] == pd.expected_path(nodes, leaf_num // 2, idx)


def edge_groups(field, lpn):
    """Leaf groups (lpn base elements each, zero printed empty) whose messages have every length from 0 to lpn * max digits, EDGE_LENGTHS several times over,
    ordered so that neighbouring groups - neighbouring lanes of a workgroup - differ widely in length and end on different blocks."""
    p = MODULUS[field]
    maxd = len(str(p - 1))
    top = lpn * maxd
    lengths = list(range(top + 1)) + [t for t in EDGE_LENGTHS if t <= top] * 4
    n = 1
    while n < len(lengths):
        n <<= 1
    lengths += [lengths[(7 * i) % len(lengths)] for i in range(n - len(lengths))]
    lengths = [lengths[(g * 37) % n] for g in range(n)]   # 37 is odd: a permutation
    leafs = np.zeros(n * lpn, dtype=np.uint64)
    for g, total in enumerate(lengths):
        digs = [0] * lpn
        left, k = total, g   # the digits go round the elements from element g on: zeros (empty strings) land anywhere in the group
        while left > 0:
            add = min(maxd - digs[k % lpn], left)
            digs[k % lpn] += add
            left -= add
            k += 1
        for j, d in enumerate(digs):
            leafs[g * lpn + j] = 0 if d == 0 else 10 ** (d - 1) + (g * 31 + j) % 9
    assert int(leafs.max()) < p
    return leafs, lengths


def case_length_edges(make, field, lpns, lazy):
    """lazy: MS_LEAF_LAZY_MIN at ms_create forces the two-block (True) or the plain (False) leaf kernel"""
    ctx = make(field, ZAE | B2, env={"MS_LEAF_LAZY_MIN": "1" if lazy else "1000000"})
    sets = [(lpn,) + edge_groups(field, lpn) for lpn in lpns]
    present = set()
    for lpn, leafs, _ in sets:
        present |= {len(m) for m in pd.leaf_messages(leafs, 1, lpn, True)}
    for t in EDGE_LENGTHS:
        assert t in present, f"no message of {t} bytes in the input"
    for lpn, leafs, lengths in sets:
        msgs = pd.leaf_messages(leafs, 1, lpn, True)
        assert [len(m) for m in msgs] == lengths
        rc, nodes, root = ctx.merkle_commit(leafs, 1, lpn, 2)
        assert rc == 0, ctx.last_error()
        want = pd.tree_nodes(leafs, 1, lpn, 2, True)
        bad = np.nonzero((nodes != want).any(axis=1))[0]
        assert bad.size == 0, f"lpn {lpn}: first wrong node {bad[0]}" + (f" (message of {lengths[bad[0]]} bytes)" if bad[0] < len(lengths) else "")
        assert root == want[-1].tobytes()


class _Kept(np.ndarray):
    def tolist(self):   # parity_cases.drive lists what it reads back; at 2^21 rows that is tens of millions of Python integers - keep the array
        return self.view(np.ndarray)


class NumpySession:
    """A Context whose read-backs stay numpy arrays through parity_cases.drive"""
    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        f = getattr(self._ctx, name)
        if name in ("poly_read", "lde_read", "validity_read", "fri_round_poly", "fri_round_codeword"):
            return lambda *a: f(*a).view(_Kept)
        return f


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def _is_digest_output(key):
    return key.endswith("_root") or key.startswith("fri_root") or key == "fri_proof"


def check_proof_outputs(field, trace, nq, out, digest, trees=None):
    """Every root of `out` (the stage outputs of parity_cases.drive) is the root of the hashlib tree over the values read back, and every Merkle path of the MSFP
    blob holds the siblings of that tree.  Returns the trees (trace, lde, one per round) so that variants of the same proof share them."""
    o, e = dict(out), EXT[field]
    w = trace.shape[1]
    rounds = sum(1 for k in o if k.startswith("round_info"))
    if trees is None:
        trees = {"trace": pd.tree_nodes(trace, 1, 2 * w, 2, True, digest), "lde": pd.tree_nodes(o["lde"], 1, 2 * w, 2, True, digest)}
        for i in range(rounds):
            trees[i] = pd.tree_nodes(o[f"round_cw{i}"], e, 2, 2, True, digest)
    assert o["trace_root"] == trees["trace"][-1].tobytes()
    assert o["lde_root"] == trees["lde"][-1].tobytes()
    for i in range(rounds):
        assert o[f"fri_root{i}"] == trees[i][-1].tobytes(), f"root of FRI round {i}"
    _, paths = pd.fri_paths(o["fri_proof"], e, rounds - 1, nq)
    for win, idx, levels in paths:
        D = o[f"round_info{win}"][1]
        assert levels == pd.expected_path(trees[win], D // 2, idx), f"Merkle path of window {win}, leaf {idx}"
    return trees


def case_whole_proof(make, field, log_n, blowup, variants=(("default", ZAE | B2, None),), seed=77, against_pyprover=False):
    """parity_cases.drive on a SHA-256 context and on BLAKE2s contexts (`variants`: (name, flags, env)) with the same (trace, seed)."""
    trace = fibonacci_trace_fast(field, 1 << log_n)
    nq_fri = 2
    nq = nq_fri + 2   # drive adds two fixed betas
    e = EXT[field]
    sha = pc.drive(NumpySession(make(field, ZAE)), field, trace, blowup, nq_fri, seed)
    check_proof_outputs(field, trace, nq, sha, pd.SHA256)
    trees, first = None, None
    for name, flags, env in variants:
        ctx = make(field, flags, env=env)
        assert ctx.digest == 1
        b2 = pc.drive(NumpySession(ctx), field, trace, blowup, nq_fri, seed)
        ctx.close()
        assert [k for k, _ in b2] == [k for k, _ in sha]
        for (k, vs), (_, vb) in zip(sha, b2):
            if not _is_digest_output(k):   # the challenges are inputs: whatever is not a digest does not depend on D
                assert _same(vs, vb), f"{name}: stage output {k} differs between the digests"
        rounds = sum(1 for k, _ in b2 if k.startswith("round_info"))
        ps, _ = pd.fri_paths(dict(sha)["fri_proof"], e, rounds - 1, nq)
        pb, _ = pd.fri_paths(dict(b2)["fri_proof"], e, rounds - 1, nq)
        assert ps == pb, f"{name}: points / quotients / opened leaves of the FRI proof differ between the digests"
        trees = check_proof_outputs(field, trace, nq, b2, pd.BLAKE2S, trees)
        if first is None:
            first = b2
        else:
            for (k, v0), (_, v1) in zip(first, b2):
                assert _same(v0, v1), f"{name}: stage output {k} differs from the first variant's"
    if against_pyprover:
        with pd.as_blake2s():
            _against_pyprover(field, trace, blowup, nq_fri, seed, first)


def _against_pyprover(field, trace, blowup, nq_fri, seed, out):
    """tests/pyref.py's PyProver (big integers, hashlib) end to end, with drive's challenge schedule"""
    p, e = MODULUS[field], EXT[field]
    N, w = trace.shape
    o = dict(out)
    rng = SplitMix64(seed)
    y = pyref.PyProver(field, True)
    assert y.trace_commit(trace, 2 * w) == o["trace_root"]
    y.interpolate()
    from common import fibonacci_closures
    from oracle import oracle as orc
    for sc, idx in fibonacci_closures(field, N, orc.root_of_unity(field, N)):
        y.lincomb(sc, idx)
    shift = rng.nonzero(p)
    assert y.lde_commit(blowup, shift, 2 * w) == o["lde_root"]
    assert np.array_equal(np.asarray(o["lde"]), np.array(y.lde, dtype=np.uint64))
    y.mix(rng.field(p))
    zs = [[rng.field(p) for _ in range(e)] for _ in range(2)]
    assert o["ood"] == [[list(v) for v in row] for row in y.eval_ext(zs)]
    rounds = sum(1 for k in o if k.startswith("round_info"))
    assert y.fri_begin(blowup, rounds) == o["fri_root0"]
    for i in range(1, rounds):
        B = y.fri_deep([rng.field(p) for _ in range(e)])
        assert o[f"B{i}"] == [c for b in B for c in b]
        assert y.fri_fold_commit([rng.field(p) for _ in range(e)]) == o[f"fri_root{i}"]
    betas = [rng.next() for _ in range(nq_fri)] + [3, 2 * N * blowup]
    assert y.serialise_fri(y.fri_query(betas)) == o["fri_proof"]


def case_roundtrip_and_cross_rejection(make, field, steps, blowup):
    """prove -> verify through the C++ mirror (msh_stark_prove / msh_stark_verify_mssp) and the Python mirror (stark.Stark.prove) with either digest; a proof made
    with one digest is rejected by a verifier configured with the other; a flipped byte in a Merkle path is rejected."""
    from mini_stark_amd.host import HostStark
    from mini_stark_amd.stark import Stark, StarkConfig, fibonacci_air
    ctxs = {d: make(field, ZAE | (B2 if d else 0)) for d in (0, 1)}
    hs, wire, cons = {}, {}, None
    for d, ctx in ctxs.items():
        tt = fibonacci_air(ctx, steps)
        hs[d] = HostStark(ctx, 20, blowup, steps, tt.constrain_number())
        if cons is None:
            cons = hs[d].derive_constrains(tt)   # (polynomials: the same for both digests)
        proof = hs[d].prove(tt)
        wire[d] = hs[d].proof_bytes()
        py = Stark(StarkConfig(ctx, 20, blowup, steps, tt.constrain_number())).prove(tt)   # the Python mirror draws the same challenges from the same chain
        assert py.to_bytes() == wire[d] and proof.arthur == py.arthur
        assert hs[d].verify_bytes(cons, wire[d]), hs[d].last_verify_error
        assert hs[d].verify(cons, py), hs[d].last_verify_error
    assert wire[0] != wire[1]
    for d in (0, 1):
        assert not hs[d].verify_bytes(cons, wire[1 - d]) and hs[d].last_verify_error
    # a byte of the LAST Merkle path's top level under the digest that made the proof
    bad = bytearray(wire[1]); bad[-1] ^= 1
    assert not hs[1].verify_bytes(cons, bytes(bad)) and "Merkle" in hs[1].last_verify_error


def case_shard_fails_closed(make, field=0):
    import ctypes as C
    from mini_stark_amd._native import EXCHANGE_FN, ERR_ARG
    ctx = make(field, ZAE | B2)
    calls = []
    cb = EXCHANGE_FN(lambda user, op, nbytes: calls.append((op, nbytes)) or 0)
    buf = (C.c_uint8 * 8192)()
    ctx.L.ms_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, EXCHANGE_FN, C.c_void_p]
    rc = ctx.L.ms_set_shard(ctx.h, 0, 2, C.addressof(buf), C.addressof(buf) + 4096, 4096, cb, None)
    assert rc == ERR_ARG and "SHA-256 only" in ctx.last_error()
    ctx.L.ms_set_shard_rccl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    assert ctx.L.ms_set_shard_rccl(ctx.h, 0, 2, bytes(128), 1 << 20) == ERR_ARG and "SHA-256 only" in ctx.last_error()
    # the context is unsharded and whole: a commitment goes through without a single exchange
    rc, _, root = ctx.merkle_commit(np.arange(16, dtype=np.uint64), 1, 2, 2)
    assert rc == 0 and root.hex() == ROOT_0_15_BLAKE2S and calls == []
