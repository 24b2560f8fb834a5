"""Directed decimal corners through every VIEW the leaf-hash kernel (csrc/merkle.hpp LeafHashKernel) reads its input by, shared by the emulation suite
(tests/test_views_emu.py) and the GPU suite (tests/test_views_gpu.py).  parity_cases.case_merkle brings the directed values (parity_cases.directed_values) to the
kernel through ms_merkle_commit only - an array of leaves, width 1; here they travel through the views the prover commits with: the transposed trace
(width = w, any leafs_per_node), the LDE matrix with stored and VIRTUAL columns (values chosen on the coset), the FRI round-0 codeword (limb stride), the
deferred pad-only lists of SHA-256 filled to capacity, and the runs / output offset of the sharded commitments on a one-rank world.

`make(field, flags, env=None, fresh=False)` returns a mini_stark_amd.Context created with `flags` while the variables of `env` are set (a context of its own
when env is given or fresh is true).  Every expected value comes from the references of the suite (the oracle; hashlib and the numpy hashes of pyref_*), applied to
the row-major matrix the view stands for - never to anything read back from the library under test.  All comparisons are bit-exact."""
import ctypes as C
import functools
import json

import numpy as np

import keccak_cases as kc
import parity_cases as pc
import pyref_blake3 as pb3
import pyref_digest as pd
from common import MODULUS, SplitMix64
from oracle import oracle as orc

ZAE, MONT64 = 1, 2                              # MS_FLAG_ZERO_DISPLAY_EMPTY, MS_FLAG_TRACE_MONT64
SHA, B2, B3, KECCAK, SHA3 = 0, 1, 2, 4, 5       # ms_digest_id
FLAG = {SHA: 0, B2: 8, B3: 0x10, KECCAK: 0x20, SHA3: 0x40}
OTHER_DIGESTS = (B2, B3, KECCAK, SHA3)


def flags(digest, zae=True):
    return FLAG[digest] | (ZAE if zae else 0)


def ref_nodes(digest, values, ext, lpn, zae=True):
    """every node of the binary tree over `values` (row-major, element-major limbs), level-major, root last"""
    values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    if digest == SHA:
        rc, nodes, _ = orc.merkle_build(values, ext, lpn, 2, 1 if zae else 0)
        assert rc == 0
        return nodes
    if digest == B2:
        return pd.tree_nodes(values, ext, lpn, 2, zae)
    if digest == B3:
        return pb3.tree_nodes(values, ext, lpn, 2, zae)
    return kc.tree(digest, values, ext, lpn, 2, zae)


def ref_root(digest, values, ext, lpn, zae=True):
    return ref_nodes(digest, values, ext, lpn, zae)[-1].tobytes()


def _coprime_stride(size, w):
    """an odd stride (size is a power of two times w) that shares no factor with w: j -> j * stride mod size visits every position once and walks the columns"""
    s = 7
    while np.gcd(s, w) != 1 or np.gcd(s, size) != 1:
        s += 2
    return s


def directed_matrix(field, N, w, seed=0, lpns=()):
    """N x w random canonical values with the directed values strewn over the row-major matrix at a stride coprime to w (the list cycled over up to half the matrix,
    all of a matrix that is smaller than the list), a zero and a one-digit value put into every column, and for every leafs_per_node of `lpns` a zero as the first
    element of one leaf group and as the last element of another: every column holds empty / short texts, and some messages begin and some end with one."""
    vals = pc.directed_values(field)
    t = pc.rand_field(field, (N, w), seed=1000 * w + N + seed)
    flat = t.reshape(-1)
    size = flat.size
    s = _coprime_stride(size, w)
    for j in range(min(size, max(len(vals), size // 2))):
        flat[(j * s) % size] = vals[j % len(vals)]
    for c in range(w):
        t[(3 * c + 1) % N, c] = 0
        t[(5 * c + 2) % N, c] = 1 + c % 9
    for lpn in lpns:
        groups = size // lpn
        flat[(groups // 3) * lpn] = 0
        flat[(2 * groups // 3) * lpn + lpn - 1] = 0
    assert all((t[:, c] == 0).any() and (t[:, c] < 10).sum() >= 2 for c in range(w))
    assert all((flat[0::lpn] == 0).any() and (flat[lpn - 1::lpn] == 0).any() for lpn in lpns)
    if size >= 2 * len(vals) + 2 * w:
        assert set(vals) <= set(flat.tolist())
    return t


# ------------------------------------------------------------------ 1. trace view: transposed columns, width = w, col_stride = N
# (log2 N, w, leafs_per_node ...): the plain and the two-block (lpn >= 16) leaf kernel; groups inside a row, equal to a row and spanning up to 16 rows; the plain
# transpose (w < 16, or fewer than 64 rows) and the tiled one
TRACE_SHAPES = [(6, 1, (1, 2, 16, 32)), (6, 2, (1, 2, 4, 16, 32)), (6, 3, (3, 6, 12, 24, 48)), (6, 5, (5, 10, 20)), (7, 16, (1, 2, 8, 16, 32, 64)), (7, 17, (17, 34)),
                (8, 64, (4, 64, 128)), (5, 16, (16,))]
OTHER_DIGEST_TRACE_SHAPES = [TRACE_SHAPES[2], TRACE_SHAPES[4]]
# one shape per kernel forced the other way with MS_LEAF_LAZY_MIN
FORCED_KERNEL = [(6, 3, (3, 6), "1"), (7, 16, (16, 32, 64), "1000000")]
ENTRY_SHAPES = [(6, 3, (3, 12)), (7, 16, (2, 64)), (7, 17, (17,)), (5, 16, (16,))]


def case_trace_view(ctx, digest, field, log_n, w, lpns, zae):
    N = 1 << log_n
    trace = directed_matrix(field, N, w, lpns=lpns)
    for lpn in lpns:
        rc, root = ctx.trace_commit(trace, lpn)
        assert rc == 0, ctx.last_error()
        want = ref_root(digest, trace, 1, lpn, zae)
        assert root == want, f"trace view 2^{log_n} x {w}, {lpn} leaves per node, digest {digest}"
        if digest == SHA and w == 3:   # the oracle's tree once more from hashlib
            assert want == pd.tree_nodes(trace, 1, lpn, 2, zae, pd.SHA256)[-1].tobytes()


def case_trace_entries(make, field, to_device, pinned):
    """The same root from ms_trace_commit_device, from a MS_FLAG_TRACE_MONT64 context fed x * 2^64 mod p (host and device pointer), and - pinned - from a page-locked
    source that ms_trace_upload_async prefetched and from one it did not.  `to_device(array) -> (pointer, keepalive)`."""
    p = MODULUS[field]
    R = (1 << 64) % p
    ctx, mctx = make(field, ZAE), make(field, ZAE | MONT64)
    own = make(field, ZAE, fresh=True) if pinned else None
    held = []
    for log_n, w, lpns in ENTRY_SHAPES:
        N = 1 << log_n
        trace = np.ascontiguousarray(directed_matrix(field, N, w, seed=5, lpns=lpns))
        mont = np.array([int(v) * R % p for v in trace.reshape(-1)], dtype=np.uint64).reshape(N, w)
        if pinned:
            pp = own.pinned_alloc(trace.nbytes)
            assert pp
            held.append(pp)
            C.memmove(pp, trace.ctypes.data, trace.nbytes)
        for i, lpn in enumerate(lpns):
            want = ref_root(SHA, trace, 1, lpn)
            what = f"2^{log_n} x {w}, {lpn} leaves per node"
            ptr, keep = to_device(trace)
            assert ctx.trace_commit_device(ptr, N, w, lpn) == (0, want), what
            assert mctx.trace_commit(mont, lpn) == (0, want), what
            mptr, mkeep = to_device(mont)
            assert mctx.trace_commit_device(mptr, N, w, lpn) == (0, want), what
            del keep, mkeep
            if pinned:
                if i == 0:
                    assert own.trace_upload_async(pp, N, w) == 0, own.last_error()
                assert own.trace_commit_ptr(pp, N, w, lpn) == (0, want), what
    if pinned:
        own.close()
        for pp in held:
            own.pinned_free(pp)


# ------------------------------------------------------------------ 2. LDE view: stored and virtual columns, values chosen on the coset
LDE_N, LDE_LPNS = 64, (3, 6, 12, 24)   # c = 6 columns: half a row, a row, 2 and 4 rows per group; 24 selects the two-block kernel


def lde_chunks(field):
    return (len(pc.directed_values(field)) + LDE_N - 1) // LDE_N


def coset_column(field, V, shift):
    """The values on the trace domain of the polynomial of degree < N that takes the values V on the coset shift * H_N (V[k] at shift * w^k): interpolate Q(x) =
    P(shift x) on H_N, unscale coefficient k by shift^-k, evaluate on H_N."""
    p = MODULUS[field]
    q = orc.intt(field, np.array(V, dtype=np.uint64))
    inv = pow(shift, -1, p)
    coef = np.array([int(c) * pow(inv, k, p) % p for k, c in enumerate(q)], dtype=np.uint64)
    return orc.ntt(field, coef)


@functools.lru_cache(maxsize=None)
def lde_inputs(field, chunk):
    """(trace 64 x 3, shift, V2, V3, program A, program B).  On the coset shift * H_N - the rows k * blowup of the LDE - stored column 2 takes the values V2 and
    s0 * P0 + s1 * P1 the values V3 (a chunk of the directed values, forwards and backwards).  Program A: [s0, s1] over [0, 1]; [1, p-1] over [2, 2], identically
    zero; [1, p-1, s0, s1] over [0, 0, 0, 1], LIN_MAXT terms and the three arithmetic branches in one column (again V3).  Program B: the last column gets a fifth
    term, + P2 (V3 + V2): more than LIN_MAXT, the whole table falls back to written columns."""
    p = MODULUS[field]
    vals = pc.directed_values(field)
    rng = SplitMix64(4000 + 10 * chunk + field)
    V3 = [vals[(chunk * LDE_N + i) % len(vals)] for i in range(LDE_N)]
    V2 = V3[::-1]
    shift = rng.nonzero(p)
    s0, s1 = [2 + rng.next() % (p - 3) for _ in range(2)]   # neither 0, 1 nor p - 1: the general branch
    L0 = [rng.field(p) for _ in range(LDE_N)]
    inv1 = pow(s1, -1, p)
    L1 = [(v - s0 * a) * inv1 % p for v, a in zip(V3, L0)]
    trace = np.stack([coset_column(field, L, shift) for L in (L0, L1, V2)], axis=1)
    trace.setflags(write=False)
    A = (((s0, s1), (0, 1)), ((1, p - 1), (2, 2)), ((1, p - 1, s0, s1), (0, 0, 0, 1)))
    B = A[:2] + (((1, p - 1, s0, s1, 1), (0, 0, 0, 1, 2)),)
    return trace, shift, V2, V3, A, B


@functools.lru_cache(maxsize=None)
def lde_oracle(field, zae, blowup, chunk, prog):
    """The oracle's LDE matrix and its roots per leafs_per_node, with the directed values asserted ON THIS MATRIX: a construction that lost them fails here."""
    p = MODULUS[field]
    trace, shift, V2, V3, A, B = lde_inputs(field, chunk)
    o = orc.Session(field, 1 if zae else 0)
    assert o.trace_commit(trace, 3)[0] == 0 and o.interpolate() == 0
    for sc, idx in (A, B)[prog]:
        assert o.polys_lincomb(list(sc), list(idx)) == 0
    roots = {}
    for lpn in LDE_LPNS:
        rc, roots[lpn] = o.lde_commit(blowup, shift, lpn)
        assert rc == 0
    M = o.lde_read()
    o.close()
    assert M.shape == (LDE_N * blowup, 6)
    D = M[::blowup]
    assert D[:, 2].tolist() == V2 and D[:, 3].tolist() == V3, "the directed columns do not hold the directed values on the coset"
    assert not M[:, 4].any(), "the zero column is not zero"
    assert D[:, 5].tolist() == (V3 if prog == 0 else [(a + b) % p for a, b in zip(V3, V2)])
    M.setflags(write=False)
    return M, roots


def _profiled(ctx, call):
    """(result of call(), launches per kernel while it ran)"""
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    out = call()
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    return out, {k: v["launches"] for k, v in json.loads(buf.value.decode()).items() if isinstance(v, dict) and "launches" in v}


def case_lde_view(make, field, zae, blowup, virtual):
    """ms_lde_commit root and ms_lde_read against the oracle for both programs, every chunk of the directed values and every leafs_per_node, with MS_LDE_VIRTUAL
    = `virtual` at ms_create.  The per-kernel profile says which way the linear columns went: no lincomb launch in a commitment with virtual columns."""
    ctx = make(field, flags(SHA, zae), env={"MS_LDE_VIRTUAL": virtual})
    stored, virt = set(), set()
    for chunk in range(lde_chunks(field)):
        trace, shift, V2, V3, A, B = lde_inputs(field, chunk)
        for prog in (0, 1):
            M, roots = lde_oracle(field, zae, blowup, chunk, prog)
            assert ctx.trace_commit(trace, 3)[0] == 0 and ctx.interpolate() == 0, ctx.last_error()
            for sc, idx in (A, B)[prog]:
                assert ctx.polys_lincomb(list(sc), list(idx)) == 0, ctx.last_error()
            for lpn in LDE_LPNS:
                what = f"chunk {chunk}, program {'AB'[prog]}, {lpn} leaves per node"
                (rc, root), launches = _profiled(ctx, lambda: ctx.lde_commit(blowup, shift, lpn))
                assert rc == 0, ctx.last_error()
                assert root == roots[lpn], what
                assert (launches["lincomb"] == 0) == (virtual == "1" and prog == 0), (what, launches)
                assert (ctx.lde_read() == M).all(), what
            if prog == 0:
                stored |= set(M[::blowup, 2].tolist())
                virt |= set(M[::blowup, 3].tolist()) & set(M[::blowup, 5].tolist())
    ctx.close()
    want = set(pc.directed_values(field))
    assert want <= stored and want <= virt, "a directed value reached no stored / no virtual column"


def case_lde_view_other_digest(make, digest, field, blowup):
    """lpn in {6, 24} with virtual columns under the other digests: the pyref tree over the oracle's LDE matrix"""
    ctx = make(field, flags(digest), env={"MS_LDE_VIRTUAL": "1"})
    for chunk in range(lde_chunks(field)):
        trace, shift, V2, V3, A, B = lde_inputs(field, chunk)
        M, _ = lde_oracle(field, True, blowup, chunk, 0)
        assert ctx.trace_commit(trace, 3)[0] == 0 and ctx.interpolate() == 0, ctx.last_error()
        for sc, idx in A:
            assert ctx.polys_lincomb(list(sc), list(idx)) == 0, ctx.last_error()
        for lpn in (6, 24):
            (rc, root), launches = _profiled(ctx, lambda: ctx.lde_commit(blowup, shift, lpn))
            assert rc == 0, ctx.last_error()
            assert launches["lincomb"] == 0, launches
            assert root == ref_root(digest, M, 1, lpn), f"digest {digest}, chunk {chunk}, {lpn} leaves per node"
    ctx.close()


# ------------------------------------------------------------------ 3. FRI round-0 codeword view (EL = E, limb_stride = D) and the path kernels
FRI_N, FRI_BLOWUP, FRI_DISTINCT = 64, 4, 32   # 32 directed values per proof, each twice: true duplicates


def fri_chunks(field):
    return (len(pc.directed_values(field)) + FRI_DISTINCT - 1) // FRI_DISTINCT


@functools.lru_cache(maxsize=None)
def fri_trace(field, chunk):
    vals = pc.directed_values(field)
    t = pc.rand_field(field, (FRI_N, 3), seed=6000 + chunk)
    t[:, 0] = [vals[(chunk * FRI_DISTINCT + i % FRI_DISTINCT) % len(vals)] for i in range(FRI_N)]
    t.setflags(write=False)
    return t


def drive_fri(sess, field, trace, blowup, seed, nbetas=5):
    """A proof whose validity polynomial is polynomial 0 (ms_mix with r = 0) on `sess` (oracle Session or Context): every root, round, codeword and the MSFP blob"""
    p, e = MODULUS[field], sess.e
    N = trace.shape[0]
    rng = SplitMix64(seed)
    out = []
    rc, root = sess.trace_commit(trace, 6)
    assert rc == 0
    out.append(("trace_root", root))
    assert sess.interpolate() == 0
    rc, root = sess.lde_commit(blowup, rng.nonzero(p), 6)
    assert rc == 0
    out.append(("lde_root", root))
    assert sess.mix(0) == 0
    out.append(("validity", sess.validity_read().tolist()))
    rounds = int(orc.lib().or_ceil_log2_k(C.c_uint64((N - 1) * blowup + 1), C.c_uint64(2)))
    rc, root = sess.fri_begin(blowup, rounds)
    assert rc == 0
    out.append(("fri_root0", root))
    for i in range(1, rounds):
        rc, B = sess.fri_deep([rng.field(p) for _ in range(e)])
        assert rc == 0
        out.append((f"B{i}", B.tolist()))
        rc, root = sess.fri_fold_commit([rng.field(p) for _ in range(e)])
        assert rc == 0
        out.append((f"fri_root{i}", root))
    for i in range(rounds):
        out.append((f"round_info{i}", tuple(sess.fri_round_info(i))))
        out.append((f"round_cw{i}", sess.fri_round_codeword(i).tolist()))
    rc, proof = sess.fri_query([rng.next() for _ in range(nbetas)] + [0, 1, 2 * N * blowup - 1])
    assert rc == 0
    out.append(("fri_proof", proof))
    return out


@functools.lru_cache(maxsize=None)
def fri_oracle(field, chunk):
    trace = fri_trace(field, chunk)
    o = orc.Session(field)
    want = drive_fri(o, field, trace, FRI_BLOWUP, seed=90 + chunk)
    o.close()
    d = dict(want)
    assert d["validity"] == orc.intt(field, trace[:, 0]).tolist()                     # polynomial 0
    cw = np.array(d["round_cw0"], dtype=np.uint64)
    assert cw.shape[0] == FRI_N * FRI_BLOWUP
    assert (cw[::FRI_BLOWUP, 0] == trace[:, 0]).all() and not cw[:, 1:].any(), "the round-0 codeword does not hold the directed values at stride blowup"
    return want


def case_fri_view(make, field, tail_max):
    """tail_max: MS_FRI_TAIL_MAX at ms_create ("0": a launch per step; None: the default, whose fused rounds hash their leaves without deferred-block lists)"""
    ctx = make(field, ZAE, env={} if tail_max is None else {"MS_FRI_TAIL_MAX": tail_max}, fresh=True)
    for chunk in range(fri_chunks(field)):
        want = fri_oracle(field, chunk)
        got, launches = _profiled(ctx, lambda: drive_fri(ctx, field, fri_trace(field, chunk), FRI_BLOWUP, seed=90 + chunk))
        assert [k for k, _ in got] == [k for k, _ in want]
        for (k, a), (_, b) in zip(got, want):
            assert a == b, f"chunk {chunk}: stage output {k} differs from the oracle's"
        assert (launches["fri_tail"] > 0) == (tail_max is None), launches
    ctx.close()


# ------------------------------------------------------------------ 4. SHA-256: deferred pad-only lists at capacity
# digits per element of a group: 56 bytes (the length does not fit the message's last block: every group defers a pad-only block) / 55 bytes (none does)
PAD_DIGITS = {True: {0: (19, 19, 18), 1: (10, 10, 9, 9, 9, 9)}, False: {0: (19, 18, 18), 1: (10, 9, 9, 9, 9, 9)}}


@functools.lru_cache(maxsize=None)
def pad_groups(field, log_groups, defer):
    """(groups x lpn values that differ from group to group, every node of the oracle's tree over them)"""
    p = MODULUS[field]
    rng = np.random.default_rng(7000 + log_groups + field)
    n = 1 << log_groups
    leafs = np.stack([rng.integers(10 ** (d - 1), min(10 ** d, p), n, dtype=np.uint64) for d in PAD_DIGITS[defer][field]], axis=1)
    lpn = leafs.shape[1]
    lens = np.array([len(m) for m in pd.leaf_messages(leafs, 1, lpn, True)])
    assert lens.size == n, "a group was left out"
    deferring = (lens % 64 >= 56)
    assert deferring.all() if defer else not deferring.any()
    assert len({r.tobytes() for r in leafs[:4096]}) == 4096
    nodes = ref_nodes(SHA, leafs, 1, lpn)
    leafs.setflags(write=False)
    nodes.setflags(write=False)
    return leafs, nodes


def case_pad_lists(ctx, field, log_groups, defer=True):
    """2^16 groups: 256 workgroups, one per list, each list exactly full; 2^17: two workgroups per list; 2^19: 8 workgroups' entries per list, more than PAD_GRID_Y
    workgroups of PadOnlyBlockKernel take in one step.  Through ms_merkle_commit (every node) and through the trace view (w = lpn: the same tree)."""
    leafs, nodes = pad_groups(field, log_groups, defer)
    lpn = leafs.shape[1]
    rc, got, root = ctx.merkle_commit(leafs.reshape(-1), 1, lpn, 2)
    assert rc == 0, ctx.last_error()
    bad = np.nonzero((got != nodes).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} wrong nodes, first {bad[0]}"
    assert root == nodes[-1].tobytes()
    assert ctx.trace_commit(leafs, lpn) == (0, nodes[-1].tobytes())


# ------------------------------------------------------------------ 5. sharded views on one rank: runs (run_len / run_stride) and the output offset
SHARD_LOG_N, SHARD_BLOWUP, SHARD_SLICES = 7, 8, 4
SHARD_ENVS = {"default": {}, "sliced": {"MS_SHARD_SLICES": str(SHARD_SLICES), "MS_SHARD_SLICE_MIN": "8"}, "replicated": {"MS_SHARD_DIST": "0"}}


def case_sharded_views(make_ctx, set_env, field, rccl=False, device=None):
    """The directed 2^7 x 3 matrix through the sharded prover on a one-rank world (MS_SHARD_WORLD1=1, MS_SHARD_MIN_LEAVES=16): defaults, the digest exchange in four
    slices, and MS_SHARD_DIST=0; every stage output against the oracle (parity_cases.case_sharded_paths_on_one_rank).
    Which counter shows the sliced launches: tree_build_sharded hashes a commitment in S launches of the leaf kernel over runs (and S of PadOnlyBlockKernel) instead
    of one, and hands every slice to exchange_slice, which counts ONE all-to-all per commitment in ms_shard_stats whatever S is - that count cannot tell.  What can:
    the `leaf_hash` launches of the per-kernel profile (2 (S - 1) more per sliced commitment), and, where the exchanges are callbacks, the number of
    MS_XCHG_ALL_TO_ALL_SLICE calls (S per sliced commitment).  The sharded commitments here are the LDE (1024 leaf groups) and the FRI rounds of 512 ... 16 leaf
    groups (MS_SHARD_MIN_LEAVES): all but the last are sliced, and that one - 16 groups, 4 per slice, fewer than MS_SHARD_SLICE_MIN - goes out in one piece."""
    trace = directed_matrix(field, 1 << SHARD_LOG_N, 3, seed=9)
    set_env("MS_SHARD_WORLD1", "1")
    set_env("MS_SHARD_MIN_LEAVES", "16")
    res = {}
    for name, env in SHARD_ENVS.items():
        for k, v in env.items():
            set_env(k, v)
        info = {}
        st, dist_rounds = pc.case_sharded_paths_on_one_rank(make_ctx, field, SHARD_LOG_N, SHARD_BLOWUP, rccl=rccl, device=device, trace=trace, info=info)
        for k in env:
            set_env(k, None)
        res[name] = (st, dist_rounds, info["calls"], info["profile"]["leaf_hash"]["launches"])
    set_env("MS_SHARD_WORLD1", None)
    set_env("MS_SHARD_MIN_LEAVES", None)
    (st, dist_rounds, calls, leaf), (st_s, dist_s, calls_s, leaf_s), (st_r, dist_r, calls_r, leaf_r) = res["default"], res["sliced"], res["replicated"]
    assert dist_rounds >= 2 and dist_s == dist_rounds and dist_r == 0, (dist_rounds, dist_s, dist_r)
    assert st[0] >= 3 and st_s[:4] == st[:4], (st, st_s)           # the digest all-to-alls: the LDE and the sharded rounds, counted once per commitment
    assert st_r[0] >= 3, st_r
    sliced = st[0] - 1
    assert leaf_s == leaf + 2 * (SHARD_SLICES - 1) * sliced, (leaf, leaf_s, st)
    if not rccl:
        assert calls[4] == 0 and calls_r[4] == 0 and calls[0] == st[0], (calls, calls_r, st)
        assert calls_s[4] == SHARD_SLICES * sliced and calls_s[0] == 1, (calls_s, st)
