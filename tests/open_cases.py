"""Cases of ms_tree_open and ms_fri_query_index (openings by index; include/ministark.h - build-defined, no reference counterpart), shared by the emulation suite
(tests/test_open_emu.py) and the GPU suite (tests/test_open_gpu.py).  Expected bytes: tests/pyref_open.py over trees hashed by hashlib / pyref_blake3 / pyref_keccak;
every comparison is exact.  The verifying side is checked twice: msh_merkle_path_check_index / msh_fri_index_verify (the host library) and pyref_open's big-integer
restatement must agree on every blob, whole or tampered.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set; `d` is the ms_digest_id."""
import ctypes as C
import json
import struct

import numpy as np

import mini_stark_amd as ms
import pyref
import pyref_open as ro
from common import MODULUS, EXT, SplitMix64, fibonacci_trace, fibonacci_closures
from grind_cases import FLAG
from mini_stark_amd.host import fri_index_verify, merkle_path_check_index
from parity_cases import drive, rand_field

ZAE = 1
LATENCY = 4
DIGESTS = (ro.SHA256, ro.BLAKE3, ro.KECCAK256)
HEIGHTS = (1, 2, 16, 32, 1 << 12)   # leaf groups: nlevels 0, 1, 4, 5 (80 path words: more than one pass of a wave), 12
_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)


def ctx_of(make, d, field=0, extra=0, env=None):
    ctx = make(field, ZAE | FLAG[d] | extra, env)
    assert ctx.digest == d
    return ctx


def raw_open(ctx, tree, rnd, index, n, out, cap, want_len=True):
    """ms_tree_open with the arguments as given (index: a list or None; out: a ctypes buffer or None) -> (rc, *len)"""
    ix = None if index is None else np.ascontiguousarray(index, dtype=np.uint64)
    ln = C.c_size_t(0xDEAD)
    rc = ctx.L.ms_tree_open(ctx.h, C.c_int(tree), C.c_int(rnd), None if ix is None else ix.ctypes.data_as(_u64p), C.c_size_t(n), out, C.c_size_t(cap),
                            C.byref(ln) if want_len else None)
    return rc, ln.value


def raw_query_index(ctx, betas, nq, out, cap, want_len=True):
    b = None if betas is None else np.ascontiguousarray(betas, dtype=np.uint64)
    ln = C.c_size_t(0xDEAD)
    rc = ctx.L.ms_fri_query_index(ctx.h, None if b is None else b.ctypes.data_as(_u64p), C.c_int(nq), out, C.c_size_t(cap), C.byref(ln) if want_len else None)
    return rc, ln.value


def index_lists(ngroups):
    """index 0, the last, a middle one, and a list with duplicates in descending order"""
    mid = ngroups // 2
    lists = [[0], [ngroups - 1], [mid]]
    desc = sorted({ngroups - 1, mid, (2 * ngroups) // 3, ngroups // 3, 0}, reverse=True)
    lists.append([desc[0]] + desc + [desc[-1], desc[0]])
    return lists


def check_paths(ctx, d, field, blob, values, ext, lpn, nodes, root, indices):
    """the bytes of one ms_tree_open call against pyref_open, and every path through both positional checkers against `root`"""
    want = b"".join(ro.path_at(values, ext, lpn, nodes, g) for g in indices)
    assert blob == want
    assert bytes(nodes[-1]) == root
    p = MODULUS[field]
    pos = 0
    for g in indices:
        rc, used = merkle_path_check_index(d, field, ext, lpn, True, root, blob[pos:], g)
        ok, used2 = ro.check_path_index(d, p, ext, lpn, True, root, blob[pos:], g)
        assert rc == 1 and ok and used == used2 == ro.path_size(ext, lpn, len(nodes) // 2 + 1)
        pos += used
    assert pos == len(blob)


# ---------------------------------------------------------------- 1. tree heights, on the trace tree (one row of w = 2 columns per leaf group)
def case_tree_heights(make, d, field, extra=0, heights=HEIGHTS):
    ctx = ctx_of(make, d, field, extra)
    for ngroups in heights:
        trace = rand_field(field, (ngroups, 2), seed=ngroups + 17 * field)
        trace[0, 0] = 0                                # (a zero prints as the empty string)
        rc, root = ctx.trace_commit(trace, 2)
        assert rc == 0, ctx.last_error()
        nodes = ro.tree_nodes(d, trace.reshape(-1, 1), 1, 2)
        if d == ro.SHA256 and ngroups <= 32:           # the tree of pyref.merkle_nodes, node for node
            assert [bytes(n) for n in nodes] == pyref.merkle_nodes([(int(v),) for v in trace.reshape(-1)], 2, 2)
        for ix in index_lists(ngroups):
            check_paths(ctx, d, field, ctx.tree_open(ms.TREE_TRACE, ix), trace.reshape(-1, 1), 1, 2, nodes, root, ix)
        # a wrong group, and a path whose two halves of one level are swapped: rejected where "either half" would pass
        if ngroups >= 2:
            blob = ctx.tree_open(ms.TREE_TRACE, [1])
            assert merkle_path_check_index(d, field, 1, 2, True, root, blob, 1)[0] == 1
            assert merkle_path_check_index(d, field, 1, 2, True, root, blob, 0)[0] == 0
            head = 8 + 2 * 8 + 8
            swapped = blob[:head] + blob[head + 32:head + 64] + blob[head:head + 32] + blob[head + 64:]
            assert merkle_path_check_index(d, field, 1, 2, True, root, swapped, 1)[0] == 0
            assert not ro.check_path_index(d, MODULUS[field], 1, 2, True, root, swapped, 1)[0]


def case_trace_tree(make, d, field):
    """a leaf group that is two rows (lpn = 2 w, the grouping of the proofs); after ms_interpolate the tree is gone"""
    ctx = ctx_of(make, d, field)
    N, w = 16, 3
    trace = fibonacci_trace(field, N)
    rc, root = ctx.trace_commit(trace, 2 * w)
    assert rc == 0
    nodes = ro.tree_nodes(d, trace.reshape(-1, 1), 1, 2 * w)
    for ix in index_lists(N // 2):
        check_paths(ctx, d, field, ctx.tree_open(ms.TREE_TRACE, ix), trace.reshape(-1, 1), 1, 2 * w, nodes, root, ix)
    assert raw_open(ctx, ms.TREE_LDE, 0, [0], 1, None, 0)[0] == ms.ERR_STATE          # not yet
    assert raw_open(ctx, ms.TREE_FRI, 0, [0], 1, None, 0)[0] == ms.ERR_STATE
    assert ctx.interpolate() == 0
    rc, ln = raw_open(ctx, ms.TREE_TRACE, 0, [0], 1, None, 0)
    assert rc == ms.ERR_STATE and "interpolate" in ctx.last_error()
    rc, root2 = ctx.trace_commit(trace, 2 * w)                                      # a new trace: the tree is back
    assert rc == 0 and root2 == root
    check_paths(ctx, d, field, ctx.tree_open(ms.TREE_TRACE, [3]), trace.reshape(-1, 1), 1, 2 * w, nodes, root, [3])


# ---------------------------------------------------------------- 2. LDE rows
def build_lde(ctx, field, c, N=16, blowup=4, seed=3):
    """a trace with an ms_aux_running extension column (c = 65), lincomb columns and an appended column, committed with one row per leaf group: (root, L, the
    lincomb launches of the commit - none when the linear columns are virtual, i.e. only ever hashed)"""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(seed + c)
    if c == 1:
        w, naux, nlin, napp = 1, 0, 0, 0
    elif c == 3:
        w, naux, nlin, napp = 1, 0, 1, 1
    else:
        naux, nlin, napp = e, 2, 2
        w = c - naux - nlin - napp
    trace = rand_field(field, (N, w), seed=seed + 100 * c)
    rc, _ = ctx.trace_commit(trace, w)
    assert rc == 0, ctx.last_error()
    if naux:
        gamma = tuple(rng.nonzero(p) for _ in range(e))
        one = (1,) + (0,) * (e - 1)
        rc, _fin, _col = ctx.aux_running(ms.AUX_SUM, [((one, []), (gamma, [(0, one)]))], ext=e)
        assert rc == 0, ctx.last_error()
    assert ctx.interpolate() == 0
    assert ctx.polys_count() == w + naux
    for k in range(nlin):
        srcs = [k % (w + naux), (k + 1) % (w + naux)] if w + naux > 1 else [0]
        sc = [p - 1, rng.nonzero(p)][:len(srcs)]
        assert ctx.polys_lincomb(sc, srcs) == 0
    for k in range(napp):
        assert ctx.polys_append([rng.field(p) for _ in range(N - k)]) == 0
    assert ctx.polys_count() == c
    (rc, root), prof = profile(ctx, lambda: ctx.lde_commit(blowup, rng.nonzero(p), c))
    assert rc == 0, ctx.last_error()
    return root, N * blowup, prof["lincomb"]["launches"]


def case_lde_rows(make, d, field, c, env=None, virtual=None):
    """every row of the committed LDE opened BEFORE ms_lde_read (a virtual column is then opened from its specification) and again after it: both times the rows
    ms_lde_read returns, under the LDE root"""
    ctx = ctx_of(make, d, field, env=env)
    root, L, lincombs = build_lde(ctx, field, c)
    assert virtual is None or (lincombs == 0) == virtual   # (the form of the linear columns the case is about)
    rows = list(range(L))
    before = ctx.tree_open(ms.TREE_LDE, rows)
    lde = ctx.lde_read()
    assert lde.shape == (L, c)
    after = ctx.tree_open(ms.TREE_LDE, rows)
    assert before == after
    nodes = ro.tree_nodes(d, lde.reshape(-1, 1), 1, c)
    check_paths(ctx, d, field, before, lde.reshape(-1, 1), 1, c, nodes, root, rows)
    paths = ro.split_paths(before, 1, c)
    for r in rows:                                     # row for row
        assert struct.unpack_from("<%dQ" % c, paths[r], 8) == tuple(int(v) for v in lde[r])
    for ix in index_lists(L)[3:]:
        check_paths(ctx, d, field, ctx.tree_open(ms.TREE_LDE, ix), lde.reshape(-1, 1), 1, c, nodes, root, ix)
    assert ctx.polys_append([1, 2, 3]) == 0           # the polynomials changed: the committed LDE is no longer theirs
    assert raw_open(ctx, ms.TREE_LDE, 0, [0], 1, None, 0)[0] == ms.ERR_STATE


# ---------------------------------------------------------------- the FRI commit phase, driven by hand
def prepare(ctx, field, trace, blowup, seed):
    """trace -> validity polynomial (the Fibonacci closures as three lincomb polynomials, ms_mix); the SplitMix64 the challenges come from"""
    p = MODULUS[field]
    N, w = trace.shape
    rng = SplitMix64(seed)
    assert ctx.trace_commit(trace, 2 * w)[0] == 0
    assert ctx.interpolate() == 0
    for sc, idx in fibonacci_closures(field, N, ctx.root_of_unity(N)):
        assert ctx.polys_lincomb(sc, idx) == 0
    assert ctx.lde_commit(blowup, rng.nonzero(p), 2 * w)[0] == 0
    assert ctx.mix(rng.field(p)) == 0
    return rng


def commit_phase(ctx, field, blowup, R, seed):
    """ms_fri_begin and R - 1 rounds with challenges from SplitMix64(seed): what the verifier is given"""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(seed)
    rc, root = ctx.fri_begin(blowup, R)
    assert rc == 0, ctx.last_error()
    S = dict(field=field, blowup=blowup, R=R, roots=[root], zs=[], Bs=[], alphas=[])
    for _ in range(1, R):
        z = [rng.field(p) for _ in range(e)]
        rc, B = ctx.fri_deep(z)
        assert rc == 0, ctx.last_error()
        a = [rng.field(p) for _ in range(e)]
        rc, root = ctx.fri_fold_commit(a)
        assert rc == 0, ctx.last_error()
        S["roots"].append(root); S["zs"].append(tuple(z)); S["alphas"].append(tuple(a))
        S["Bs"].append((tuple(int(v) for v in B[:e]), tuple(int(v) for v in B[e:])))
    S["D0"] = ctx.fri_round_info(0)[1]
    return S


def expected_rounds(ctx, d, S, cache=None):
    """codewords and trees of the committed rounds (a tree is rebuilt from the codeword ms_fri_round_codeword_read returns and must end at the committed root);
    `cache`: {root: (codeword, nodes)} shared by commit phases that repeat rounds"""
    e = EXT[S["field"]]
    cws, nodes = [], []
    for r in range(S["R"]):
        hit = None if cache is None else cache.get(S["roots"][r])
        if hit is None:
            cw = ctx.fri_round_codeword(r)
            hit = (cw, ro.tree_nodes(d, cw, e, 2))
            assert bytes(hit[1][-1]) == S["roots"][r]
            if cache is not None:
                cache[S["roots"][r]] = hit
        cws.append(hit[0]); nodes.append(hit[1])
    return cws, nodes, ctx.fri_round_poly(S["R"] - 1)


def verify_both(d, S, betas, blob):
    """(host library's verdict, pyref_open's verdict, the library's why) - which must agree"""
    rc, why = fri_index_verify(d, S["field"], True, S["blowup"], S["roots"], S["zs"], S["Bs"], S["alphas"], betas, blob)
    ok, _ = ro.verify_msfi(S["field"], d, True, S["blowup"], S["roots"], S["zs"], S["Bs"], S["alphas"], betas, blob)
    assert rc in (0, 1) and (rc == 1) == ok, (rc, ok, why)
    assert rc == 1 or why
    return rc == 1, why


def beta_sets(D0):
    """0, D0 - 1, D0, D0 + 1, a 64-bit value and two equal betas, in calls of 3 and of 1"""
    big = 0xDEADBEEFCAFEF00D
    return [[0, D0 - 1, D0], [D0 + 1, big, D0 + 1], [big], [D0]]


# ---------------------------------------------------------------- 3. FRI round trees, every round of a small proof
def case_fri_rounds(make, d, field, extra=0, log_n=4, blowup=4):
    ctx = ctx_of(make, d, field, extra)
    prepare(ctx, field, fibonacci_trace(field, 1 << log_n), blowup, seed=21)
    R = log_n + blowup.bit_length() - 1
    S = commit_phase(ctx, field, blowup, R, seed=22)
    assert S["D0"] == (1 << log_n) * blowup and ctx.fri_round_info(R - 1)[1] == 2   # the last round's tree is one leaf group
    e = EXT[field]
    cws, nodes, _ = expected_rounds(ctx, d, S)
    for r in range(R):
        groups = len(cws[r]) // 2
        ix = list(range(groups)) + index_lists(groups)[3]
        check_paths(ctx, d, field, ctx.tree_open(ms.TREE_FRI, ix, r), cws[r], e, 2, nodes[r], S["roots"][r], ix)
    assert raw_open(ctx, ms.TREE_FRI, R, [0], 1, None, 0)[0] == ms.ERR_ARG
    assert raw_open(ctx, ms.TREE_FRI, -1, [0], 1, None, 0)[0] == ms.ERR_ARG


# ---------------------------------------------------------------- 4. refusals
def case_refusals(make, d, field):
    ctx, fresh = ctx_of(make, d, field), ctx_of(make, d, field)
    N, w = 16, 3
    trace = fibonacci_trace(field, N)
    for c in (ctx, fresh):
        assert c.trace_commit(trace, w)[0] == 0
    want = fresh.tree_open(ms.TREE_TRACE, [5, 0])
    size = len(want)
    buf = (C.c_uint8 * (size + 8))(*([0xAB] * (size + 8)))
    untouched = bytes(buf)

    def valid():
        assert ctx.tree_open(ms.TREE_TRACE, [5, 0]) == want

    assert raw_open(ctx, ms.TREE_TRACE, 0, [5, 0], 2, None, 0) == (0, size); valid()                  # the size query
    assert raw_open(ctx, ms.TREE_TRACE, 0, [5, 0], 2, buf, size - 1) == (ms.ERR_ARG, size)            # one byte short: nothing computed
    assert bytes(buf) == untouched; valid()
    assert raw_open(ctx, ms.TREE_TRACE, 0, None, 2, buf, size)[0] == ms.ERR_ARG; valid()              # null index
    assert raw_open(ctx, ms.TREE_TRACE, 0, [5, 0], 2, buf, size, want_len=False)[0] == ms.ERR_ARG; valid()   # null len
    assert raw_open(ctx, ms.TREE_TRACE, 0, [5, 0], 2, None, size)[0] == ms.ERR_ARG; valid()           # null out with a capacity
    assert raw_open(ctx, ms.TREE_TRACE, 0, [5, 0], 0, buf, size)[0] == ms.ERR_ARG; valid()            # n outside 1..65536
    assert raw_open(ctx, ms.TREE_TRACE, 0, [0] * 65537, 65537, None, 0)[0] == ms.ERR_ARG; valid()
    assert raw_open(ctx, 3, 0, [5, 0], 2, buf, size)[0] == ms.ERR_ARG; valid()                        # unknown tree id
    assert raw_open(ctx, -1, 0, [5, 0], 2, buf, size)[0] == ms.ERR_ARG; valid()
    assert raw_open(ctx, ms.TREE_TRACE, 0, [5, N], 2, buf, size)[0] == ms.ERR_OUT_OF_RANGE; valid()   # an index at the number of leaf groups
    assert raw_open(ctx, ms.TREE_TRACE, 0, [2**64 - 1, 0], 2, buf, size)[0] == ms.ERR_OUT_OF_RANGE; valid()
    assert raw_open(ctx, ms.TREE_LDE, 0, [0], 1, buf, size)[0] == ms.ERR_STATE; valid()               # trees that do not exist yet
    assert raw_open(ctx, ms.TREE_FRI, 0, [0], 1, buf, size)[0] == ms.ERR_STATE; valid()
    assert bytes(buf) == untouched
    assert ctx.L.ms_tree_open(None, 0, 0, None, C.c_size_t(1), None, C.c_size_t(0), None) == ms.ERR_ARG
    assert raw_query_index(ctx, [1], 1, None, 0)[0] == ms.ERR_STATE; valid()                          # no commit phase
    # 65536 indices are allowed
    many = list(range(N)) * 4096
    blob = ctx.tree_open(ms.TREE_TRACE, many)
    assert len(blob) == 65536 * size // 2 and blob[:size // 2 * N] == fresh.tree_open(ms.TREE_TRACE, list(range(N)))
    # the query phase's own refusals, on a finished commit phase
    for c in (ctx, fresh):
        prepare(c, field, trace, 4, seed=5)
        commit_phase(c, field, 4, 3, seed=6)
    wq = fresh.fri_query_index([7, 9])
    qb = (C.c_uint8 * len(wq))()

    def validq():
        assert ctx.fri_query_index([7, 9]) == wq

    assert raw_query_index(ctx, [7, 9], 2, None, 0) == (0, len(wq)); validq()
    assert raw_query_index(ctx, [7, 9], 2, qb, len(wq) - 1) == (ms.ERR_ARG, len(wq)); validq()
    assert raw_query_index(ctx, None, 2, qb, len(wq))[0] == ms.ERR_ARG; validq()
    assert raw_query_index(ctx, [7, 9], 2, qb, len(wq), want_len=False)[0] == ms.ERR_ARG; validq()
    assert raw_query_index(ctx, [7, 9], 0, qb, len(wq))[0] == ms.ERR_ARG; validq()
    assert raw_query_index(ctx, [7] * 4097, 4097, None, 0)[0] == ms.ERR_ARG; validq()
    assert raw_query_index(ctx, [7] * 4096, 4096, None, 0)[0] == 0; validq()
    assert bytes(qb) == bytes(len(wq))
    assert ctx.fri_begin(4, 3)[0] == 0                                                                # a commit phase under way: not yet
    assert raw_query_index(ctx, [7, 9], 2, None, 0)[0] == ms.ERR_STATE
    assert raw_open(ctx, ms.TREE_FRI, 1, [0], 1, None, 0)[0] == ms.ERR_ARG                            # round 1 is not committed
    assert raw_open(ctx, ms.TREE_FRI, 0, [0], 1, None, 0)[0] == 0


def case_sharded(ctx):
    """a context with sharding on (a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses both entry points, as ms_aux_running does"""
    from mini_stark_amd.dist import LocalShard
    sh = LocalShard(ctx, 4 << 20)
    assert ctx.trace_commit(fibonacci_trace(0, 64), 3)[0] == 0
    assert raw_open(ctx, ms.TREE_TRACE, 0, [0], 1, None, 0)[0] == ms.ERR_STATE and "sharding" in ctx.last_error()
    assert raw_query_index(ctx, [1], 1, None, 0)[0] == ms.ERR_STATE
    sh.close()


# ---------------------------------------------------------------- 5. the context is unchanged
class Opening:
    """a Context whose every stage is followed by openings of whatever trees exist, and by the compact query phase once the commit phase is over"""
    STAGES = ("trace_commit", "interpolate", "polys_lincomb", "lde_commit", "lde_read", "mix", "eval_ext", "fri_begin", "fri_deep", "fri_fold_commit", "fri_query")

    def __init__(self, ctx):
        self.ctx, self.opened, self.rounds = ctx, {0: 0, 1: 0, 2: 0, "msfi": 0}, 0

    def __getattr__(self, name):
        fn = getattr(self.ctx, name)
        if name not in self.STAGES:
            return fn

        def stage(*a, **k):
            out = fn(*a, **k)
            self.after(name)
            return out
        return stage

    def after(self, name):
        ctx = self.ctx
        if name == "fri_begin":
            self.rounds = 1
        elif name == "fri_fold_commit":
            self.rounds += 1
        for tree, rnd in ((ms.TREE_TRACE, 0), (ms.TREE_LDE, 0), (ms.TREE_FRI, max(0, self.rounds - 1))):
            rc, n = raw_open(ctx, tree, rnd, [0, 0], 2, None, 0)
            assert rc in (0, ms.ERR_STATE), (name, tree, rc)
            if rc == 0:
                buf = (C.c_uint8 * n)()
                assert raw_open(ctx, tree, rnd, [0, 0], 2, buf, n)[0] == 0, ctx.last_error()
                self.opened[tree] += 1
        rc, n = raw_query_index(ctx, [3, 1 << 40], 2, None, 0)
        assert rc in (0, ms.ERR_STATE)
        if rc == 0:
            assert len(ctx.fri_query_index([3, 1 << 40])) == n
            self.opened["msfi"] += 1


def case_context_unchanged(make, d, field, extra=0, log_n=5, blowup=4):
    trace = fibonacci_trace(field, 1 << log_n)
    plain = drive(ctx_of(make, d, field, extra), field, trace, blowup, 2, seed=41)
    wrapped = Opening(ctx_of(make, d, field, extra))
    got = drive(wrapped, field, trace, blowup, 2, seed=41)
    assert [k for k, _ in got] == [k for k, _ in plain]
    for (k, a), (_, b) in zip(got, plain):
        assert a == b, f"stage output {k} differs with openings between the stages"
    assert all(v > 0 for v in wrapped.opened.values()), wrapped.opened


# ---------------------------------------------------------------- 6. the compact query phase
def case_query_index(make, d, field, N, blowup, tail, extra=0, all_rounds=True):
    """R from 1 to the most the domain allows (the fused tail on: default, or off), nq 1 and 3: the blob is pyref_open's, both verifiers accept"""
    ctx = ctx_of(make, d, field, extra, env=None if tail else {"MS_FRI_TAIL_MAX": "0"})
    e = EXT[field]
    prepare(ctx, field, fibonacci_trace(field, N), blowup, seed=N + blowup)
    Rmax = (N * blowup).bit_length() - 1
    cache = {}
    for R in (range(Rmax, 0, -1) if all_rounds else (Rmax,)):
        S = commit_phase(ctx, field, blowup, R, seed=7)
        assert S["D0"] == N * blowup
        cws, nodes, fin = expected_rounds(ctx, d, S, cache)
        for betas in beta_sets(S["D0"]):
            blob = ctx.fri_query_index(betas)
            assert blob == ro.msfi_blob(e, cws, nodes, fin, betas), (R, betas)
            assert verify_both(d, S, betas, blob)[0], (R, betas)
        if R == 1:
            assert len(blob) == 48 + len(fin) * e * 8
    assert len(cache) == Rmax                          # (the rounds of a shorter commit phase are the first rounds of the longest)


def case_pyprover(make, field=0):
    """the smallest shape against pyref.PyProver from the trace on: its rounds' evaluations and trees give the MSFI bytes"""
    N, blowup, e, p = 8, 2, EXT[field], MODULUS[field]
    ctx = ctx_of(make, ro.SHA256, field)
    trace = fibonacci_trace(field, N)
    prepare(ctx, field, trace, blowup, seed=11)
    R = 3
    S = commit_phase(ctx, field, blowup, R, seed=12)
    py = pyref.PyProver(field)
    r2 = SplitMix64(11)
    py.trace_commit(trace, 6); py.interpolate()
    for sc, idx in fibonacci_closures(field, N, pyref.root_of_unity(field, N)):
        py.lincomb(sc, idx)
    py.lde_commit(blowup, r2.nonzero(p), 6)
    py.mix(r2.field(p))
    assert py.fri_begin(blowup, R) == S["roots"][0]
    for i in range(R - 1):
        py.fri_deep(S["zs"][i])
        assert py.fri_fold_commit(S["alphas"][i]) == S["roots"][i + 1]
    cws = [np.array(r["ev"], dtype=np.uint64) for r in py.rounds]
    nodes = [np.frombuffer(b"".join(r["nodes"]), dtype=np.uint8).reshape(-1, 32) for r in py.rounds]
    fin = np.array(py.rounds[-1]["poly"], dtype=np.uint64).reshape(-1, e)
    for betas in beta_sets(S["D0"]):
        assert ctx.fri_query_index(betas) == ro.msfi_blob(e, cws, nodes, fin, betas)


def case_agreement_with_by_value(make, d, field, log_n=6, blowup=8, seeds=(1, 2)):
    """random traces: every MerklePath of MSFI is, byte for byte, the path of the same (window, query, side) inside ms_fri_query's MSFP blob - betas below D_0, so
    quirk Q6 does not bite; the codewords' values are pairwise distinct, so the lookup by value finds the position"""
    ctx = ctx_of(make, d, field)
    e, N = EXT[field], 1 << log_n
    for seed in seeds:
        trace = rand_field(field, (N, 3), seed=900 + seed)
        prepare(ctx, field, trace, blowup, seed=seed)
        R = log_n               # the opened rounds 0 .. R - 2 have polynomials of at least 3 coefficients (round i >= 1: N / 2^i - 1): no constant codeword among them
        S = commit_phase(ctx, field, blowup, R, seed=seed + 50)
        for r in range(R - 1):
            cw = ctx.fri_round_codeword(r)
            assert len({tuple(row) for row in cw.tolist()}) == len(cw), "the seeds must give codewords of pairwise distinct values"
        D0 = S["D0"]
        betas = [0, D0 - 1, D0 // 2, 1, D0 // 2 + 1, 12345 % D0, 12345 % D0]
        msfi = ctx.fri_query_index(betas)
        rc, msfp = ctx.fri_query(betas)
        assert rc == 0
        _, _, pi = ro.msfi_parse(msfi, e)
        pv = ro.msfp_paths(msfp, e, R - 1, len(betas))
        assert len(pi) == len(pv) == R - 1
        for i in range(R - 1):
            assert len(pi[i]) == len(pv[i]) == len(betas)
            for j in range(len(betas)):
                assert pi[i][j] == pv[i][j], (i, j)
        assert verify_both(d, S, betas, msfi)[0]


def case_constant_trace(make, d, field, blowup=8):
    """a constant trace: the validity polynomial is a constant, every codeword is one repeated value.  ms_fri_query opens position 0 whatever the beta (first match
    by value, quirk Q7) - on file here as the reason for the feature; ms_fri_query_index opens exactly the positions b_(i,j), and the verifier accepts"""
    ctx = ctx_of(make, d, field)
    e = EXT[field]
    trace = np.full((16, 3), 5, dtype=np.uint64)
    prepare(ctx, field, trace, blowup, seed=8)
    R = blowup.bit_length() - 1
    S = commit_phase(ctx, field, blowup, R, seed=9)
    assert S["D0"] == blowup and ctx.fri_round_info(0)[0] <= 1
    cws, nodes, fin = expected_rounds(ctx, d, S)
    assert all(len({tuple(r) for r in cw.tolist()}) == 1 for cw in cws)
    betas = [5, 3, blowup - 1]
    blob = ctx.fri_query_index(betas)
    assert blob == ro.msfi_blob(e, cws, nodes, fin, betas)
    _, _, paths = ro.msfi_parse(blob, e)
    want = ro.positions(betas, S["D0"], R - 1)
    for i in range(R - 1):
        for j in range(len(betas)):
            assert tuple(struct.unpack_from("<Q", paths[i][j][s], 0)[0] for s in range(2)) == want[i][j]
    assert any(pos != 0 for row in want for pair in row for pos in pair)
    assert verify_both(d, S, betas, blob)[0]
    rc, msfp = ctx.fri_query(betas)
    assert rc == 0
    for row in ro.msfp_paths(msfp, e, R - 1, len(betas)):
        for pair in row:
            assert [struct.unpack_from("<Q", pth, 0)[0] for pth in pair] == [0, 0]     # by value: position 0, every time


# ---------------------------------------------------------------- 7. tampering
def case_tampering(make, d, field, log_n=4, blowup=4):
    ctx = ctx_of(make, d, field)
    e, p = EXT[field], MODULUS[field]
    prepare(ctx, field, fibonacci_trace(field, 1 << log_n), blowup, seed=61)
    R = 3                                              # D_2 = 16: the final polynomial has N / 4 - 1 = 3 coefficients, one below the bound D_2 / blowup
    S = commit_phase(ctx, field, blowup, R, seed=62)
    betas = [9, 40]
    blob = ctx.fri_query_index(betas)
    assert verify_both(d, S, betas, blob)[0]
    hd, fin, paths = ro.msfi_parse(blob, e)
    nfinal, bound = hd[5], max(1, (S["D0"] >> (R - 1)) // blowup)
    assert 2 <= nfinal <= bound
    p0 = 48 + nfinal * e * 8                           # the first path: leaf_index | 2 e neighbours | nlevels | levels
    nb, lv = p0 + 8, p0 + 8 + 2 * e * 8

    def flip(at, bit=0):
        b = bytearray(blob); b[at] ^= 1 << bit
        return bytes(b)

    def rejected(b, S_=S, betas_=betas):
        ok, why = verify_both(d, S_, betas_, b)
        assert not ok and why
        return why
    for at in (0, 8, 16, 24, 32, 40):                  # every word of the header
        rejected(flip(at))
    rejected(flip(48))                                 # the final polynomial
    rejected(flip(48 + nfinal * e * 8 - 8))
    rejected(flip(p0))                                 # a leaf_index
    rejected(flip(p0, 1))
    rejected(flip(nb)); rejected(flip(nb + e * 8))     # a neighbour: the opened one, and the other
    rejected(flip(lv)); rejected(flip(lv, 3))          # nlevels
    rejected(flip(lv + 8)); rejected(flip(lv + 8 + 63)); rejected(flip(len(blob) - 1))   # sibling digests
    swapped = blob[:lv + 8] + blob[lv + 40:lv + 72] + blob[lv + 8:lv + 40] + blob[lv + 72:]
    assert "slot" in rejected(swapped)                 # the two halves of one level swapped: check_path's "either half" would let it through
    rejected(blob + b"\0")                             # one byte appended
    rejected(blob[:-1])
    # a non-canonical neighbour
    rejected(blob[:nb] + struct.pack("<Q", p) + blob[nb + 8:])
    # wrong root, z, alpha, B
    def but(key, i, v):
        T = dict(S); T[key] = list(S[key]); T[key][i] = v
        return T
    bump = lambda t: ((t[0] + 1) % p,) + tuple(t[1:])   # noqa: E731
    rejected(blob, but("roots", 0, bytes(32)))
    rejected(blob, but("roots", R - 2, S["roots"][R - 1]))
    for i in (0, R - 2):
        rejected(blob, but("zs", i, bump(S["zs"][i])))
        rejected(blob, but("alphas", i, bump(S["alphas"][i])))
        rejected(blob, but("Bs", i, (bump(S["Bs"][i][0]), S["Bs"][i][1])))
        rejected(blob, but("Bs", i, (S["Bs"][i][0], bump(S["Bs"][i][1]))))
    rejected(blob, betas_=[10, 40])                    # other positions than the verifier's
    # nfinal above the bound: a longer "final polynomial" (zero coefficients appended evaluate the same: only the length check can refuse it) ...
    pad = bound + 1 - nfinal
    longer = blob[:40] + struct.pack("<Q", nfinal + pad) + blob[48:p0] + bytes(8 * e * pad) + blob[p0:]
    assert "longer" in rejected(longer)
    fits = blob[:40] + struct.pack("<Q", bound) + blob[48:p0] + bytes(8 * e * (bound - nfinal)) + blob[p0:]
    assert verify_both(d, S, betas, fits)[0]            # ... and up to the bound it is accepted
    T = dict(S); T["blowup"] = S["D0"]                  # the same blob under a rate that allows one coefficient
    assert "longer" in rejected(blob, T)


# ---------------------------------------------------------------- 8. launches, order, repetition
def profile(ctx, fn):
    buf = C.create_string_buffer(1 << 15)
    assert ctx.L.ms_profile_begin(ctx.h) == 0
    out = fn()
    assert ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))) == 0
    return out, json.loads(buf.value.decode())


def case_launch_count(make, d, field, N=1 << 10, blowup=8):
    """at the largest R and nq of the drive: at most two launches, none of them a pass over a codeword or a polynomial"""
    ctx = ctx_of(make, d, field)
    prepare(ctx, field, fibonacci_trace(field, N), blowup, seed=71)
    R = (N * blowup).bit_length() - 1
    commit_phase(ctx, field, blowup, R, seed=72)
    betas = [1, 2, 3]
    blob, prof = profile(ctx, lambda: ctx.fri_query_index(betas))
    launches = {k: v["launches"] for k, v in prof.items() if isinstance(v, dict) and v.get("launches")}
    assert 1 <= sum(launches.values()) <= 2, launches
    assert set(launches) <= {"merkle_path", "io_copy"}, launches
    (rc, _), prof2 = profile(ctx, lambda: ctx.fri_query(betas))
    assert rc == 0 and sum(v["launches"] for v in prof2.values() if isinstance(v, dict) and "launches" in v) > 2
    _, prof3 = profile(ctx, lambda: ctx.tree_open(ms.TREE_LDE, list(range(64))))
    assert sum(v["launches"] for v in prof3.values() if isinstance(v, dict) and "launches" in v) == 1
    assert blob == ctx.fri_query_index(betas)


def case_order_and_repetition(make, d, field, log_n=5, blowup=4):
    """index then value, value then index, index twice: each call gives the bytes it gives alone"""
    trace = fibonacci_trace(field, 1 << log_n)
    R = log_n + blowup.bit_length() - 1
    betas = [3, 77, 1 << 50]

    def fresh():
        c = ctx_of(make, d, field)
        prepare(c, field, trace, blowup, seed=81)
        commit_phase(c, field, blowup, R, seed=82)
        return c
    a, b = fresh(), fresh()
    index_alone = a.fri_query_index(betas)
    value_alone = b.fri_query(betas)
    assert value_alone[0] == 0
    c = fresh()
    assert c.fri_query_index(betas) == index_alone and c.fri_query(betas) == value_alone           # index then value
    assert c.fri_query_index(betas) == index_alone and c.fri_query_index(betas) == index_alone     # ... value then index, index twice
    assert c.fri_proof_read() == value_alone[1]                                                     # the MSFP blob stays readable
    c = fresh()
    assert c.fri_query(betas) == value_alone and c.fri_query_index(betas) == index_alone           # value then index
    assert c.fri_query(betas) == value_alone
