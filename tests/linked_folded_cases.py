"""Cases of the coset-grouped row trees (ms_lde_commit_coset, ms_lde_commit_stage_coset, ms_validity_commit_coset), of ms_query_linked_folded (the MSLF blob) and of
the link verifier msh_deep_link_verify_folded (include/ministark.h, include/ministark_host.h - build-defined, no reference counterpart), shared by the emulation suite
(tests/test_linked_folded_emu.py) and the GPU suite (tests/test_linked_folded_gpu.py).  Expected values: tests/pyref_linked_folded.py - the trees over the matrices
ms_lde_read returns (which the plain commits' tests hold to the transforms) and over pyref_deep's chunk matrix; the MSLF blob by its definition; every comparison is exact.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set; `d` is the ms_digest_id."""
import ctypes as C
import struct

import numpy as np

import mini_stark_amd as ms
import deep_cases as dc
import fri_folded_cases as fc
import open_cases as oc
import pyref
import pyref_linked_folded as rlf
import staged_cases as sc
from common import MODULUS, EXT, SplitMix64
from mini_stark_amd import host as mh

SHA = dc.SHA
ro, rd = dc.ro, dc.rd
LATENCY = oc.LATENCY
DIGESTS = (ro.SHA256, ro.BLAKE2S, ro.BLAKE3, ro.KECCAK256, ro.SHA3_256)
ctx_of = oc.ctx_of
_u64p = C.POINTER(C.c_uint64)
TREES = {"lde": ms.TREE_LDE, "stg": ms.TREE_LDE_STAGED, "val": ms.TREE_VALIDITY}


# ---------------------------------------------------------------- statements
def lowdeg_spec(field, N, seed=19, deg=7):
    """x_i = c w^(deg i): the trace polynomial is c X^deg, the constraint x' = w^deg x has degree one and the DEEP polynomial deg coefficients - a round-0 domain
    D_0 = next_pow2(deg * blowup) below L, so that position q of round 0 lies over the LDE row q * L / D_0"""
    p = MODULUS[field]
    c, w = SplitMix64(seed).nonzero(p), pow(pyref.root_of_unity(field, N), deg, p)
    rows = [[c * pow(w, i, p) % p] for i in range(N)]
    return np.array(rows, dtype=np.uint64), [[(1, [(0, 1)]), (p - w, [(0, 0)])]], [[N - 1]], (), [(0, 0, c)]


def statement(field, name, N, seed):
    """(trace rows as an array, the arguments of its staged columns ([] for none), air(finals) -> the program)"""
    if name in sc.CASES:
        rows, main, op, fr = sc.CASES[name](field, N, seed)
        w = len(rows[0])
        args = [(op, fr)]
        return np.array(rows, dtype=np.uint64), args, lambda finals: sc.combined_air(field, N, w, main, args, finals)
    if name == "lowdeg":
        spec = lowdeg_spec(field, N, seed)
    elif name.startswith("cubic"):
        spec = dc.cubic_spec(field, N, seed=seed, w=int(name[5:] or 4))
    else:
        spec = dc.SPECS[name](field, N, seed=seed)
    return spec[0], [], lambda finals: tuple(spec[1:])


def build_state(ctx, d, field, k, name, N=64, blowup=8, seed=1, R=None, stop=None, plain=(), fri_k=None):
    """trace -> ms_lde_commit_coset [-> staged columns -> ms_lde_commit_stage_coset] -> ms_mix_air_ext -> ms_validity_commit_coset -> ms_deep_evals, ms_deep_compose ->
    the folded commit phase at fri_k (default k).  `plain`: the trees committed by the plain call instead; `stop`: "lde", "stage", "validity", "compose" return early"""
    p, e = MODULUS[field], EXT[field]
    trace, args, air_of = statement(field, name, N, 100 + seed)
    w = trace.shape[1]
    rng = SplitMix64(5000 + seed)
    P = dict(field=field, d=d, N=N, blowup=blowup, k=k, name=name, seed=seed, L=N * blowup, trace=trace, c0=w, c1=0, shift=rng.nonzero(p), stg_root=None)
    rc, _ = ctx.trace_commit(trace, w)
    assert rc == 0 and ctx.interpolate() == 0, ctx.last_error()
    rc, P["lde_root"] = ctx.lde_commit(blowup, P["shift"], w) if "lde" in plain else ctx.lde_commit_coset(blowup, P["shift"], k)
    assert rc == 0, ctx.last_error()
    if stop == "lde":
        return P
    finals = []
    for op, fr in args:
        rc, final, _col = ctx.aux_running_staged(op, fr, e, read=True)
        assert rc == 0, ctx.last_error()
        finals.append(final)
    if args:
        P["c1"] = e * len(args)
        rc, P["stg_root"] = ctx.lde_commit_stage(P["c1"]) if "stg" in plain else ctx.lde_commit_stage_coset(k)
        assert rc == 0, ctx.last_error()
    P["c"] = c = w + P["c1"]
    P["air"] = air = air_of(finals)
    if stop == "stage":
        return P
    cons, exempt, periodic, boundary = air
    P["r"] = dc.full_ext(rng, field)
    assert ctx.mix_air_ext(P["r"], cons, exempt, periodic, boundary) == 0, ctx.last_error()
    P["m"] = m = e * dc.vl_of(ctx) // N
    rc, P["val_root"] = ctx.validity_commit(m) if "val" in plain else ctx.validity_commit_coset(k)
    assert rc == 0, ctx.last_error()
    if stop == "validity":
        return P
    P["z"] = dc.full_ext(rng, field)
    rows = ms.air_rows(cons, boundary)
    P["zs"] = dc.shifted_points(field, P["z"], ctx.root_of_unity(N), rows)
    P["lists"] = [list(range(c)) + (list(range(c, c + m)) if t == 0 else []) for t in range(len(rows))]
    rc, ev = ctx.deep_evals(P["zs"], P["lists"])
    assert rc == 0, ctx.last_error()
    P["evals"] = dc.tuples(ev)
    P["gamma"] = dc.full_ext(rng, field)
    if stop == "compose":
        return P
    assert ctx.deep_compose(P["zs"], P["lists"], P["gamma"]) == 0, ctx.last_error()
    P["S"] = fc.commit_phase(ctx, field, blowup, k if fri_k is None else fri_k, R=R, seed=6000 + seed)
    P["D0"] = P["S"]["D0"]
    return P


def plain_validity_matrix(make, P):
    """the (L, m) chunk matrix at sizes where pyref_deep's quadratic chunk_lde takes minutes: every row of the PLAIN validity tree of a second context that went the
    same way (tests/deep_cases.py holds that tree and its openings to pyref_deep at the small sizes)"""
    plain = ctx_of(make, P["d"], P["field"])
    Q = build_state(plain, P["d"], P["field"], P["k"], P["name"], N=P["N"], blowup=P["blowup"], seed=P["seed"], stop="validity", plain=("lde", "stg", "val"))
    L, m = P["L"], P["m"]
    assert Q["m"] == m
    blob = plain.tree_open(ms.TREE_VALIDITY, list(range(L)))
    rows = np.frombuffer(blob, dtype=np.uint8).reshape(L, ro.path_size(1, m, L))
    return np.ascontiguousarray(rows[:, 8:8 + 8 * m]).view(np.uint64).reshape(L, m)


def matrices(ctx, P, make):
    """the (L, c) matrices the three trees are over: the LDE's first c0 columns, its staged columns, the chunk columns of the validity polynomial on the coset"""
    lde = ctx.lde_read()
    out = {"lde": np.ascontiguousarray(lde[:, :P["c0"]])}
    if P["c1"]:
        out["stg"] = np.ascontiguousarray(lde[:, P["c0"]:])
    if "m" in P and P["L"] <= 512:
        cols = rd.chunk_columns(dc.val_rows(ctx), max(1, ctx.validity_ext()), P["N"])
        assert len(cols) == P["m"]
        out["val"] = rd.chunk_lde(P["field"], cols, P["shift"], P["L"])
    elif "m" in P:
        out["val"] = plain_validity_matrix(make, P)
    return out


def group_lists(ngroups, seed=1):
    """every group of a small tree; else the first, the last, a middle one, a list with duplicates in descending order, and random ones"""
    if ngroups <= 256:
        return [list(range(ngroups))]
    rng = np.random.default_rng(seed)
    return oc.index_lists(ngroups) + [[int(x) for x in rng.integers(0, ngroups, 40)]]


def check_tree(ctx, d, field, tree, mat, k, root):
    """root, leaf digests (every sibling digest of every opened path is compared) and ms_tree_open's bytes of one coset tree against pyref_linked_folded"""
    v, lpn, nodes = rlf.coset_tree(d, mat, k)
    ng = len(mat) >> k
    assert bytes(nodes[-1]) == root and len(nodes) == 2 * ng - 1
    for ix in group_lists(ng):
        oc.check_paths(ctx, d, field, ctx.tree_open(tree, ix), v, 1, lpn, nodes, root, ix)
    buf = (C.c_uint8 * 65536)()
    assert oc.raw_open(ctx, tree, 0, [ng], 1, buf, 65536)[0] == ms.ERR_OUT_OF_RANGE and oc.raw_open(ctx, tree, 0, [0, len(mat) - 1], 2, buf, 65536)[0] == ms.ERR_OUT_OF_RANGE
    return v, lpn, nodes


# ---------------------------------------------------------------- 1. + 2. trees and openings
def case_trees(make, d, field, k, name, N=64, blowup=8, extra=0):
    """the three `_coset` commits: roots, leaf digests and openings against the restatement; ms_lde_read and a following plain commit are the plain flow's"""
    p = MODULUS[field]
    ctx, plain = ctx_of(make, d, field, extra), ctx_of(make, d, field, extra)
    P = build_state(ctx, d, field, k, name, N=N, blowup=blowup, stop="validity")
    Q = build_state(plain, d, field, k, name, N=N, blowup=blowup, stop="validity", plain=("lde", "stg", "val"))
    a, L = 1 << k, P["L"]
    M = matrices(ctx, P, make)
    assert np.array_equal(ctx.lde_read(), plain.lde_read()) and ctx.validity_read().tobytes() == plain.validity_read().tobytes()
    if L <= 512:
        assert rlf.coset_values(M["lde"], k).tolist() == rlf.coset_values_slow(M["lde"].tolist(), k)
    for t, root in (("lde", P["lde_root"]), ("stg", P["stg_root"]), ("val", P["val_root"])):
        if t in M:
            assert root != Q[t + "_root"]
            check_tree(ctx, d, field, TREES[t], M[t], k, root)
    betas = np.array([1, 2], dtype=np.uint64)
    ln = C.c_size_t(0)
    assert ctx.L.ms_query_linked(ctx.h, betas.ctypes.data_as(_u64p), C.c_int(2), None, C.c_size_t(0), C.byref(ln)) == ms.ERR_STATE   # no FRI yet; and see case_refusals
    # a plain commit after a coset one: the plain context's roots, and plain openings again
    c = ctx.polys_count()                                 # (a new ms_lde_commit covers the staged columns too)
    got, want = ctx.lde_commit(blowup, P["shift"], c), plain.lde_commit(blowup, P["shift"], c)
    assert got[0] == 0 and got == want and (P["c1"] or got[1] == Q["lde_root"])
    rows = oc.index_lists(L)[3]
    assert ctx.tree_open(ms.TREE_LDE, rows) == plain.tree_open(ms.TREE_LDE, rows)
    return P


def case_trees_lde_only(make, d, field, k, w, N=64, blowup=8):
    """the LDE tree alone over w random columns (no program): the leaf message lengths the instance choice depends on"""
    p = MODULUS[field]
    rng = np.random.default_rng(17 * w + k)
    trace = rng.integers(0, p, (N, w), dtype=np.uint64)
    trace[0, 0] = 0
    trace[1, :] = p - 1                                   # the longest decimals in one row
    ctx, plain = ctx_of(make, d, field), ctx_of(make, d, field)
    for c in (ctx, plain):
        assert c.trace_commit(trace, w)[0] == 0 and c.interpolate() == 0
    shift = SplitMix64(w + 3).nonzero(p)
    rc, root = ctx.lde_commit_coset(blowup, shift, k)
    assert rc == 0, ctx.last_error()
    rc, proot = plain.lde_commit(blowup, shift, w)
    assert rc == 0
    lde = ctx.lde_read()
    assert np.array_equal(lde, plain.lde_read())
    check_tree(ctx, d, field, ms.TREE_LDE, lde, k, root)
    rc, again = ctx.lde_commit(blowup, shift, w)
    assert rc == 0 and again == proot


# ---------------------------------------------------------------- 3. ms_query_linked_folded
def raw_linked(ctx, betas, nq, out, cap, want_len=True):
    b = None if betas is None else np.ascontiguousarray(betas, dtype=np.uint64)
    ln = C.c_size_t(0xDEAD)
    rc = ctx.L.ms_query_linked_folded(ctx.h, None if b is None else b.ctypes.data_as(_u64p), C.c_int(nq), out, C.c_size_t(cap), C.byref(ln) if want_len else None)
    return rc, ln.value


def sections(ctx, P, betas):
    g = rlf.groups(betas, P["D0"], P["L"], P["S"]["k"])
    return (ctx.fri_query_folded(betas), ctx.tree_open(ms.TREE_LDE, g), ctx.tree_open(ms.TREE_LDE_STAGED, g) if P["c1"] else b"", ctx.tree_open(ms.TREE_VALIDITY, g))


def by_definition(ctx, P, betas):
    return rlf.mslf(*sections(ctx, P, betas))


def beta_sets(D0):
    """nq = 1, 2 and 33: a beta equal to D_0, one above 2^63, equal betas, the last position"""
    return [[D0], [D0 - 1, 2**63 + 12345], [(j * 0x9E3779B97F4A7C15) % (1 << 64) for j in range(31)] + [0, 0]]


def case_definition(make, d, field, k, name, N=64, blowup=8, extra=0, R=None):
    ctx = ctx_of(make, d, field, extra)
    P = build_state(ctx, d, field, k, name, N=N, blowup=blowup, R=R)
    D0, L = P["D0"], P["L"]
    assert D0 <= L and L % D0 == 0
    if name == "lowdeg":
        assert D0 == 64 < L                               # s = L / D_0 > 1
    M = matrices(ctx, P, make)
    a = 1 << k
    others = lambda: (ctx.fri_query_folded([3, 2**40]), ctx.tree_open(ms.TREE_LDE, [0, (L >> k) - 1]), ctx.tree_open(ms.TREE_VALIDITY, [1]))   # noqa: E731
    before = others()
    for betas in beta_sets(D0):
        want = by_definition(ctx, P, betas)
        got = ctx.query_linked_folded(betas)
        assert got == want
        sec = rlf.split_mslf(got)
        assert sec is not None and [len(s) for s in sec[1:]] == [len(betas) * ro.path_size(1, a * c, L >> k) if c else 0 for c in (P["c0"], P["c1"], P["m"])]
        assert others() == before
    betas = beta_sets(D0)[1]
    g = rlf.groups(betas, D0, L, k)
    sec = rlf.split_mslf(ctx.query_linked_folded(betas))
    for t, blob, root in (("lde", sec[1], P["lde_root"]), ("stg", sec[2], P["stg_root"]), ("val", sec[3], P["val_root"])):
        if t in M:                                        # ... and against the restatement's trees
            v, lpn, nodes = rlf.coset_tree(d, M[t], k)
            oc.check_paths(ctx, d, field, blob, v, 1, lpn, nodes, root, g)
    blob, prof = oc.profile(ctx, lambda: ctx.query_linked_folded(betas))
    launches = {n: v["launches"] for n, v in prof.items() if isinstance(v, dict) and v.get("launches")}
    assert launches == {"merkle_path": 1}, launches
    assert blob == by_definition(ctx, P, betas)
    size = len(blob)                                      # the size query and the cap rule
    buf = (C.c_uint8 * (size + 8))(*([0xAB] * (size + 8)))
    untouched = bytes(buf)
    nq = len(betas)
    assert raw_linked(ctx, betas, nq, None, 0) == (0, size)
    assert raw_linked(ctx, betas, nq, buf, size - 1) == (ms.ERR_ARG, size)
    assert raw_linked(ctx, None, nq, buf, size)[0] == ms.ERR_ARG
    assert raw_linked(ctx, betas, nq, buf, size, want_len=False)[0] == ms.ERR_ARG
    assert raw_linked(ctx, betas, nq, None, size)[0] == ms.ERR_ARG
    assert raw_linked(ctx, betas, 0, buf, size)[0] == ms.ERR_ARG
    assert raw_linked(ctx, [7] * 4097, 4097, None, 0)[0] == ms.ERR_ARG and raw_linked(ctx, [7] * 4096, 4096, None, 0)[0] == 0
    assert bytes(buf) == untouched
    assert raw_linked(ctx, betas, nq, buf, size + 8) == (0, size) and bytes(buf)[:size] == blob and bytes(buf)[size:] == untouched[size:]
    assert others() == before
    return ctx, P


# ---------------------------------------------------------------- 6. refusals and state
def raw_commit(ctx, which, k, blowup=8, shift=3, root=True):
    r = (C.c_uint8 * 32)() if root else None
    if which == "lde":
        return ctx.L.ms_lde_commit_coset(ctx.h, C.c_size_t(blowup), C.c_uint64(shift), C.c_int(k), r)
    return (ctx.L.ms_lde_commit_stage_coset if which == "stg" else ctx.L.ms_validity_commit_coset)(ctx.h, C.c_int(k), r)


def case_refusals(make, d, field, k=2, name="permutation", N=64, blowup=8):
    """every refusal of the three commits and of ms_query_linked_folded at its site, on ONE context that then gives the bytes of a context never refused"""
    p, e = MODULUS[field], EXT[field]
    fresh = ctx_of(make, d, field)
    W = build_state(fresh, d, field, k, name, N=N, blowup=blowup)
    betas = [5, 2**63 + 9, W["D0"] - 1]
    want = fresh.query_linked_folded(betas)
    ctx = ctx_of(make, d, field)
    assert raw_commit(ctx, "lde", k) == ms.ERR_STATE                                  # before ms_interpolate
    assert raw_linked(ctx, betas, 3, None, 0)[0] == ms.ERR_STATE
    # ---- the three commits
    P = build_state(ctx, d, field, k, name, N=N, blowup=blowup, stop="lde")
    lde = ctx.lde_read().tobytes()
    probe = [0, 1, (P["L"] >> k) - 1]
    opened = ctx.tree_open(ms.TREE_LDE, probe)
    for bad in (0, 4, -1):
        assert raw_commit(ctx, "lde", bad, blowup, P["shift"]) == ms.ERR_ARG and "log_arity" in ctx.last_error()
        assert raw_commit(ctx, "stg", bad) == ms.ERR_ARG and raw_commit(ctx, "val", bad) == ms.ERR_ARG
    assert raw_commit(ctx, "lde", k, blowup, P["shift"], root=False) == ms.ERR_ARG
    assert raw_commit(ctx, "lde", k, 0, P["shift"]) == ms.ERR_ARG and raw_commit(ctx, "lde", k, blowup, 0) == ms.ERR_ARG
    assert raw_commit(ctx, "stg", k) == ms.ERR_STATE                                  # no staged columns
    assert raw_commit(ctx, "val", k) == ms.ERR_STATE                                  # no validity polynomial
    assert ctx.lde_read().tobytes() == lde and ctx.tree_open(ms.TREE_LDE, probe) == opened   # the refused calls changed nothing
    assert fc.raw_begin(ctx, blowup, k) == ms.ERR_STATE
    # a plain LDE tree, or one of another k, under ms_lde_commit_stage_coset
    for other_k in (0, k % 3 + 1):
        c2 = ctx_of(make, d, field)
        build_state(c2, d, field, other_k or k, name, N=N, blowup=blowup, stop="lde", plain=("lde",) if other_k == 0 else ())
        trace, args, _air = statement(field, name, N, 101)
        for op, fr in args:
            assert c2.aux_running_staged(op, fr, e, read=True)[0] == 0
        assert raw_commit(c2, "stg", k) == ms.ERR_STATE and "coset tree" in c2.last_error()
        assert c2.aux_staged_count() == e * len(args)
        rc, r1 = (c2.lde_commit_stage(e * len(args)) if other_k == 0 else c2.lde_commit_stage_coset(other_k))   # ... which the matching call then commits
        assert rc == 0, c2.last_error()
    # L < 2a: N = 2, blowup 2, a = 4 and 8
    small = ctx_of(make, d, field)
    t2 = np.array([[1, 2], [3, 4]], dtype=np.uint64)
    assert small.trace_commit(t2, 2)[0] == 0 and small.interpolate() == 0
    assert raw_commit(small, "lde", 2, 2, 3) == ms.ERR_SHAPE and raw_commit(small, "lde", 3, 2, 3) == ms.ERR_SHAPE
    assert raw_commit(small, "lde", 1, 2, 3) == 0                                      # two leaf groups
    # ---- ms_query_linked_folded
    for plain_tree in ("lde", "stg", "val"):                                           # a plain tree among the three
        c3 = ctx_of(make, d, field)
        if plain_tree == "stg":
            Q = build_state(c3, d, field, k, name, N=N, blowup=blowup, plain=("stg",))  # a plain staged tree on a coset LDE tree is a valid commitment ...
        else:
            Q = build_state(c3, d, field, k, name, N=N, blowup=blowup, plain=(plain_tree,) + (("stg",) if plain_tree == "lde" else ()))
        assert raw_linked(c3, betas, 3, None, 0)[0] == ms.ERR_STATE and "coset tree" in c3.last_error()   # ... that this query phase refuses
        assert len(c3.fri_query_folded(betas)) > 0
    c4 = ctx_of(make, d, field)                                                        # FRI k != tree k
    build_state(c4, d, field, k, name, N=N, blowup=blowup, fri_k=k % 3 + 1)
    assert raw_linked(c4, betas, 3, None, 0)[0] == ms.ERR_STATE and "log_arity" in c4.last_error()
    assert oc.raw_open(c4, ms.TREE_LDE, 0, [0], 1, None, 0)[0] == 0
    c5 = ctx_of(make, d, field)                                                        # ms_query_linked on coset trees under a legacy FRI
    build_state(c5, d, field, k, name, N=N, blowup=blowup, stop="compose")
    Pc = build_state(ctx, d, field, k, name, N=N, blowup=blowup, stop="compose")       # (the refused context goes the same way)
    for c in (c5, ctx):
        assert c.deep_compose(Pc["zs"], Pc["lists"], Pc["gamma"]) == 0
    oc.commit_phase(c5, field, blowup, 3, seed=9)
    ln = C.c_size_t(0)
    b = np.array(betas, dtype=np.uint64)
    assert c5.L.ms_query_linked(c5.h, b.ctypes.data_as(_u64p), C.c_int(3), None, C.c_size_t(0), C.byref(ln)) == ms.ERR_STATE and "one row per leaf group" in c5.last_error()
    assert raw_linked(c5, betas, 3, None, 0)[0] == ms.ERR_STATE                        # ... and the folded call under a legacy FRI
    # the commit phase under way, then finished, on the context refused so often
    assert raw_linked(ctx, betas, 3, None, 0)[0] == ms.ERR_STATE
    assert ctx.fri_begin_folded(blowup, k)[0] == 0
    assert raw_linked(ctx, betas, 3, None, 0)[0] == ms.ERR_STATE and "fri_fold_final" in ctx.last_error()
    S = fc.commit_phase(ctx, field, blowup, k, seed=6001)
    assert S["roots"] == W["S"]["roots"] and S["final"] == W["S"]["final"]
    assert ctx.query_linked_folded(betas) == want
    cons, exempt, periodic, boundary = Pc["air"]
    assert ctx.mix_air_ext(Pc["r"], cons, exempt, periodic, boundary) == 0              # a mix stage kills the validity tree and the FRI state
    assert raw_linked(ctx, betas, 3, None, 0)[0] == ms.ERR_STATE
    # no DEEP polynomial: the validity polynomial itself under the folded FRI
    assert ctx.validity_commit_coset(k)[0] == 0
    fc.commit_phase(ctx, field, blowup, k, seed=6001)
    assert raw_linked(ctx, betas, 3, None, 0)[0] == ms.ERR_STATE and "DEEP" in ctx.last_error()
    assert ctx.L.ms_query_linked_folded(None, None, C.c_int(1), None, C.c_size_t(0), None) == ms.ERR_ARG
    # and once more from the trace on: the clean context's bytes
    P2 = build_state(ctx, d, field, k, name, N=N, blowup=blowup)
    assert (P2["lde_root"], P2["stg_root"], P2["val_root"], P2["S"]["roots"]) == (W["lde_root"], W["stg_root"], W["val_root"], W["S"]["roots"])
    assert ctx.query_linked_folded(betas) == want


def case_virtual_columns(make, d, field=0):
    """an LDE whose linear columns would be virtual (MS_LDE_VIRTUAL=1) is refused, and the plain commit then makes them virtual as ever"""
    ctx = ctx_of(make, d, field, env={"MS_LDE_VIRTUAL": "1"})
    p = MODULUS[field]
    trace = dc.fib_spec(field, 16)[0]
    assert ctx.trace_commit(trace, 2)[0] == 0 and ctx.interpolate() == 0
    assert ctx.polys_lincomb([1, p - 1], [0, 1]) == 0
    assert raw_commit(ctx, "lde", 1, 4, 3) == ms.ERR_STATE and "virtual" in ctx.last_error()
    assert oc.raw_open(ctx, ms.TREE_LDE, 0, [0], 1, None, 0)[0] == ms.ERR_STATE        # nothing was committed
    rc, root = ctx.lde_commit(4, 3, 3)
    assert rc == 0
    other = ctx_of(make, d, field, env={"MS_LDE_VIRTUAL": "0"})                        # written out: the coset commit goes through, over the same matrix
    assert other.trace_commit(trace, 2)[0] == 0 and other.interpolate() == 0 and other.polys_lincomb([1, p - 1], [0, 1]) == 0
    rc, croot = other.lde_commit_coset(4, 3, 1)
    assert rc == 0, other.last_error()
    lde = other.lde_read()
    assert np.array_equal(lde, ctx.lde_read())
    check_tree(other, d, field, ms.TREE_LDE, lde, 1, croot)


def case_sharded(ctx):
    """a context with sharding on (a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses the three commits and the query phase"""
    from mini_stark_amd.dist import LocalShard
    sh = LocalShard(ctx, 4 << 20)
    trace = dc.fib_spec(0, 64)[0]
    assert ctx.trace_commit(trace, 2)[0] == 0 and ctx.interpolate() == 0
    for which in ("lde", "stg", "val"):
        assert raw_commit(ctx, which, 2, 4, 3) == ms.ERR_STATE and "sharding" in ctx.last_error(), which
    assert raw_linked(ctx, [1], 1, None, 0)[0] == ms.ERR_STATE
    assert ctx.lde_commit(4, 3, 2)[0] == 0
    sh.close()


# ---------------------------------------------------------------- 4. the link verifier
def proof_of(make, d, field, k, name, seed=1, betas=(5, 2**40 + 77, 2**63 + 12345), N=64, blowup=8):
    ctx = ctx_of(make, d, field)
    P = build_state(ctx, d, field, k, name, N=N, blowup=blowup, seed=seed)
    P["betas"] = list(betas)
    P["msff"], P["lde_open"], P["stg_open"], P["val_open"] = rlf.split_mslf(ctx.query_linked_folded(P["betas"]))
    return P


def link(P, **over):
    """(the host library's verdict and reason, pyref_linked_folded's step) with any input replaced; the two must agree on the verdict and on the step"""
    a = dict(P, **over)
    rc, why = mh.deep_link_verify_folded(a["d"], a["field"], True, a["N"], a["blowup"], a["shift"], a["k"], a["c0"], a["c1"], a["m"], a["lde_root"], a["stg_root"], a["val_root"],
                                         a["zs"], a["lists"], a["evals"], a["gamma"], a["betas"], a["msff"], a["lde_open"], a["stg_open"], a["val_open"])
    ok, step = rlf.link_verify(a["field"], a["d"], True, a["N"], a["blowup"], a["shift"], a["k"], a["c0"], a["c1"], a["m"], a["lde_root"], a["stg_root"], a["val_root"],
                               a["zs"], a["lists"], a["evals"], a["gamma"], a["betas"], a["msff"], a["lde_open"], a["stg_open"], a["val_open"])
    assert rc in (0, 1) and (rc == 1) == ok and (ok or why.startswith(step)), (rc, why, step)
    return rc, why, step


def link_rejected(P, step, **over):
    rc, why, got = link(P, **over)
    assert rc == 0 and got == step, (why, got, step)


def flip_word(blob, word_at, bit=0):
    """bit `bit` of the little-endian word at byte offset word_at, flipped"""
    at = word_at + bit // 8
    return blob[:at] + bytes([blob[at] ^ (1 << (bit % 8))]) + blob[at + 1:]


def case_link(make, d, field, k, name):
    p, e, a = MODULUS[field], EXT[field], 1 << k
    P = proof_of(make, d, field, k, name)
    S = P["S"]
    nq = len(P["betas"])
    assert link(P) == (1, "", "")
    assert fc.verify_both(d, S, P["betas"], P["msff"]) == (True, "")
    # every limb of every slot of every section, for the first and the last query
    names = {"lde_open": ("LDE opening", P["c0"]), "stg_open": ("staged opening", P["c1"]), "val_open": ("validity opening", P["m"])}
    for key, (step, c) in names.items():
        if not c:
            continue
        blob = P[key]
        psize = len(blob) // nq
        assert psize == ro.path_size(1, a * c, P["L"] >> k)
        for j in (0, nq - 1):
            for i in range(a * c):
                link_rejected(P, step, **{key: flip_word(blob, j * psize + 8 + 8 * i, bit=i % 31)})
            link_rejected(P, step, **{key: flip_word(blob, j * psize)})                              # the leaf_index word
            link_rejected(P, step, **{key: flip_word(blob, j * psize + 16 + 8 * a * c + 7)})         # a path digest
            link_rejected(P, step, **{key: blob[:j * psize + 8] + struct.pack("<Q", p) + blob[j * psize + 16:]})   # a limb that is no field element
        link_rejected(P, step, **{key: blob[:-1]})                                                   # the section's length
        link_rejected(P, step, **{key: blob + bytes(8)})
        link_rejected(P, step, **{key: blob[:-psize]})
    # round 0's slots in the MSFF: each of the a slots, each limb
    nfinal = len(S["final"])
    h0 = (P["D0"] >> k).bit_length() - 1
    p0, ps0 = 56 + nfinal * e * 8, 16 + a * e * 8 + 64 * h0
    for j in (0, nq - 1):
        for i in range(a * e):
            link_rejected(P, "DEEP link", msff=flip_word(P["msff"], p0 + j * ps0 + 8 + 8 * i, bit=i % 31))
        link_rejected(P, "MSFF", msff=flip_word(P["msff"], p0 + j * ps0))                             # its leaf_index word
    for wd in (0, 1, 2, 4, 5):                                                                        # magic, E, k, nq, D_0
        link_rejected(P, "MSFF", msff=flip_word(P["msff"], 8 * wd))
    link_rejected(P, "MSFF", msff=P["msff"][:p0 + nq * ps0 - 1])
    link_rejected(P, "MSFF", msff=P["msff"][:40])
    # a beta, an evaluation, gamma, the shift, a root
    moved = [P["betas"][0] + 1] + P["betas"][1:]
    link_rejected(P, "LDE opening", betas=moved)
    ev = list(P["evals"]); ev[1] = ((ev[1][0] + 1) % p,) + tuple(ev[1][1:])
    link_rejected(P, "DEEP link", evals=ev)
    link_rejected(P, "DEEP link", gamma=((P["gamma"][0] + 1) % p,) + tuple(P["gamma"][1:]))
    link_rejected(P, "DEEP link", shift=P["shift"] % (p - 1) + 1)
    link_rejected(P, "LDE opening", lde_root=bytes(32))
    link_rejected(P, "validity opening", val_root=P["lde_root"])
    if P["c1"]:
        link_rejected(P, "staged opening", stg_root=P["val_root"])
    # malformed arguments are no verdict
    rc, why = mh.deep_link_verify_folded(d, field, True, P["N"], P["blowup"], P["shift"], 4, P["c0"], P["c1"], P["m"], P["lde_root"], P["stg_root"], P["val_root"], P["zs"], P["lists"],
                                         P["evals"], P["gamma"], P["betas"], P["msff"], P["lde_open"], P["stg_open"], P["val_open"])
    assert rc < 0
    rc, why = mh.deep_link_verify_folded(d, field, True, P["N"], P["blowup"], P["shift"], k, P["c0"], P["c1"], P["m"], P["lde_root"], None if P["c1"] else P["lde_root"], P["val_root"],
                                         P["zs"], P["lists"], P["evals"], P["gamma"], P["betas"], P["msff"], P["lde_open"], P["stg_open"], P["val_open"])
    assert rc < 0                                                                                     # stg_root is NULL iff c1 = 0
    return P


def case_splice(make, d, field, k, name="permutation"):
    """proof A's MSFF beside proof B's commitments: a valid folded FRI (msh_fri_folded_verify accepts it under A's roots) that the link refuses"""
    A, B = proof_of(make, d, field, k, name, seed=1), proof_of(make, d, field, k, name, seed=2)
    assert A["D0"] == B["D0"] and A["msff"] != B["msff"] and len(A["msff"]) == len(B["msff"])
    assert link(A)[0] == 1 and link(B)[0] == 1
    assert fc.verify_both(d, A["S"], A["betas"], A["msff"]) == (True, "")
    link_rejected(B, "DEEP link", msff=A["msff"])
    link_rejected(B, "LDE opening", lde_open=A["lde_open"])
    link_rejected(B, "validity opening", val_open=A["val_open"])


# ---------------------------------------------------------------- 8. the fixture of the stand-alone sanitizer program (tests/asan_link_folded)
def apply_edits(base, cut, append, edits):
    out = bytearray(base[:cut] + bytes(append))
    for at, new in edits:
        out[at:at + len(new)] = new
    return bytes(out)


SECTIONS = ("msff", "lde_open", "stg_open", "val_open")


def link_fixture(make, field=0, k=2, N=16):
    """(the proof's dict, [(name, section, cut, append, edits, rc, the beginning of why up to its first colon)]): truncated and tampered copies of the four byte
    sections msh_deep_link_verify_folded reads, as edits of them, with the verdict it gives for each"""
    P = proof_of(make, SHA, field, k, "permutation", N=N)
    e, a = EXT[field], 1 << k
    big = 2**64 - 1
    out = [("whole", 0, len(P["msff"]), 0, [])]
    for s, key in enumerate(SECTIONS):
        blob = P[key]
        n = len(blob)
        width = {0: a * e, 1: a * P["c0"], 2: a * P["c1"], 3: a * P["m"]}[s]
        first = 56 + len(P["S"]["final"]) * e * 8 if s == 0 else 0      # the first path the verifier reads in this section
        psize = (n - first) // len(P["betas"]) if s else 16 + a * e * 8 + 64 * ((P["D0"] >> k).bit_length() - 1)
        out += [("%s cut to %d" % (key, c), s, c, 0, []) for c in sorted({0, 1, 7, 8, 39, 55, 56, first, first + 8, first + 8 + 8 * width, first + 16 + 8 * width, first + psize - 1, first + psize,
                                                                            first + psize + 9, n - 64, n - 1}) if 0 <= c < n]
        out += [("%s trailing" % key, s, n, 8, [])]
        out += [("%s flip %d" % (key, at), s, n, 0, [(at, bytes([blob[at] ^ 0x80]))]) for at in list(range(0, min(n, first + 16 + 8 * width + 70))) + list(range(first + psize, n, 41))]
        nlev = first + 8 + 8 * width
        for v in (big, 65, 64, 63, 0):
            out.append(("%s nlevels=%d" % (key, v), s, n, 0, [(nlev, struct.pack("<Q", v))]))
        if s == 0:
            for wd in (5, 6):                                            # D_0 and nfinal: huge, a non-power, a larger power, zero
                for v in (big, 2**63, 3, P["D0"] * 2, P["L"] * 2, 0):
                    out.append(("msff word %d=%d" % (wd, v), s, n, 0, [(8 * wd, struct.pack("<Q", v))]))
    cases = []
    for name, s, cut, append, edits in out:
        over = {SECTIONS[s]: apply_edits(P[SECTIONS[s]], cut, append, edits)}
        rc, why, _step = link(P, **over)
        cases.append((name, s, cut, append, edits, rc, why.split(":")[0]))
    return P, cases


def link_fixture_bytes(make):
    """tests/golden/link_folded_tampered.bin (layout: tests/golden/gen_link_folded_tampered.py)"""
    P, cases = link_fixture(make)
    e = EXT[P["field"]]
    blob = lambda b: struct.pack("<I", len(b)) + b   # noqa: E731
    u64s = lambda rows: b"".join(struct.pack("<%dQ" % len(r), *r) for r in rows)   # noqa: E731
    begin, poly = [0], []
    for lst in P["lists"]:
        poly += lst
        begin.append(len(poly))
    out = b"MSKF" + struct.pack("<12I", 1, P["field"], P["d"], P["N"], P["blowup"], P["k"], P["c0"], P["c1"], P["m"], len(P["lists"]), len(poly), len(P["betas"]))
    out += struct.pack("<Q", P["shift"]) + struct.pack("<%dI" % len(begin), *begin) + struct.pack("<%dI" % len(poly), *poly)
    out += u64s(P["zs"]) + u64s(P["evals"]) + u64s([P["gamma"]]) + u64s([P["betas"]]) + P["lde_root"] + P["stg_root"] + P["val_root"]
    for key in SECTIONS:
        out += blob(P[key])
    out += struct.pack("<I", len(cases))
    for name, s, cut, append, edits, rc, step in cases:
        out += blob(name.encode()) + struct.pack("<4I", s, cut, append, len(edits)) + b"".join(struct.pack("<I", at) + blob(new) for at, new in edits)
        out += struct.pack("<i", rc) + blob(step.encode())
    return out, cases


# ================================================================ 5. MSLP v3 and the drivers (include/ministark_host.h)
import linked_cases as lc   # noqa: E402
from mini_stark_amd.stark import Stark   # noqa: E402

HEAD3 = struct.calcsize("<4s12I5Q")
PREFIXES = ("header: ", "transcript: ", "proof of work: ", "AIR identity: ", "FRI: ", "LDE opening: ", "staged opening: ", "validity opening: ", "DEEP link: ", "MSFF")


def statement3(field, which, N, seed, spoil=False):
    """(trace, air over the w trace columns, args, nch): `which` None - the fib program without running columns; else staged_cases' statement with one argument"""
    if which is None:
        trace, cons, exempt, periodic, boundary = lc.spec_of("fib", field, N, 100 + seed)
        if spoil:
            trace = trace.copy(); trace[3, 1] = (int(trace[3, 1]) + 1) % MODULUS[field]
        return trace, (cons, exempt, periodic, boundary), [], 0
    return sc.statement(field, which, N, 3000 + seed, spoil=spoil)


def prove3(make, d, field, which, k, N=16, gb=0, seed=1, folds=0, ctx=None):
    ctx = ctx or ctx_of(make, d, field)
    trace, air, args, nch = statement3(field, which, N, seed)
    w = trace.shape[1]
    hs, cfg = lc.handle(ctx, N, w, gb)
    rc = hs.prove_linked_folded(trace, air, k, args, nch, folds)
    assert rc == 0, (rc, ctx.last_error())
    return dict(ctx=ctx, hs=hs, cfg=cfg, d=d, field=field, N=N, w=w, k=k, gb=gb, folds=folds, air=air, args=args, nch=nch, trace=trace, data=hs.linked_proof())


def verdict3(P, data=None, **over):
    a = dict(P, **over)
    rc, why = a["hs"].verify_linked_folded(P["data"] if data is None else data, a["air"], a["N"], a["w"], a["k"], a["args"], a["nch"], a["folds"])
    assert rc in (0, 1) and (why == "" if rc == 1 else why.startswith(PREFIXES)), (rc, why)
    return rc, why


def rejected3(P, data=None, steps=None, **over):
    rc, why = verdict3(P, data, **over)
    assert rc == 0 and (steps is None or why.startswith(steps)), (why, steps)
    return why.split(":")[0]


def case_v3_end_to_end(make, d, field, which, k, gb=0, N=16):
    e = EXT[field]
    P = prove3(make, d, field, which, k, N=N, gb=gb)
    data, w, args, nch = P["data"], P["w"], P["args"], P["nch"]
    assert verdict3(P) == (1, "")
    st = Stark(P["cfg"])
    aux = (args, nch) if args else None
    lp = st.prove_air(P["trace"], P["air"], aux=aux, log_arity=k)                  # the Python driver writes the same bytes
    assert lp.to_bytes() == data
    hd = struct.unpack_from("<4s12I5Q", data, 0)
    R = (N.bit_length() - 1) // k
    assert hd[:6] == (b"MSLP", 3, e, k, w, e * len(args)) and hd[8:13] == (R, P["hs"].fri_queries, gb, len(args), nch) and hd[13:15] == (N, lc.BLOWUP)
    D0, la, lq = hd[15:]
    assert HEAD3 + la + lq == len(data) and D0 <= N * lc.BLOWUP
    sec = rlf.split_mslf(data[HEAD3 + la:])
    assert sec is not None and bool(sec[2]) == bool(args) and struct.unpack_from("<Q", sec[0], 40)[0] == D0
    assert st.verify_air(data, P["air"], N, w, aux=aux, log_arity=k) is True and st.verify_air(lp, P["air"], N, w, aux=aux, log_arity=k) is True
    assert st.verify_air(data[:-1], P["air"], N, w, aux=aux, log_arity=k) is False and st.last_verify_error.startswith("header: ")
    assert P["hs"].prove_linked_folded(P["trace"], P["air"], k, args, nch) == 0 and P["hs"].linked_proof() == data     # a second proof on the same handle: the same bytes
    if R > 1:                                                                        # fewer folds than the most: a longer final polynomial
        Q = prove3(make, d, field, which, k, N=N, gb=gb, folds=1, ctx=P["ctx"])
        assert verdict3(Q) == (1, "") and Q["data"] != data
        assert st.prove_air(P["trace"], P["air"], aux=aux, log_arity=k, fri_folds=1).to_bytes() == Q["data"]
        rejected3(P, Q["data"], steps=("header: ",))                                 # ... which a verifier of the other schedule refuses
    return P


def case_v3_rejections(make, d, field, which, k, gb=4, N=16):
    p, e = MODULUS[field], EXT[field]
    P = prove3(make, d, field, which, k, N=N, gb=gb)
    data, w, args, nch = P["data"], P["w"], P["args"], P["nch"]
    assert verdict3(P) == (1, "")
    flip, put_u64 = lc.flip, lc.put_u64
    hd = struct.unpack_from("<4s12I5Q", data, 0)
    c1, m, npts, R, nq = hd[5], hd[6], hd[7], hd[8], hd[9]
    D0, la, lq = hd[15:]
    a0, q0 = HEAD3, HEAD3 + la
    for j in range(13):                                                              # every header field
        rejected3(P, flip(data, 4 * j), steps=("header: ",))
    for j in range(5):
        rejected3(P, flip(data, 52 + 8 * j), steps=("header: ",))
    rejected3(P, put_u64(data, 52 + 16, D0 * 2), steps=("header: ",))                # another power of two as D_0
    rejected3(P, put_u64(data, 52 + 16, D0 // 2), steps=("header: ",))
    # every arthur region
    nroots = 3 + (1 if args else 0)
    ne = npts * (w + c1) + m
    ev0 = a0 + 32 * nroots
    rr0 = ev0 + ne * e * 8
    fin0 = rr0 + 32 * R
    nfinal = (D0 >> (k * R)) // lc.BLOWUP
    assert fin0 + nfinal * e * 8 + (8 if gb else 0) == q0
    regions = {"trace root": a0 + 3, "LDE root": a0 + 32 + 3, "validity root": a0 + 32 * (nroots - 1) + 3, "first evaluation": ev0, "a chunk's evaluation": ev0 + (w + c1) * e * 8,
               "last evaluation": rr0 - 8, "round 0's root": rr0 + 1, "last round's root": fin0 - 1}
    if gb:
        regions["the nonce"] = q0 - 8
    if args:
        regions["staged root"] = a0 + 64 + 3
    seen = {rejected3(P, flip(data, at)) for at in regions.values()}
    assert seen <= {"proof of work", "AIR identity", "FRI", "LDE opening", "staged opening", "validity opening", "DEEP link"} and (gb or len(seen) >= 2), seen   # (with grinding the seed moves first)
    rejected3(P, put_u64(data, ev0, p), steps=("transcript: ",))                     # a limb that is no field element
    rejected3(P, put_u64(data, fin0, p), steps=("transcript: ",))
    # the final polynomial changed in only one of its two places
    l_msff, l_lde, l_stg, l_val = struct.unpack_from("<4Q", data, q0 + 8)
    s_msff = q0 + 40
    assert data[fin0:fin0 + nfinal * e * 8] == data[s_msff + 56:s_msff + 56 + nfinal * e * 8]
    rejected3(P, flip(data, fin0), steps=("transcript: ",))
    rejected3(P, flip(data, s_msff + 56), steps=("transcript: ",))
    rejected3(P, flip(flip(data, fin0), s_msff + 56))                                 # in both: the transcript moves on, something later fails
    # the sections
    s_lde = s_msff + l_msff
    s_stg, s_val = s_lde + l_lde, s_lde + l_lde + l_stg
    assert s_val + l_val == len(data)
    rejected3(P, flip(data, s_msff + 56 + nfinal * e * 8 + 8), steps=("FRI: ", "DEEP link: "))      # a slot of round 0's coset
    rejected3(P, flip(data, s_msff + l_msff - 1), steps=("FRI: ",))
    rejected3(P, flip(data, s_lde + 8), steps=("LDE opening: ",))
    rejected3(P, flip(data, s_val + 8), steps=("validity opening: ",))
    rejected3(P, flip(data, len(data) - 1), steps=("validity opening: ",))
    if args:
        rejected3(P, flip(data, s_stg + 8), steps=("staged opening: ",))
    for j in range(5):                                                               # the MSLF magic and every length word
        rejected3(P, flip(data, q0 + 8 * j), steps=("header: ",))
    rejected3(P, put_u64(put_u64(data, q0 + 16, l_lde + 8), q0 + 32, l_val - 8))     # the sum fits: the sections are cut elsewhere
    # every truncation length, trailing bytes
    for cut in range(len(data)):
        rejected3(P, data[:cut], steps=("header: ",))
    rejected3(P, data + bytes(8), steps=("header: ",))
    rejected3(P, data + b"\0", steps=("header: ",))
    # another proof's MSLF
    B = prove3(make, d, field, which, k, N=N, gb=gb, seed=2)
    assert len(B["data"]) == len(data) and verdict3(B) == (1, "")
    rejected3(B, B["data"][:q0] + data[q0:])
    # statement binding
    cons, exempt, periodic, boundary = P["air"]
    bnd2 = list(boundary); bnd2[0] = (bnd2[0][0], bnd2[0][1], (bnd2[0][2] + 1) % p)
    rejected3(P, air=(cons, exempt, periodic, bnd2), steps=("proof of work: ", "AIR identity: "))
    rejected3(P, k=k % 3 + 1, steps=("header: ",))
    rejected3(P, N=2 * N, steps=("header: ",))
    # the versions and their verifiers, both ways
    rc, why = P["hs"].verify_linked(data, P["air"], N, w, 3)
    assert rc == 0 and why.startswith("header: ")
    if args:
        rc, why = P["hs"].verify_linked_aux(data, P["air"], args, nch, N, w, 3)
        assert rc == 0 and why.startswith("header: ")
        assert P["hs"].prove_linked_aux(P["trace"], P["air"], args, nch, 3) == 0
    else:
        assert P["hs"].prove_linked(P["trace"], P["air"], 3) == 0
    rejected3(P, P["hs"].linked_proof(), steps=("header: ",))


def case_v3_false_trace(make, d, field, which, k, N=16):
    """a trace that violates the program (or an argument that does not hold): MS_ERR_SHAPE, an empty slot; the same handle then gives a clean run's bytes"""
    want = prove3(make, d, field, which, k, N=N)["data"]
    ctx = ctx_of(make, d, field)
    trace, air, args, nch = statement3(field, which, N, 1)
    bad = statement3(field, which, N, 1, spoil=True)[0]
    hs, cfg = lc.handle(ctx, N, trace.shape[1])
    assert hs.prove_linked_folded(bad, air, k, args, nch) == ms.ERR_SHAPE and hs.linked_proof() == b""
    assert hs.prove_linked_folded(trace, air, 0, args, nch) == ms.ERR_ARG and hs.prove_linked_folded(trace, air, 4, args, nch) == ms.ERR_ARG
    assert hs.prove_linked_folded(trace, air, k, args, nch, 9) == ms.ERR_SHAPE and hs.linked_proof() == b""     # more folds than the DEEP polynomial's domain holds
    assert hs.prove_linked_folded(trace, air, k, args, nch) == 0 and hs.linked_proof() == want
    assert hs.prove_linked_folded(bad, air, k, args, nch) == ms.ERR_SHAPE and hs.linked_proof() == b""
    with np.testing.assert_raises(ms.MsError):
        Stark(cfg).prove_air(bad, air, aux=(args, nch) if args else None, log_arity=k)
    assert Stark(cfg).prove_air(trace, air, aux=(args, nch) if args else None, log_arity=k).to_bytes() == want


# ---------------------------------------------------------------- 8. the fixture of the stand-alone sanitizer program of the v3 verifier (tests/asan_linked_v3)
def v3_edits(P):
    """[(name, cut, append, edits)]: the truncated and tampered copies of the v3 proof P["data"], as edits of it (apply_edits)"""
    data, e, k = P["data"], EXT[P["field"]], P["k"]
    n = len(data)
    hd = struct.unpack_from("<4s12I5Q", data, 0)
    la = hd[16]
    q0 = HEAD3 + la
    l_msff, l_lde, l_stg, l_val = struct.unpack_from("<4Q", data, q0 + 8)
    s_msff = q0 + 40
    s_lde = s_msff + l_msff
    s_stg, s_val = s_lde + l_lde, s_lde + l_lde + l_stg
    out = [("whole", n, 0, [])]
    out += [("cut to %d" % c, c, 0, []) for c in sorted({0, 1, 51, 52, HEAD3 - 1, HEAD3, HEAD3 + 40, q0 - 9, q0 - 1, q0, q0 + 39, q0 + 40, s_msff + 55, s_msff + 56, s_msff + 100, s_lde - 8, s_lde,
                                                         s_lde + 24, s_stg, s_stg + 16, s_val, s_val + 16, n - 64, n - 1})]
    out += [("trailing", n, 8, [])]
    out += [("flip %d" % at, n, 0, [(at, bytes([data[at] ^ 0x80]))]) for at in list(range(0, HEAD3)) + list(range(q0, s_msff + 56 + 24)) + list(range(s_lde, s_lde + 40)) +
            list(range(s_stg, s_stg + 40)) + list(range(s_val, s_val + 40)) + list(range(HEAD3, q0, 29))]
    big = 2**64 - 1
    for at in (52 + 16, 52 + 24, 52 + 32, q0 + 8, q0 + 16, q0 + 24, q0 + 32, s_msff + 40, s_msff + 48):      # D_0 and the length words: huge, and off by 8 either way
        v0 = struct.unpack_from("<Q", data, at)[0]
        for v in (big, big - 7, 2**63, v0 + 8, v0 - 8, v0 * 2, 0):
            out.append(("u64@%d=%d" % (at, v), n, 0, [(at, struct.pack("<Q", v % 2**64))]))
    a = 1 << k
    nfinal = struct.unpack_from("<Q", data, s_msff + 48)[0]
    for at in (s_msff + 56 + nfinal * e * 8 + 8 + a * e * 8, s_lde + 8 + a * P["w"] * 8, s_stg + 8 + a * e * 8):   # nlevels words of the first path of three sections
        for v in (big, 65, 64, 63, 0):
            out.append(("nlevels@%d=%d" % (at, v), n, 0, [(at, struct.pack("<Q", v))]))
    return out


def v3_fixture(make, field=0, k=2, N=16, gb=4):
    """(the proof's dict, [(name, cut, append, edits, rc, the beginning of why up to its first colon)]): truncated and tampered copies of one v3 proof with one
    permutation argument, as edits of it, with the verdict msh_stark_verify_linked_folded gives for each"""
    P = prove3(make, SHA, field, "permutation", k, N=N, gb=gb)
    cases = []
    for name, cut, append, edits in v3_edits(P):
        rc, why = P["hs"].verify_linked_folded(apply_edits(P["data"], cut, append, edits), P["air"], N, P["w"], k, P["args"], P["nch"])
        cases.append((name, cut, append, edits, rc, why.split(":")[0]))
    return P, cases


def v3_fixture_bytes(make):
    """tests/golden/linked_v3_tampered.bin (layout: tests/golden/gen_linked_v3_tampered.py)"""
    P, cases = v3_fixture(make)
    blob = lambda b: struct.pack("<I", len(b)) + b   # noqa: E731
    out = b"MSL3" + struct.pack("<13I", 1, P["field"], P["d"], lc.SECURITY_BITS, lc.BLOWUP, P["N"] - 1, P["w"], P["gb"], P["N"], P["k"], P["folds"], len(P["args"]), P["nch"])
    out += blob(mh.air_encode(P["air"])) + blob(mh.aux_encode(P["field"], P["args"], P["nch"])) + blob(P["data"]) + struct.pack("<I", len(cases))
    for name, cut, append, edits, rc, step in cases:
        out += blob(name.encode()) + struct.pack("<3I", cut, append, len(edits)) + b"".join(struct.pack("<I", at) + blob(new) for at, new in edits)
        out += struct.pack("<i", rc) + blob(step.encode())
    return out, cases


# ---------------------------------------------------------------- 9. the verdicts of the three linked verifiers on tampered proofs (tests/golden/linked_verdicts.json)
def v2_edits(P):
    """([(name, cut, append, edits)], the cuts of the truncation sweep) of the v2 proof P["data"]: every header word flipped, one flipped byte at the start of each
    arthur region and of each MSLS section; every truncation length"""
    data, e = P["data"], EXT[P["field"]]
    n = len(data)
    hd = struct.unpack_from("<4s11I4Q", data, 0)
    c0, c1, m, npts, R, gb, la = hd[3], hd[4], hd[5], hd[6], hd[7], hd[9], hd[14]
    a0, q0 = sc.HEAD2, sc.HEAD2 + la
    l_msfi, l_lde, l_stg, l_val = struct.unpack_from("<4Q", data, q0 + 8)
    fri0 = a0 + 128 + (npts * (c0 + c1) + m) * e * 8
    regions = [a0, a0 + 32, a0 + 64, a0 + 96, a0 + 128, fri0]
    for i in range(R - 1):
        regions += [fri0 + 32 + i * (2 * e * 8 + 32), fri0 + 32 + i * (2 * e * 8 + 32) + 2 * e * 8]
    if gb:
        regions.append(q0 - 8)
    assert regions[-1] < q0 and q0 + 40 + l_msfi + l_lde + l_stg + l_val == n
    regions += [q0, q0 + 40, q0 + 40 + l_msfi, q0 + 40 + l_msfi + l_lde, q0 + 40 + l_msfi + l_lde + l_stg]
    out = [("whole", n, 0, []), ("trailing", n, 8, [])]
    out += [("flip %d" % at, n, 0, [(at, bytes([data[at] ^ 0x80]))]) for at in [4 * j for j in range(12)] + [48 + 8 * j for j in range(4)] + regions]
    return out, range(n)


def verdict_cases():
    """(name, version, digest, field, which, k, gb): v1 and v2 at N = 8, R = 3, v3 at N = 16, on both fields at grinding bits 0 and 4 under SHA-256; one v3 case per
    other digest"""
    out = []
    for field in (0, 1):
        for gb in (0, 4):
            out.append(("v1 fib field %d gb %d" % (field, gb), 1, SHA, field, None, 0, gb))
            out.append(("v2 permutation field %d gb %d" % (field, gb), 2, SHA, field, "permutation", 0, gb))
            for k in (1, 2, 3):
                for which in (None, "permutation"):
                    out.append(("v3 %s k %d field %d gb %d" % (which or "fib", k, field, gb), 3, SHA, field, which, k, gb))
    for d in DIGESTS[1:]:
        out.append(("v3 permutation k 2 field 0 gb 4 digest %d" % d, 3, d, 0, "permutation", 2, 4))
    return out


def linked_verdicts(make):
    """tests/golden/linked_verdicts.json as a dict: per case the SHA-256 of the proof's bytes and, for every tampered copy in the order of the edit list, the index of
    its (rc, why) in `table`; v2's truncation sweep as a SHA-256 over its verdicts, one 'rc|why' line per length"""
    import hashlib
    table, index, cases = [], {}, {}

    def idx(rc, why):
        if (rc, why) not in index:
            index[(rc, why)] = len(table)
            table.append([rc, why])
        return index[(rc, why)]

    for name, version, d, field, which, k, gb in verdict_cases():
        sweep = ()
        if version == 1:
            P = lc.prove(make, d, field, "fib", N=8, R=3, gb=gb)
            edits, verify = lc.tampered_edits(P), lambda b: P["hs"].verify_linked(b, P["air"], 8, P["w"], 3)   # noqa: E731
        elif version == 2:
            P = sc.prove2(make, d, field, which, N=8, R=3, gb=gb)
            (edits, sweep), verify = v2_edits(P), lambda b: P["hs"].verify_linked_aux(b, P["air"], P["args"], P["nch"], 8, P["w"], 3)   # noqa: E731
        else:
            P = prove3(make, d, field, which, k, N=16, gb=gb)
            edits, verify = v3_edits(P), lambda b: P["hs"].verify_linked_folded(b, P["air"], 16, P["w"], k, P["args"], P["nch"])   # noqa: E731
        data = P["data"]
        case = dict(sha256=hashlib.sha256(data).hexdigest(), verdicts=[idx(*verify(apply_edits(data, cut, append, ed))) for _n, cut, append, ed in edits])
        if sweep:
            case["truncations"] = hashlib.sha256("".join("%d|%s\n" % verify(data[:cut]) for cut in sweep).encode()).hexdigest()
        cases[name] = case
    return dict(table=table, cases=cases)


def linked_verdicts_text(verdicts):
    """the file's text for the dict of linked_verdicts"""
    import json
    return json.dumps(verdicts, indent=0, separators=(",", ":"), ensure_ascii=True) + "\n"
