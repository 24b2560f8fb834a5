"""Cases of the composition commitment and the DEEP stage (ms_validity_commit, ms_deep_evals, ms_deep_compose, ms_tree_open(MS_TREE_VALIDITY), msh_deep_link_verify,
msh_validity_from_chunks; include/ministark.h - build-defined, no reference counterpart), shared by the emulation suite (tests/test_deep_emu.py) and the GPU suite
(tests/test_deep_gpu.py).  Expected values: tests/pyref_deep.py, a big-integer restatement of the definitions; every comparison is exact.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set; `d` is the ms_digest_id."""
import ctypes as C
import struct

import numpy as np

import mini_stark_amd as ms
import open_cases as oc
import pyref
import pyref_deep as rd
import pyref_open as ro
from common import MODULUS, EXT, SplitMix64
from mini_stark_amd.host import air_expected_validity_ext, deep_link_verify, fri_index_verify, merkle_path_check_index, validity_from_chunks
from parity_cases import rand_field

SHA = ro.SHA256
ctx_of = oc.ctx_of
_u64p = C.POINTER(C.c_uint64)


# ---------------------------------------------------------------- AIR programs: (trace, constraints, exempt, periodic, boundary)
def power_spec(field, N, deg, seed=7):
    """x' = x^deg + 1 on the rows 0 .. N-2, x_0 fixed by a boundary constraint: degree deg, VL = N / 2N / 4N for deg = 2 / 3 / 5"""
    p = MODULUS[field]
    rows = [[SplitMix64(seed + deg).nonzero(p)]]
    for _ in range(N - 1):
        rows.append([(pow(rows[-1][0], deg, p) + 1) % p])
    cons = [[(1, [(0, 1)]), (p - 1, [(0, 0)] * deg), (p - 1, [])]]
    return np.array(rows, dtype=np.uint64), cons, [[N - 1]], (), [(0, 0, rows[0][0])]


def fib_spec(field, N, seed=11):
    """Fibonacci-style: a' = b, b' = a + b"""
    p, rng = MODULUS[field], SplitMix64(seed)
    rows = [[rng.nonzero(p), rng.nonzero(p)]]
    for _ in range(N - 1):
        a, b = rows[-1]
        rows.append([b, (a + b) % p])
    cons = [[(1, [(0, 1)]), (p - 1, [(1, 0)])], [(1, [(1, 1)]), (p - 1, [(0, 0)]), (p - 1, [(1, 0)])]]
    return np.array(rows, dtype=np.uint64), cons, [[N - 1], [N - 1]], (), [(0, 0, rows[0][0]), (1, 0, rows[0][1])]


def cubic_spec(field, N, seed=13, w=4):
    """the cubic spec: col_j' = col_j col_(j+1) col_(j+2) + s_j col_(j+3), column indices mod w"""
    p, rng = MODULUS[field], SplitMix64(seed)
    s = [rng.nonzero(p) for _ in range(w)]
    rows = [[rng.nonzero(p) for _ in range(w)]]
    for _ in range(N - 1):
        r = rows[-1]
        rows.append([(r[j] * r[(j + 1) % w] * r[(j + 2) % w] + s[j] * r[(j + 3) % w]) % p for j in range(w)])
    cons = [[(1, [(j, 1)]), (p - 1, [(j, 0), ((j + 1) % w, 0), ((j + 2) % w, 0)]), (p - s[j], [((j + 3) % w, 0)])] for j in range(w)]
    return np.array(rows, dtype=np.uint64), cons, [[N - 1]] * w, (), [(0, 0, rows[0][0])]


def constant_spec(field, N, seed=17):
    """a' = a on a constant column: every polynomial is a constant and the DEEP polynomial is zero - the smallest round-0 domain (D_0 = blowup < L)"""
    p = MODULUS[field]
    k = SplitMix64(seed).nonzero(p)
    return np.array([[k]] * N, dtype=np.uint64), [[(1, [(0, 1)]), (p - 1, [(0, 0)])]], [[N - 1]], (), [(0, 0, k)]


SPECS = {"fib": fib_spec, "cubic": cubic_spec, "constant": constant_spec}


def commit(ctx, trace, blowup, shift):
    N, w = trace.shape
    rc, troot = ctx.trace_commit(trace, w)
    assert rc == 0, ctx.last_error()
    assert ctx.interpolate() == 0
    rc, root = ctx.lde_commit(blowup, shift, w)
    assert rc == 0, ctx.last_error()
    return root


def full_ext(rng, field):
    return tuple(rng.nonzero(MODULUS[field]) for _ in range(EXT[field]))


def vl_of(ctx):
    ctx.L.ms_validity_len.restype = C.c_size_t
    return int(ctx.L.ms_validity_len(ctx.h))


def val_rows(ctx):
    v = ctx.validity_read()
    return [int(x) for x in v] if v.ndim == 1 else [tuple(int(x) for x in row) for row in v]


def coefficient_columns(ctx, c, N):
    """F_0 .. F_(c+m-1) as lists of N integers, read back through ms_poly_read and ms_validity_read"""
    F = [[int(v) for v in ctx.poly_read(j)] for j in range(c)]
    return F + rd.chunk_columns(val_rows(ctx), max(1, ctx.validity_ext()), N)


def shifted_points(field, z, omega, rows):
    T, p = rd.tower(field), MODULUS[field]
    return [T.mul(tuple(z), T.from_base(pow(omega, k, p))) for k in rows]


def tuples(a):
    return [tuple(int(x) for x in row) for row in a]


# ---------------------------------------------------------------- 1. chunks and tree
def case_chunks_tree(make, d, field, ext, deg, N, blowup=8):
    p, e = MODULUS[field], EXT[field]
    trace, cons, exempt, periodic, boundary = power_spec(field, N, deg)
    rng = SplitMix64(40 + deg + N)
    shift = rng.nonzero(p)
    r = full_ext(rng, field) if ext else rng.nonzero(p)
    ctxs = [ctx_of(make, d, field), ctx_of(make, d, field)]   # [0] commits the validity polynomial, [1] does not
    for ctx in ctxs:
        commit(ctx, trace, blowup, shift)
        assert (ctx.mix_air_ext(r, cons, exempt, periodic, boundary) if ext else ctx.mix_air(r, cons, exempt, periodic, boundary)) == 0, ctx.last_error()
    ctx, plain = ctxs
    L, ve, VL = N * blowup, (e if ext else 1), vl_of(ctx)
    assert VL == N * {2: 1, 3: 2, 5: 4}[deg] and ctx.validity_ext() == ve
    m = ve * VL // N
    before = ctx.validity_read().tobytes()
    assert ctx.validity_commit(m + 1)[0] == ms.ERR_ARG and ctx.validity_commit(0)[0] == ms.ERR_ARG
    assert oc.raw_open(ctx, ms.TREE_VALIDITY, 0, [0], 1, None, 0)[0] == ms.ERR_STATE
    rc, root = ctx.validity_commit(m)
    assert rc == 0, ctx.last_error()
    cols = rd.chunk_columns(val_rows(ctx), ve, N)
    assert len(cols) == m
    mat = rd.chunk_lde(field, cols, shift, L)
    nodes = ro.tree_nodes(d, mat.reshape(-1, 1), 1, m)
    assert bytes(nodes[-1]) == root
    for ix in oc.index_lists(L):
        oc.check_paths(ctx, d, field, ctx.tree_open(ms.TREE_VALIDITY, ix), mat.reshape(-1, 1), 1, m, nodes, root, ix)
    # V(z) from the chunk evaluations is the validity value of ms_eval_ext
    z = full_ext(rng, field)
    rc, ev = ctx.deep_evals([z], [list(range(1, 1 + m))])
    assert rc == 0, ctx.last_error()
    assert tuples(ev) == rd.deep_evals(field, [None] + cols, [z], [list(range(1, 1 + m))])
    rc, allv = ctx.eval_ext(np.array(z, dtype=np.uint64))
    assert rc == 0
    rc, vz = validity_from_chunks(field, ve, N, z, ev)
    assert rc == 0 and tuple(int(x) for x in vz) == tuple(int(x) for x in allv[0][1]) == rd.validity_from_chunks(field, ve, N, z, tuples(ev))
    # the polynomial and a following plain ms_fri_begin are what they are without the call
    assert ctx.validity_read().tobytes() == before == plain.validity_read().tobytes()
    rounds = 3
    a, b = ctx.fri_begin(blowup, rounds), plain.fri_begin(blowup, rounds)
    assert a[0] == 0 and a == b and ctx.fri_round_info(0) == plain.fri_round_info(0)
    assert ctx.deep_len() == 0


# ---------------------------------------------------------------- 2. evaluations
def case_evals(make, field, c, d=SHA):
    p, e = MODULUS[field], EXT[field]
    ctx = ctx_of(make, d, field)
    N = 16
    _root, L, _ = oc.build_lde(ctx, field, c, N=N)       # c = 3 and 65 hold polynomials ms_polys_lincomb defined lazily
    rng = SplitMix64(900 + c)
    assert ctx.mix(rng.field(p)) == 0
    assert ctx.validity_commit(1)[0] == 0, ctx.last_error()
    omega = ctx.root_of_unity(N)
    z = full_ext(rng, field)
    pts = shifted_points(field, z, omega, [0, 1, N - 1])
    every = list(range(c + 1))
    cases = [([pts[0]], [every]),                                            # full
             (pts[:2], [every[::2], [c] + every[1::2]]),                     # partial, with the chunk column at the second point
             (pts, [every[:c // 3 + 1], every[c // 3 + 1:2 * c // 3 + 1] or [0], every[2 * c // 3 + 1:]])]   # disjoint
    got = []
    for zs, lists in cases:                                                  # (before any ms_poly_read: the lazily defined polynomials are written out by the call itself)
        rc, ev = ctx.deep_evals(zs, lists)
        assert rc == 0, ctx.last_error()
        got.append(tuples(ev))
    F = coefficient_columns(ctx, c, N)
    for (zs, lists), g in zip(cases, got):
        assert g == rd.deep_evals(field, F, zs, lists)
    rc, allv = ctx.eval_ext(np.array(pts[0], dtype=np.uint64))
    assert rc == 0 and got[0] == tuples(allv[0])                             # ms_eval_ext's row at z, polynomial for polynomial
    rc, vz = validity_from_chunks(field, 1, N, pts[0], [got[0][c]])
    assert rc == 0 and tuple(int(x) for x in vz) == got[0][c]


# ---------------------------------------------------------------- 3. the polynomial
def point_lists(c, npts):
    """every point names column 0 and the chunk column c; point t also names the columns j = t (mod npts): columns shared by all points, by one, and (c < npts) points with two entries only"""
    return [sorted({0, c} | set(range(t, c, npts))) for t in range(npts)]


def case_poly(make, field, N, c, npts, gamma="full", zkind="full", d=SHA, blowup=2):
    p, e = MODULUS[field], EXT[field]
    ctx = ctx_of(make, d, field)
    rng = SplitMix64(7000 + N + c + npts)
    trace = rand_field(field, (N, c), seed=N + c)
    shift = rng.nonzero(p)
    commit(ctx, trace, blowup, shift)
    assert ctx.mix(rng.nonzero(p)) == 0
    assert ctx.validity_commit(1)[0] == 0, ctx.last_error()
    L = N * blowup
    T = rd.tower(field)
    z = full_ext(rng, field) if zkind == "full" else (rng.nonzero(p),) + (0,) * (e - 1)
    while T.pow(z, L) == T.from_base(pow(shift, L, p)):                       # (a base-field z may lie in the coset)
        z = (rng.nonzero(p),) + z[1:]
    g = {"full": full_ext(rng, field), "zero": (0,) * e, "one": (1,) + (0,) * (e - 1), "base": (rng.nonzero(p),) + (0,) * (e - 1)}[gamma]
    zs = shifted_points(field, z, ctx.root_of_unity(N), range(npts))
    lists = point_lists(c, npts)
    assert ctx.deep_len() == 0
    assert ctx.deep_compose(zs, lists, g) == 0, ctx.last_error()
    assert ctx.deep_len() == N
    rc, _root0 = ctx.fri_begin(blowup, 2)
    assert rc == 0, ctx.last_error()
    nc, D0 = ctx.fri_round_info(0)
    got = tuples(ctx.fri_round_poly(0))
    want = rd.deep_poly(field, coefficient_columns(ctx, c, N), zs, lists, g, shift, N)
    trimmed = max((k + 1 for k, v in enumerate(want) if any(v)), default=0)
    assert nc == trimmed <= N - 1 and got == want[:nc]
    assert L % D0 == 0 and D0 == max(blowup, pyref.next_pow2(nc * blowup))
    # a second compose replaces the polynomial
    assert ctx.deep_compose(zs[:1], [[0]], g) == 0
    assert ctx.fri_begin(blowup, 2)[0] == 0
    F0 = [int(v) for v in ctx.poly_read(0)]
    assert tuples(ctx.fri_round_poly(0)) == rd.deep_poly(field, [F0], zs[:1], [[0]], g, shift, N)[:ctx.fri_round_info(0)[0]]


# ---------------------------------------------------------------- 4. end to end
def build_proof(ctx, d, field, name, N=64, blowup=8, R=3, seed=1, betas=(5, 2**40 + 77, 2**63 + 12345)):
    """trace -> LDE -> ms_mix_air_ext -> ms_validity_commit -> ms_deep_evals -> ms_deep_compose -> FRI commit phase -> ms_fri_query_index -> openings of both trees"""
    p, e = MODULUS[field], EXT[field]
    trace, cons, exempt, periodic, boundary = SPECS[name](field, N, seed=100 + seed)
    c = trace.shape[1]
    rng = SplitMix64(5000 + seed)
    P = dict(field=field, d=d, N=N, blowup=blowup, c=c, L=N * blowup, air=(cons, exempt, periodic, boundary))
    P["shift"] = rng.nonzero(p)
    P["lde_root"] = commit(ctx, trace, blowup, P["shift"])
    P["r"] = full_ext(rng, field)
    assert ctx.mix_air_ext(P["r"], cons, exempt, periodic, boundary) == 0, ctx.last_error()
    P["m"] = m = e * vl_of(ctx) // N
    rc, P["val_root"] = ctx.validity_commit(m)
    assert rc == 0, ctx.last_error()
    P["z"] = z = full_ext(rng, field)
    P["rows"] = rows = ms.air_rows(cons, boundary)
    P["zs"] = shifted_points(field, z, ctx.root_of_unity(N), rows)
    P["lists"] = [list(range(c)) + (list(range(c, c + m)) if k == 0 else []) for k in range(len(rows))]   # the chunks are opened at z itself
    rc, ev = ctx.deep_evals(P["zs"], P["lists"])
    assert rc == 0, ctx.last_error()
    P["evals"] = tuples(ev)
    P["gamma"] = full_ext(rng, field)
    assert ctx.deep_compose(P["zs"], P["lists"], P["gamma"]) == 0, ctx.last_error()
    P["S"] = oc.commit_phase(ctx, field, blowup, R, seed=6000 + seed)
    P["betas"] = list(betas)
    P["msfi"] = ctx.fri_query_index(P["betas"])
    P["open_rows"] = rd.link_rows(P["betas"], P["S"]["D0"], P["L"])
    P["lde_open"] = ctx.tree_open(ms.TREE_LDE, P["open_rows"])
    P["val_open"] = ctx.tree_open(ms.TREE_VALIDITY, P["open_rows"])
    return P


def link(P, **over):
    """(the host library's verdict and reason, pyref_deep's verdict and step) with any input replaced"""
    a = dict(P, **over)
    rc, why = deep_link_verify(a["d"], a["field"], True, a["N"], a["blowup"], a["shift"], a["c"], a["m"], a["lde_root"], a["val_root"], a["zs"], a["lists"], a["evals"],
                               a["gamma"], a["betas"], a["msfi"], a["lde_open"], a["val_open"])
    ok, step = rd.link_verify(a["field"], a["d"], True, a["N"], a["blowup"], a["shift"], a["c"], a["m"], a["lde_root"], a["val_root"], a["zs"], a["lists"], a["evals"],
                              a["gamma"], a["betas"], a["msfi"], a["lde_open"], a["val_open"])
    assert (rc == 1) == ok, (rc, why, step)
    return rc, why, step


def fri_ok(P, msfi=None):
    S = P["S"]
    return fri_index_verify(P["d"], P["field"], True, P["blowup"], S["roots"], S["zs"], S["Bs"], S["alphas"], P["betas"], P["msfi"] if msfi is None else msfi)[0]


def rejected(P, step, prefix, **over):
    rc, why, got = link(P, **over)
    assert rc == 0 and got == step and why.startswith(prefix), (rc, why, got)


def air_identity(P):
    """msh_air_expected_validity_ext from the opened polynomial values equals V(z) from the chunk evaluations"""
    field, c, m, e = P["field"], P["c"], P["m"], EXT[P["field"]]
    ev, pos, opened = P["evals"], 0, []
    for k, lst in enumerate(P["lists"]):
        opened.append(ev[pos:pos + c])
        if k == 0:
            chunks = ev[pos + c:pos + c + m]
        pos += len(lst)
    rc, want = air_expected_validity_ext(field, P["r"], P["air"], P["N"], P["z"], P["rows"], np.array(opened, dtype=np.uint64), npolys=c)
    rc2, vz = validity_from_chunks(field, e, P["N"], P["z"], chunks)
    assert rc == 0 and rc2 == 0 and want.tolist() == vz.tolist() and any(int(x) for x in vz)


def case_end_to_end(make, d, field, name):
    p, e = MODULUS[field], EXT[field]
    P = build_proof(ctx_of(make, d, field), d, field, name)
    c, m, L = P["c"], P["m"], P["L"]
    assert P["S"]["R"] >= 3 and len(P["betas"]) == 3 and P["S"]["D0"] == L
    air_identity(P)
    assert fri_ok(P) == 1
    assert link(P) == (1, "", "")
    # one claimed evaluation changed (the first, the last - a chunk's - and one of the second point)
    for n in (0, c + m - 1, c + m):
        ev = list(P["evals"]); ev[n] = ((ev[n][0] + 1) % p,) + ev[n][1:]
        rejected(P, "link", "DEEP link", evals=ev)
    rejected(P, "link", "DEEP link", gamma=P["gamma"][:-1] + ((P["gamma"][-1] + 1) % p,))
    # one opened element changed (the path then no longer hashes to the root), one path node changed
    lsz, vsz = ro.path_size(1, c, L), ro.path_size(1, m, L)
    for which, blob, size, lpn, step, prefix in (("lde_open", P["lde_open"], lsz, c, "lde", "LDE opening"), ("val_open", P["val_open"], vsz, m, "validity", "validity opening")):
        for path_no in (0, 5):
            at = path_no * size + 8
            v = (struct.unpack_from("<Q", blob, at)[0] + 1) % p
            rejected(P, step, prefix, **{which: blob[:at] + struct.pack("<Q", v) + blob[at + 8:]})
            at = path_no * size + 8 + lpn * 8 + 8 + 40
            rejected(P, step, prefix, **{which: blob[:at] + bytes([blob[at] ^ 1]) + blob[at + 1:]})
        rejected(P, step, prefix, **{which: blob[:-1]})
        rejected(P, step, prefix, **{which: blob[:-size]})
        rejected(P, step, prefix, **{which: blob + b"\0" * 8})
        rejected(P, step, prefix, **{which: blob + blob[:size]})
    rejected(P, "msfi", "MSFI", msfi=P["msfi"][:40])
    rejected(P, "link", "DEEP link", msfi=swap_first_value(P))
    # the roots swapped, another shift, another query
    rejected(P, "lde", "LDE opening", lde_root=P["val_root"])
    rejected(P, "link", "DEEP link", shift=P["shift"] % (p - 1) + 1)
    rejected(P, "lde", "LDE opening", betas=[P["betas"][0] + 1] + P["betas"][1:])


def swap_first_value(P):
    """the MSFI blob with one limb of the first opened value of window 0 changed"""
    e, p = EXT[P["field"]], MODULUS[P["field"]]
    nfinal = struct.unpack_from("<Q", P["msfi"], 40)[0]
    at = 48 + nfinal * e * 8 + 8 + (rd.link_rows(P["betas"], P["S"]["D0"], P["S"]["D0"])[0] & 1) * e * 8
    v = (struct.unpack_from("<Q", P["msfi"], at)[0] + 1) % p
    return P["msfi"][:at] + struct.pack("<Q", v) + P["msfi"][at + 8:]


def case_small_domain(make, d, field):
    """D_0 < L: rows opened at b instead of b (L / D_0) are refused by position"""
    ctx = ctx_of(make, d, field)
    P = build_proof(ctx, d, field, "constant", R=3)
    D0, L = P["S"]["D0"], P["L"]
    assert D0 == P["blowup"] < L and L % D0 == 0
    assert fri_ok(P) == 1 and link(P) == (1, "", "")
    at_b = rd.link_rows(P["betas"], D0, D0)                                  # the FRI positions themselves
    assert at_b != P["open_rows"]
    rejected(P, "lde", "LDE opening", lde_open=ctx.tree_open(ms.TREE_LDE, at_b), val_open=ctx.tree_open(ms.TREE_VALIDITY, at_b))
    rejected(P, "validity", "validity opening", val_open=ctx.tree_open(ms.TREE_VALIDITY, at_b))


# ---------------------------------------------------------------- 5. the splice
def case_splice(make, d, field, name="fib"):
    """proof A's FRI beside proof B's commitments: today's verifiers accept (nothing ties round 0 to the LDE tree); the link verifier does not"""
    A = build_proof(ctx_of(make, d, field), d, field, name, seed=1)
    B = build_proof(ctx_of(make, d, field), d, field, name, seed=2)
    assert A["lde_root"] != B["lde_root"] and A["S"]["D0"] == B["S"]["D0"] and A["open_rows"] == B["open_rows"]
    assert link(A)[0] == 1 and link(B)[0] == 1
    # msh_fri_index_verify is given no LDE root at all: A's MSFI passes whichever LDE root stands beside it
    assert fri_ok(A) == 1
    spliced = dict(B, msfi=A["msfi"])                                        # A's FRI with B's roots, evaluations and openings
    rejected(spliced, "link", "DEEP link")
    rejected(A, "lde", "LDE opening", lde_open=B["lde_open"], val_open=B["val_open"])   # A's roots, B's openings
    rejected(A, "validity", "validity opening", val_open=B["val_open"])


# ---------------------------------------------------------------- 6. refusals and invariance
def raw_deep(ctx, fn, z, lists, extra, npts=None, null_struct=False):
    """ms_deep_evals / ms_deep_compose through the raw ABI: any array may be None (NULL); `extra` the evals buffer / gamma"""
    s, _keep = ms.deep_struct(z, lists, npts=npts)
    x = None if extra is None else np.ascontiguousarray(extra, dtype=np.uint64)
    return getattr(ctx.L, fn)(ctx.h, None if null_struct else C.byref(s), None if x is None else x.ctypes.data_as(_u64p))


def case_refusals(make, field, d=SHA):
    p, e = MODULUS[field], EXT[field]
    N, blowup = 16, 8
    trace, cons, exempt, periodic, boundary = fib_spec(field, N)
    c = 2
    rng = SplitMix64(77)
    shift, r, g = rng.nonzero(p), full_ext(rng, field), full_ext(rng, field)
    z = full_ext(rng, field)
    ctx, fresh = ctx_of(make, d, field), ctx_of(make, d, field)
    root = bytes(32)
    assert ctx.validity_commit(1)[0] == ms.ERR_STATE                          # nothing committed at all
    for k in (ctx, fresh):
        commit(k, trace, blowup, shift)
    assert ctx.validity_commit(1)[0] == ms.ERR_STATE and "mix" in ctx.last_error()   # before a mix stage
    assert raw_deep(ctx, "ms_deep_compose", [z], [[0]], g) == ms.ERR_STATE    # no validity tree
    assert raw_deep(ctx, "ms_deep_evals", [z], [[0]], [0] * e) == ms.ERR_STATE
    for k in (ctx, fresh):
        assert k.mix_air_ext(r, cons, exempt, periodic, boundary) == 0
    m = e * vl_of(ctx) // N
    assert raw_deep(ctx, "ms_deep_compose", [z], [[0]], g) == ms.ERR_STATE    # still none
    assert ctx.L.ms_validity_commit(ctx.h, C.c_size_t(m), None) == ms.ERR_ARG
    assert ctx.validity_commit(m + 1)[0] == ms.ERR_ARG
    for k in (ctx, fresh):
        rc, root = k.validity_commit(m)
        assert rc == 0
    lists, zs = [[0, 1, c], [1]], shifted_points(field, z, ctx.root_of_unity(N), [0, 1])

    def reference(k):
        rc, ev = k.deep_evals(zs, lists)
        assert rc == 0 and k.deep_compose(zs, lists, g) == 0 and k.fri_begin(blowup, 2)[0] == 0
        return tuples(ev), tuples(k.fri_round_poly(0)), k.validity_read().tobytes()
    want = reference(fresh)
    flat = [x for zz in zs for x in zz]
    coset = (shift * pow(pyref.root_of_unity(field, N * blowup), 3, p) % p,) + (0,) * (e - 1)
    bad = [  # (z, lists, gamma / evals, npts override, expected status)
        (None, lists, g, None, ms.ERR_ARG), (flat, (None, [0, 1, c, 1]), g, 2, ms.ERR_ARG), (flat, ([0, 3, 4], None), g, None, ms.ERR_ARG), (flat, lists, None, None, ms.ERR_ARG),
        (flat, lists, g, 0, ms.ERR_ARG), (flat * 5, [[0]] * 9, g, None, ms.ERR_ARG),                           # npts outside 1..8
        (flat, ([1, 3, 4], [0, 1, c, 1]), g, None, ms.ERR_ARG), (flat, ([0, 3, 2], [0, 1, c, 1]), g, None, ms.ERR_ARG),   # pt_begin not from 0, decreasing
        (flat, ([0, 4, 4], [0, 1, c, 1]), g, None, ms.ERR_ARG),                                                # an empty point
        (flat, [[0] * 8000, [1] * 193], g, None, ms.ERR_ARG),                                                  # 8193 entries
        (flat, [[0, c + m], [1]], g, None, ms.ERR_ARG),                                                        # an index at c + m
        (flat[:-1] + [p], lists, g, None, ms.ERR_ARG), (flat, lists, g[:-1] + (p,), None, ms.ERR_ARG),         # a limb at p
        (list(coset) + flat[e:], lists, g, None, ms.ERR_SHAPE), (flat[:e] + list(coset), lists, g, None, ms.ERR_SHAPE)]   # a point in the LDE coset
    for zz, ll, gg, npts, code in bad:
        assert raw_deep(ctx, "ms_deep_compose", zz, ll, gg, npts=npts) == code, (ll if not isinstance(ll, list) or len(ll) < 5 else "...", code, ctx.last_error())
        assert ctx.deep_len() == 0
    assert raw_deep(ctx, "ms_deep_compose", flat, lists, g, null_struct=True) == ms.ERR_ARG
    assert raw_deep(ctx, "ms_deep_evals", flat, lists, None) == ms.ERR_ARG
    assert raw_deep(ctx, "ms_deep_evals", flat, [[0, c + m], [1]], [0] * 3 * e) == ms.ERR_ARG
    assert raw_deep(ctx, "ms_deep_evals", list(coset) + flat[e:], lists, [0] * 4 * e) == ms.ERR_SHAPE
    assert ctx.L.ms_deep_len(None) == 0
    assert reference(ctx) == want                                            # after the refusals: what a fresh context gives
    assert ctx.deep_len() == N
    for zz, ll, gg, npts, code in bad[4:]:                                   # a refusal leaves the installed polynomial alone
        assert raw_deep(ctx, "ms_deep_compose", zz, ll, gg, npts=npts) == code
    assert ctx.deep_len() == N and ctx.fri_begin(blowup, 2)[0] == 0 and tuples(ctx.fri_round_poly(0)) == want[1]
    # a mix stage clears the DEEP polynomial and the tree
    assert ctx.mix_air_ext(r, cons, exempt, periodic, boundary) == 0
    assert ctx.deep_len() == 0
    assert oc.raw_open(ctx, ms.TREE_VALIDITY, 0, [0], 1, None, 0)[0] == ms.ERR_STATE
    assert raw_deep(ctx, "ms_deep_compose", flat, lists, g) == ms.ERR_STATE
    assert ctx.fri_begin(blowup, 2)[0] == 0 and tuples(ctx.fri_round_poly(0)) == tuples(ctx.validity_read())[:ctx.fri_round_info(0)[0]]
    # ... and so do ms_lde_commit, ms_polys_* and ms_trace_commit
    for kill in (lambda: ctx.lde_commit(blowup, shift, c)[0], lambda: ctx.polys_append([1, 2, 3]), lambda: ctx.trace_commit(trace, c)[0]):
        commit(ctx, trace, blowup, shift)
        assert ctx.mix_air_ext(r, cons, exempt, periodic, boundary) == 0 and ctx.validity_commit(m) == (0, root)
        assert ctx.deep_compose(zs, lists, g) == 0 and ctx.deep_len() == N
        assert kill() == 0
        assert ctx.deep_len() == 0 and oc.raw_open(ctx, ms.TREE_VALIDITY, 0, [0], 1, None, 0)[0] == ms.ERR_STATE
    # ms_mix (ve = 1, no LDE needed for the mix itself) on a context without an LDE: no tree
    ctx.trace_commit(trace, c); ctx.interpolate()
    assert ctx.mix(5) == 0 and ctx.validity_commit(1)[0] == ms.ERR_STATE


def case_invariance(make, d, field):
    """ms_validity_commit, openings of its tree and ms_deep_evals between the stages, but no compose: MSFP and MSFI bytes of the proof are what they are without"""
    p, e = MODULUS[field], EXT[field]
    N, blowup, R = 64, 8, 4
    trace, cons, exempt, periodic, boundary = cubic_spec(field, N)
    c = trace.shape[1]
    outs = []
    for inserted in (False, True):
        ctx = ctx_of(make, d, field)
        rng = SplitMix64(31)
        commit(ctx, trace, blowup, rng.nonzero(p))
        assert ctx.mix_air_ext(full_ext(rng, field), cons, exempt, periodic, boundary) == 0
        z = full_ext(rng, field)
        if inserted:
            m = e * vl_of(ctx) // N
            assert ctx.validity_commit(m)[0] == 0
            assert ctx.deep_evals([z], [list(range(c + m))])[0] == 0
            ctx.tree_open(ms.TREE_VALIDITY, [0, N])
        o = [ctx.validity_read().tobytes(), ctx.eval_ext(np.array(z, dtype=np.uint64))[1].tobytes()]
        S = oc.commit_phase(ctx, field, blowup, R, seed=32)
        if inserted:
            assert ctx.deep_evals([z], [[0, c]])[0] == 0
            ctx.tree_open(ms.TREE_VALIDITY, [1])
        o += [S["roots"], ctx.fri_query([9, 10])[1], ctx.fri_query_index([9, 10])]
        outs.append(o)
    assert outs[0] == outs[1]


def case_sharded(ctx):
    """a context with sharding on (a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses the new entry points, as ms_aux_running and ms_tree_open do"""
    from mini_stark_amd.dist import LocalShard
    sh = LocalShard(ctx, 4 << 20)
    trace = fib_spec(0, 64)[0]
    commit(ctx, trace, 4, 3)
    assert ctx.mix(5) == 0
    assert ctx.validity_commit(1)[0] == ms.ERR_STATE and "sharding" in ctx.last_error()
    assert raw_deep(ctx, "ms_deep_evals", [(1, 2)], [[0]], [0, 0]) == ms.ERR_STATE and "sharding" in ctx.last_error()
    assert raw_deep(ctx, "ms_deep_compose", [(1, 2)], [[0]], [1, 2]) == ms.ERR_STATE and "sharding" in ctx.last_error()
    assert oc.raw_open(ctx, ms.TREE_VALIDITY, 0, [0], 1, None, 0)[0] == ms.ERR_STATE
    assert ctx.deep_len() == 0
    sh.close()


def case_launches(make, field, N, d=SHA):
    """ms_deep_compose: one combine launch whatever the number of points, 2 levels - 1 scan launches, one scale launch"""
    p, e = MODULUS[field], EXT[field]
    ctx = ctx_of(make, d, field)
    rng = SplitMix64(55)
    commit(ctx, rand_field(field, (N, 3), seed=N), 2, rng.nonzero(p))
    assert ctx.mix(rng.nonzero(p)) == 0 and ctx.validity_commit(1)[0] == 0
    zs = shifted_points(field, full_ext(rng, field), ctx.root_of_unity(N), range(8))
    rc, prof = oc.profile(ctx, lambda: ctx.deep_compose(zs, point_lists(3, 8), full_ext(rng, field)))
    assert rc == 0
    levels = 1 if N <= 2048 else 2
    assert prof["deep_combine"]["launches"] == 1 and prof["deep_scale"]["launches"] == 1 and prof["suffix_horner"]["launches"] == 2 * levels - 1
    assert sum(v["launches"] for k, v in prof.items() if isinstance(v, dict) and "launches" in v) == 2 * levels + 1
