"""Cases of ms_air_check (build-defined, diagnostic: the ms_air program of ms_mix_air evaluated on the rows of the trace domain; include/ministark.h), shared by the
emulation suite (tests/test_air_check_emu.py) and the GPU suite (tests/test_air_check_gpu.py).  The entry point is held to the restatement of its definitions in Python
integers (tests/pyref_air_check.py); every comparison is exact.  Programs and traces come from tests/air_cases.py and tests/aux_cases.py.  Nothing here is derived from
the kernel's constants: the sizes and rows are chosen so that faults share a thread, a wave, a workgroup or none of them whatever those constants are.
`mk(field, flags=0)` returns a new mini_stark_amd.Context."""
import ctypes as C
import itertools
import json

import numpy as np

import mini_stark_amd as ms
import air_cases as ac
import aux_cases as xa
import pyref
import pyref_air_check as rc_
from common import MODULUS, EXT, SplitMix64

ERR_SHAPE, ERR_STATE, ERR_ARG = ms.ERR_SHAPE, ms.ERR_STATE, ms.ERR_ARG
PER = ms.AIR_PERIODIC
assert PER == rc_.PERIODIC
_u64p = C.POINTER(C.c_uint64)


def lists(sp, **over):
    a = dict(sp, **over)
    return a["cons"], a["exempt"], a["periodic"], a["boundary"]


def columns(trace):
    return [[int(v) for v in trace[:, j]] for j in range(trace.shape[1])]


def norm(rep):
    """a report of Context.air_check with plain Python values, as pyref_air_check.check gives it"""
    return {"nfail": int(rep["nfail"]), "count": [int(v) for v in rep["count"]], "first_row": [int(v) for v in rep["first_row"]], "bnd_got": [int(v) for v in rep["bnd_got"]],
            "bnd_fail": [int(b) for b in rep["bnd_fail"]], "first": None if rep["first"] is None else (int(rep["first"][0]), int(rep["first"][1])), "ok": bool(rep["ok"])}


def checked(ctx, field, cols, prog):
    """ms_air_check of prog = (cons, exempt, periodic, boundary) on ctx equals the restatement over cols; returns the report"""
    cons, exempt, periodic, boundary = prog
    rc, rep = ctx.air_check(cons, exempt, periodic, boundary)
    assert rc == 0, ctx.last_error()
    want = rc_.check(MODULUS[field], len(cols[0]), cols, cons, exempt, periodic, boundary)
    assert norm(rep) == want
    return want


def clean(want, N, boundary):
    return (want["ok"] and want["nfail"] == 0 and not any(want["count"]) and all(r == N for r in want["first_row"]) and want["first"] is None
            and want["bnd_got"] == [int(b[2]) for b in boundary] and not want["bnd_fail"])


def commit_trace(ctx, trace):
    rc, _ = ctx.trace_commit(trace, trace.shape[1])
    assert rc == 0, ctx.last_error()


def both_states(ctx, field, trace, prog, blowup=None, shift=3):
    """the check before ms_interpolate and after it (and after ms_lde_commit when a blowup is given); the reports agree with the restatement, hence with each other"""
    cols = columns(trace)
    commit_trace(ctx, trace)
    want = checked(ctx, field, cols, prog)
    assert ctx.interpolate() == 0
    assert checked(ctx, field, cols, prog) == want
    if blowup:
        rc, _ = ctx.lde_commit(blowup, shift, ctx.polys_count())
        assert rc == 0, ctx.last_error()
        assert checked(ctx, field, cols, prog) == want
    return want


def raw_check(ctx, air, nfail=True, count=None, first_row=None, bnd_got=None):
    """ms_air_check through the raw ABI: `air` a flatten_air dict in which any array may be None (NULL), or None; returns (rc, nfail or None)"""
    nf = C.c_uint64(0xDEAD)
    ptr = [None if a is None else a.ctypes.data_as(_u64p) for a in (count, first_row, bnd_got)]
    if air is None:
        return ctx.L.ms_air_check(ctx.h, None, C.byref(nf), *ptr), None
    s, _keep = ms.air_struct(air)
    rc = ctx.L.ms_air_check(ctx.h, C.byref(s), C.byref(nf) if nfail else None, *ptr)
    return rc, (int(nf.value) if rc == 0 else None)


def profiled(ctx, stage):
    """(result of `stage`, the profile record) with every launch bracketed by ms_profile_begin / ms_profile_end"""
    buf = C.create_string_buffer(1 << 15)
    assert ctx.L.ms_profile_begin(ctx.h) == 0
    out = stage()
    assert ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))) == 0
    return out, json.loads(buf.value.decode())


def launches(prof):
    return {k: v["launches"] for k, v in prof.items() if isinstance(v, dict) and "launches" in v and v["launches"]}


# ---------------------------------------------------------------- 1. clean traces
def case_clean(mk, field, name, blowup, N=16):
    """every program of air_cases on its own trace: nothing fails, before ms_interpolate, after it and after ms_lde_commit; ms_mix_air then accepts the program"""
    sp = ac.SPECS[name](field, N)
    ctx = mk(field)
    want = both_states(ctx, field, sp["trace"], lists(sp), blowup, SplitMix64(900 + blowup).nonzero(MODULUS[field]))
    assert clean(want, N, sp["boundary"])
    assert ac.mix(ctx, 12345, sp) == 0, ctx.last_error()
    assert checked(ctx, field, columns(sp["trace"]), lists(sp)) == want


# ---------------------------------------------------------------- 2. one planted fault
def fault_rows(N):
    return [0, 1, N // 2, N - 2, N - 1]


def case_planted(mk, field, log_n, rho, blowup=4):
    """one cell of the mimc trace changed at row rho: the constraint reads rows i and i + 1 (and i + N - 1), so the rows around rho - across the wrap N - 1 -> 0 too -
    are reported exactly as the restatement says, the boundary value where rho is a boundary row; ms_mix_air refuses the trace"""
    p, N = MODULUS[field], 1 << log_n
    sp = ac.spec_mimc(field, N)
    trace = sp["trace"].copy()
    trace[rho, 0] = (int(trace[rho, 0]) + 1) % p
    ctx = mk(field)
    want = both_states(ctx, field, trace, lists(sp), blowup, 7)
    assert want["nfail"] >= 1 and want["count"][0] >= 1 and want["count"][1] == 0
    assert want["first"][0] in ((rho - 1) % N, rho)
    assert (want["bnd_fail"] == [0]) if rho == 0 else (want["bnd_fail"] == [1]) if rho == N - 1 else not want["bnd_fail"]
    assert ac.mix(ctx, 4321, sp) == ERR_SHAPE
    assert checked(ctx, field, columns(trace), lists(sp)) == want            # (the natural place to call it: behind the refusal)


def case_exempt_rows(mk, field, N=16):
    """x' = x^2 + 1, exempt on {3, N/2, N-1}, on a trace that breaks it on exactly those rows: nothing is reported; with one exempt row moved to its neighbour the row
    it left is reported, once, and nothing else"""
    sp = ac.spec_scattered(field, N)
    cols = columns(sp["trace"])
    ctx = mk(field)
    commit_trace(ctx, sp["trace"])
    X = sp["exempt"][0]
    assert sorted(X) == [3, N // 2, N - 1]
    assert clean(checked(ctx, field, cols, lists(sp)), N, ())
    for rho in X:
        moved = [k for k in X if k != rho] + [(rho + 1) % N]
        want = checked(ctx, field, cols, lists(sp, exempt=[moved]))
        assert (want["nfail"], want["count"], want["first_row"], want["first"]) == (1, [1], [rho], (rho, 0))


# ---------------------------------------------------------------- 3. dense faults
def dense_program(p, N, c=5):
    """constraint 0 is the constant c on every row, exempt on {0, 1, N-1}; constraint 1 (x - x) is there because a program needs a term with a factor"""
    return [[(c, [])], [(1, [(0, 0)]), (p - 1, [(0, 0)])]], [sorted({0, 1 % N, N - 1}), []], [], []


def case_dense_constant(mk, field, N):
    """every non-exempt row violates: the count is N - |X| exactly (rows past N of a workgroup's share are not counted, no row is counted twice), the first row is
    the smallest row outside X"""
    p = MODULUS[field]
    rng = SplitMix64(930 + N)
    trace = np.array([[rng.field(p)] for _ in range(N)], dtype=np.uint64)
    prog = dense_program(p, N)
    X = prog[1][0]
    want = both_states(mk(field), field, trace, prog)
    free = [i for i in range(N) if i not in X]
    assert want["count"] == [N - len(X), 0] and want["first_row"] == [free[0] if free else N, N] and want["nfail"] == (1 if free else 0)
    if N >= 4:
        assert want["count"][0] == N - 3 and want["first_row"][0] == 2


def case_dense_random(mk, field, name, N=1 << 11):
    """a random trace against a real program: (nearly) every row violates, every count and first row as the restatement gives them"""
    p = MODULUS[field]
    sp = ac.SPECS[name](field, N)
    rng = SplitMix64(940 + field)
    trace = np.array([[rng.field(p) for _ in range(sp["trace"].shape[1])] for _ in range(N)], dtype=np.uint64)
    want = both_states(mk(field), field, trace, lists(sp))
    assert want["count"][0] > N - 8 and want["first_row"][0] <= 8


# ---------------------------------------------------------------- 4. reduction geometry
GEOMETRY_ROWS = lambda N: [5, 5 + 64, 5 + 256, 5 + 512, 5 + 2048, N - 1]   # noqa: E731


def case_geometry(mk, field, N=1 << 12):
    """columns a, b with a_i = b_i = a_0 + i: constraint 0 is a - b, constraint 1 a' - a - 1 (exempt on {N-1}).  a is changed on two rows, for every pair of
    GEOMETRY_ROWS: the two faults share a thread's rows, a wave, a workgroup, or nothing, whatever the kernel's shape is.  Count and first row per constraint are the
    restatement's: constraint 0 exactly the two rows, the smaller first"""
    p = MODULUS[field]
    rng = SplitMix64(950 + field)
    a0 = rng.field(p)
    base = np.array([[(a0 + i) % p, (a0 + i) % p] for i in range(N)], dtype=np.uint64)
    prog = ([[(1, [(0, 0)]), (p - 1, [(1, 0)])], [(1, [(0, 1)]), (p - 1, [(0, 0)]), (p - 1, [])]], [[], [N - 1]], [], [])
    ctx = mk(field)
    for k, (r1, r2) in enumerate(itertools.combinations(GEOMETRY_ROWS(N), 2)):
        trace = base.copy()
        trace[r1, 0] = (int(trace[r1, 0]) + 7) % p
        trace[r2, 0] = (int(trace[r2, 0]) + 9) % p
        cols = columns(trace)
        commit_trace(ctx, trace)
        want = checked(ctx, field, cols, prog)
        assert want["count"][0] == 2 and want["first_row"][0] == min(r1, r2) and want["count"][1] >= 2
        if k % 4 == 0:                      # ... and through the transform, for every fourth pair
            assert ctx.interpolate() == 0
            assert checked(ctx, field, cols, prog) == want


# ---------------------------------------------------------------- 6. periodic columns
def case_periodic(mk, field, N):
    """the selector program: periods 2, 1 and min(N, 256), the last read one row ahead.  Clean on its own trace; with one value of each periodic column changed in turn
    the rows that read it are reported as the restatement says, in both states"""
    p = MODULUS[field]
    sp = ac.spec_selector(field, N)
    assert [len(v) for v in sp["periodic"]] == [2, 1, min(N, 256)]
    ctx = mk(field)
    assert clean(both_states(ctx, field, sp["trace"], lists(sp)), N, ())
    cols = columns(sp["trace"])
    for k, at in ((0, 1), (1, 0), (2, min(N, 256) - 1), (2, 1)):
        per = [list(v) for v in sp["periodic"]]
        per[k][at] = (per[k][at] + 1) % p
        commit_trace(ctx, sp["trace"])
        want = checked(ctx, field, cols, lists(sp, periodic=per))
        assert want["nfail"] == 1 and want["count"][0] >= 1
        assert ctx.interpolate() == 0
        assert checked(ctx, field, cols, lists(sp, periodic=per)) == want


# ---------------------------------------------------------------- 7. boundary constraints
def case_boundary(mk, field, N=16):
    """a wrong value; two constraints on one cell, one right and one wrong; a constraint on a running column of ms_aux_running (before ms_interpolate: index w)"""
    p = MODULUS[field]
    sp = ac.spec_fib_bounded(field, N)
    t = sp["trace"]
    right = list(sp["boundary"])
    wrong = [right[0], (1, 0, (int(t[0, 1]) + 1) % p), right[2], (1, N - 1, int(t[N - 1, 1])), (1, N - 1, (int(t[N - 1, 1]) + 5) % p)]
    ctx = mk(field)
    want = both_states(ctx, field, t, lists(sp, boundary=wrong), 2, 3)
    assert want["bnd_got"] == [int(t[0, 0]), int(t[0, 1]), int(t[N - 1, 1]), int(t[N - 1, 1]), int(t[N - 1, 1])]
    assert want["bnd_fail"] == [1, 4] and want["nfail"] == 2 and not any(want["count"]) and want["first"] is None and not want["ok"]
    assert ac.mix(ctx, 99, sp, boundary=wrong) == ERR_SHAPE and ac.mix(ctx, 99, sp) == 0
    # a running column
    rng = SplitMix64(970 + field)
    rows, op, fr = xa.spec_permutation(field, 1, N, rng)
    ctx = mk(field)
    tr = xa.commit_trace(ctx, rows)
    rc, _final, col = ctx.aux_running(op, fr, 1, read=True)
    assert rc == 0, ctx.last_error()
    w = tr.shape[1]
    cols = columns(tr) + [[int(v) for v in col[:, 0]]]
    cons = [[(1, [(w, 0)]), (p - 1, [(w, 0)])]]
    bnd = [(w, 0, int(col[0, 0])), (w, N // 2, (int(col[N // 2, 0]) + 1) % p), (0, 3, int(tr[3, 0]))]
    want = checked(ctx, field, cols, (cons, [[]], [], bnd))
    assert want["bnd_got"] == [int(col[0, 0]), int(col[N // 2, 0]), int(tr[3, 0])] and want["bnd_fail"] == [1] and want["nfail"] == 1
    assert ctx.interpolate() == 0
    assert checked(ctx, field, cols, (cons, [[]], [], bnd)) == want


# ---------------------------------------------------------------- 8. after ms_interpolate: the polynomials of ms_polys_lincomb and ms_polys_append
def case_after_interpolate(mk, field, N=16, blowup=4):
    """polynomial 2 = 2 P_0 + 3 P_1 (ms_polys_lincomb: lazily defined, or written out by ms_poly_read first), polynomial 3 uploaded by ms_polys_append as the interpolant
    of a_i^2.  The program ties both to the trace columns; with one value of the appended column wrong its row is reported.  The same report after a refused ms_mix_air and
    after a finished ms_fri_query"""
    p, e = MODULUS[field], EXT[field]
    sp = ac.spec_fib_bounded(field, N)
    t = sp["trace"]
    a, b = columns(t)
    lin = [(2 * x + 3 * y) % p for x, y in zip(a, b)]
    cons = ac.FIB_CONS(p) + [[(1, [(2, 0)]), (p - 2, [(0, 0)]), (p - 3, [(1, 0)])], [(1, [(3, 1)]), (p - 1, [(0, 1), (0, 1)])]]
    exempt = [[N - 1], [N - 1], [], []]
    bnd = [(2, 5, lin[5]), (3, 0, a[0] * a[0] % p)]
    for lazy in (True, False):
        for spoil in (False, True):
            sq = [x * x % p for x in a]
            if spoil:
                sq[7] = (sq[7] + 1) % p
            ctx = mk(field)
            commit_trace(ctx, t)
            rc, rep = ctx.air_check(cons, exempt, [], bnd)
            assert rc == ERR_ARG                                               # (polynomials 2 and 3 do not exist yet)
            assert ctx.interpolate() == 0
            assert ctx.polys_lincomb([2, 3], [0, 1]) == 0
            assert ctx.polys_append(pyref.dft(field, sq, inverse=True)) == 0
            if not lazy:
                assert [int(v) for v in ctx.poly_read(2)] == pyref.dft(field, lin, inverse=True)
            cols = [a, b, lin, sq]
            want = checked(ctx, field, cols, (cons, exempt, [], bnd))
            rc, _ = ctx.lde_commit(blowup, 3, ctx.polys_count())
            assert rc == 0, ctx.last_error()
            assert checked(ctx, field, cols, (cons, exempt, [], bnd)) == want
            if spoil:
                assert (want["nfail"], want["count"], want["first_row"], want["first"]) == (1, [0, 0, 0, 1], [N, N, N, 6], (6, 3))   # (the constraint reads row i + 1)
                assert ctx.mix_air(77, cons, exempt, [], bnd) == ERR_SHAPE
                assert checked(ctx, field, cols, (cons, exempt, [], bnd)) == want
                continue
            assert clean(want, N, bnd)
            assert ctx.mix_air(77, cons, exempt, [], bnd) == 0, ctx.last_error()
            rng = SplitMix64(980)
            rounds = (ac.validity_len_of(ctx) * blowup).bit_length() - 1
            rc, _root0 = ctx.fri_begin(blowup, rounds)
            assert rc == 0, ctx.last_error()
            for _ in range(1, rounds):
                rc, _B = ctx.fri_deep([rng.field(p) for _ in range(e)])
                assert rc == 0
                rc, _root = ctx.fri_fold_commit([rng.field(p) for _ in range(e)])
                assert rc == 0, ctx.last_error()
            rc, proof = ctx.fri_query([rng.next(), 5])
            assert rc == 0 and len(proof) > 0
            assert checked(ctx, field, cols, (cons, exempt, [], bnd)) == want
            assert ctx.fri_proof_read() == proof


# ---------------------------------------------------------------- 9. running columns
def case_running(mk, field, ext, N=64):
    """the ms_aux_running column of a permutation argument with the constraints mini_stark_amd.aux_constraints writes out: clean with the challenge the column was built
    with; with another challenge the report is the restatement's over the trace columns and column_out"""
    p = MODULUS[field]
    rng = SplitMix64(990 + 16 * field + ext)
    rows, op, fr = xa.spec_permutation(field, ext, N, rng)
    ctx = mk(field)
    tr = xa.commit_trace(ctx, rows)
    w = tr.shape[1]
    rc, _final, col = ctx.aux_running(op, fr, ext, read=True)
    assert rc == 0, ctx.last_error()
    cols = columns(tr) + [[int(v) for v in col[:, l]] for l in range(ext)]
    cons, exempt, boundary = ms.aux_constraints(field, op, fr, ext, w, exempt_last=False, N=N)
    assert clean(checked(ctx, field, cols, (cons, exempt, [], boundary)), N, boundary)
    other = xa.rand_k(rng, p, ext)
    (num_c, num_t), (den_c, den_t) = fr[0]
    assert other != num_c
    cons2, exempt2, boundary2 = ms.aux_constraints(field, op, [((other, num_t), (other, den_t))], ext, w, exempt_last=False, N=N)
    want = checked(ctx, field, cols, (cons2, exempt2, [], boundary2))
    assert want["nfail"] >= 1 and max(want["count"]) > N // 2
    assert ctx.interpolate() == 0 and ctx.polys_count() == w + ext
    assert checked(ctx, field, cols, (cons2, exempt2, [], boundary2)) == want
    assert clean(checked(ctx, field, cols, (cons, exempt, [], boundary)), N, boundary)


# ---------------------------------------------------------------- 10. the context is unchanged
def prove(ctx, field, sp, trace, blowup, hook):
    """a whole proof of sp's program over `trace` (what ms_trace_commit is fed): roots, validity polynomial, DEEP-ALI values, FRI roots, MSFP bytes.  hook(stage) runs
    behind ms_trace_commit ("trace"), ms_interpolate ("polys"), ms_lde_commit ("lde"), ms_mix_air ("mix") and ms_fri_query ("fri")"""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(1234)
    out = []
    rc, root = ctx.trace_commit(trace, trace.shape[1])
    assert rc == 0, ctx.last_error()
    out.append(root)
    hook("trace")
    assert ctx.interpolate() == 0
    hook("polys")
    rc, root = ctx.lde_commit(blowup, rng.nonzero(p), ctx.polys_count())
    assert rc == 0, ctx.last_error()
    out.append(root)
    hook("lde")
    assert ac.mix(ctx, rng.field(p), sp) == 0, ctx.last_error()
    hook("mix")
    out.append(ctx.validity_read().tolist())
    rc, ev = ctx.eval_ext(np.array([[rng.field(p) for _ in range(e)] for _ in range(2)], dtype=np.uint64))
    assert rc == 0
    out.append(ev.tolist())
    VL = ac.validity_len_of(ctx)
    rounds = (VL * blowup).bit_length() - 1
    rc, root = ctx.fri_begin(blowup, rounds)
    assert rc == 0, ctx.last_error()
    out.append(root)
    for _ in range(1, rounds):
        rc, B = ctx.fri_deep([rng.field(p) for _ in range(e)])
        assert rc == 0
        rc, root = ctx.fri_fold_commit([rng.field(p) for _ in range(e)])
        assert rc == 0, ctx.last_error()
        out.append((B.tolist(), root))
    rc, proof = ctx.fri_query([rng.next(), 5])
    assert rc == 0 and len(proof) > 0
    hook("fri")
    out.append(ctx.fri_proof_read())
    assert out[-1] == proof
    return out


def case_unchanged(mk, field, mont=False, N=16, blowup=4):
    """a proof with checks behind every stage - the program itself (clean) and another program that fails - is byte for byte the proof without them.  mont: the context
    takes the trace as x * 2^64 mod p (MS_FLAG_TRACE_MONT64); its proof is the canonical context's, and the check reads canonical column values"""
    p = MODULUS[field]
    sp = ac.spec_mimc(field, N)
    cols = columns(sp["trace"])
    flags = ms.FLAG_TRACE_MONT64 if mont else 0
    fed = np.array([[int(v) * (1 << 64) % p for v in row] for row in sp["trace"]], dtype=np.uint64) if mont else sp["trace"]
    failing = ([[(1, [(0, 0)]), (p - 1, [(1, 0)])]], [[2]], [], [(1, 3, (int(sp["trace"][3, 1]) + 1) % p)])
    seen = []

    def hook(stage):
        assert clean(checked(ctx, field, cols, lists(sp)), N, sp["boundary"])
        want = checked(ctx, field, cols, failing)
        assert want["nfail"] == 2
        seen.append(stage)
    ctx = mk(field, flags)
    with_checks = prove(ctx, field, sp, fed, blowup, hook)
    assert seen == ["trace", "polys", "lde", "mix", "fri"]
    plain = prove(mk(field, flags), field, sp, fed, blowup, lambda stage: None)
    assert with_checks == plain
    if mont:
        assert plain == prove(mk(field), field, sp, sp["trace"], blowup, lambda stage: None)
    assert prove(ctx, field, sp, fed, blowup, lambda stage: None) == plain        # ... and the context that ran the checks proves again


# ---------------------------------------------------------------- 11. refusals
def case_refusals(mk, field, N=16, blowup=4):
    p = MODULUS[field]
    sp = ac.spec_mimc(field, N)
    air = ms.flatten_air(*lists(sp))
    cols = columns(sp["trace"])
    ctx = mk(field)
    assert raw_check(ctx, air)[0] == ERR_STATE                                   # no committed trace
    commit_trace(ctx, sp["trace"])
    fresh = checked(mk_committed(mk, field, sp["trace"]), field, cols, lists(sp))
    assert clean(fresh, N, sp["boundary"])

    def still_fine():
        assert checked(ctx, field, cols, lists(sp)) == fresh

    def arg(**over):
        assert raw_check(ctx, dict(air, **over))[0] == ERR_ARG, sorted(over)
        still_fine()

    def arr(name, at, value):
        b = air[name].copy()
        b[at] = value
        return {name: b}
    u32 = lambda v: np.array(v, dtype=np.uint32)   # noqa: E731
    assert raw_check(ctx, None)[0] == ERR_ARG                                    # null program
    still_fine()
    assert raw_check(ctx, air, nfail=False)[0] == ERR_ARG                        # null nfail
    still_fine()
    assert raw_check(ctx, air) == (0, 0)                                         # all three detail pointers null
    failing = dict(air, bnd_val=arr("bnd_val", 1, (int(air["bnd_val"][1]) + 1) % p)["bnd_val"])
    assert raw_check(ctx, failing) == (0, 1)
    for name, _t in ms._native.AIR_ARRAYS:                                      # every array of this program is needed
        arg(**{name: None})
    arg(**arr("coef", 1, p))                                                     # a coefficient, a periodic value, a boundary value not canonical
    arg(**arr("per_val", 3, p))
    arg(**arr("bnd_val", 1, p))
    # the limits
    arg(ncons=0)
    arg(ncons=4097, term_begin=np.zeros(4098, dtype=np.uint32), ex_begin=np.zeros(4098, dtype=np.uint32))
    arg(nperiodic=65, per_begin=np.arange(66, dtype=np.uint32), per_val=np.ones(65, dtype=np.uint64))
    arg(nbound=4097, bnd_poly=np.zeros(4097, dtype=np.uint32), bnd_row=np.zeros(4097, dtype=np.uint32), bnd_val=np.zeros(4097, dtype=np.uint64))
    arg(ex_begin=u32([0, 17, 18]), ex_row=u32(list(range(16)) + [0, 0]))
    nt = 65537
    arg(ncons=1, term_begin=u32([0, nt]), coef=np.ones(nt, dtype=np.uint64), fac_begin=np.arange(nt + 1, dtype=np.uint32), fac_poly=np.zeros(nt, dtype=np.uint32),
        fac_row=np.zeros(nt, dtype=np.uint32), ex_begin=u32([0, 0]))
    one = dict(ncons=1, term_begin=u32([0, 1]), coef=np.array([1], dtype=np.uint64), ex_begin=u32([0, 1]), ex_row=u32([N - 1]))
    arg(**dict(one, fac_begin=u32([0, 9]), fac_poly=u32([0] * 9), fac_row=u32([0] * 9)))                     # a term with 9 factors
    assert raw_check(ctx, dict(air, **dict(one, fac_begin=u32([0, 8]), fac_poly=u32([0] * 8), fac_row=u32([0] * 8))))[0] == 0   # (8 are allowed)
    arg(**dict(one, term_begin=u32([0, 2]), coef=np.array([1, 2], dtype=np.uint64), fac_begin=u32([0, 0, 0]), fac_poly=u32([0]), fac_row=u32([0])))   # d = 0
    # malformed CSR
    arg(term_begin=u32([0, 7, 3]))
    arg(term_begin=u32([1, 6, 8]))
    arg(**arr("fac_begin", 2, int(air["fac_begin"][1]) - 1))
    arg(**arr("fac_begin", 0, 1))
    arg(ex_begin=u32([1, 1, 2]))
    arg(ex_begin=u32([0, 2, 1]))
    arg(per_begin=u32([1, 4]))
    arg(per_begin=u32([0, 0]))
    # indices
    arg(**arr("fac_poly", 0, 2))                                                 # column index >= w (+ ms_aux_count)
    arg(**arr("fac_row", 0, N))
    arg(**arr("fac_poly", 4, PER | 1))
    arg(**arr("bnd_poly", 0, 2))
    arg(**arr("bnd_row", 0, N))
    arg(**arr("ex_row", 0, N))
    arg(ex_begin=u32([0, 2, 3]), ex_row=u32([5, 5, 0]))
    # periods
    arg(per_begin=u32([0, 3]), per_val=np.ones(3, dtype=np.uint64))
    arg(per_begin=u32([0, 2 * N]), per_val=np.ones(2 * N, dtype=np.uint64))
    # more than 32 distinct exemption sets
    n = 33
    sets = [sorted({t % N, (t + t // N) % N}) for t in range(n)]
    many = dict(ncons=n, term_begin=u32(range(n + 1)), coef=np.ones(n, dtype=np.uint64), fac_begin=u32(range(n + 1)), fac_poly=u32([0] * n), fac_row=u32([0] * n),
                ex_begin=u32(np.cumsum([0] + [len(s) for s in sets])), ex_row=u32([k for s in sets for k in s]))
    arg(**many)
    sets[-1] = sets[0]                                                           # ... 32 are checked: every constraint is "x", which is not 0
    rc, nf = raw_check(ctx, dict(air, **dict(many, ex_begin=u32(np.cumsum([0] + [len(s) for s in sets])), ex_row=u32([k for s in sets for k in s]))))
    assert rc == 0 and nf >= n
    # an index that is out of range before ms_interpolate and in range after it: polynomial 2, defined by ms_polys_lincomb
    names2 = lists(sp, cons=sp["cons"] + [[(1, [(2, 0)]), (p - 1, [(0, 0)]), (p - 1, [(1, 0)])]], exempt=sp["exempt"] + [[]])
    rc, _ = ctx.air_check(*names2)
    assert rc == ERR_ARG and "air_check" in ctx.last_error()
    still_fine()
    assert ctx.interpolate() == 0
    rc, _ = ctx.air_check(*names2)
    assert rc == ERR_ARG
    assert ctx.polys_lincomb([1, 1], [0, 1]) == 0
    want = checked(ctx, field, cols + [[(x + y) % p for x, y in zip(*cols)]], names2)
    assert clean(want, N, sp["boundary"])
    rc, _ = ctx.air_check(*lists(sp, cons=[[(1, [(3, 0)])]], exempt=[[]]))
    assert rc == ERR_ARG
    still_fine()
    # no MS_ERR_SHAPE: a blowup at which ms_mix_air cannot decide exactness
    rc, _ = ctx.lde_commit(2, 3, ctx.polys_count())
    assert rc == 0
    assert ac.mix(ctx, 5, sp) == ERR_SHAPE
    still_fine()


def mk_committed(mk, field, trace):
    ctx = mk(field)
    commit_trace(ctx, trace)
    return ctx


def case_refusals_large(mk, field, N=512):
    """the limits only a longer trace reaches: a period above 256 that N would allow, periods summing to more than 4096, more than 16 distinct boundary rows"""
    sp = ac.spec_fib_bounded(field, N)
    cols = columns(sp["trace"])
    ctx = mk_committed(mk, field, sp["trace"])
    assert ctx.air_check(*lists(sp, periodic=[[1] * 512]))[0] == ERR_ARG
    assert ctx.air_check(*lists(sp, periodic=[[1] * 256] * 17))[0] == ERR_ARG
    assert clean(checked(ctx, field, cols, lists(sp, periodic=[[1] * 256] * 16)), N, sp["boundary"])
    b17 = [(0, k, int(sp["trace"][k, 0])) for k in range(17)]
    assert ctx.air_check(*lists(sp, boundary=b17))[0] == ERR_ARG
    assert clean(checked(ctx, field, cols, lists(sp, boundary=b17[:16])), N, b17[:16])


def case_sharded_refused(make_ctx, field, N=16):
    """a context with sharding on (a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses the check, as ms_aux_running and ms_mix_air_ext do"""
    from mini_stark_amd.dist import LocalShard
    sp = ac.spec_fib_bounded(field, N)
    ctx = make_ctx(field)
    sh = LocalShard(ctx, 32 * N * 4 + (4 << 20))
    commit_trace(ctx, sp["trace"])
    assert ctx.air_check(*lists(sp))[0] == ERR_STATE
    assert ctx.interpolate() == 0
    assert ctx.air_check(*lists(sp))[0] == ERR_STATE
    sh.close()


def case_alloc_failures(mk, field, lib, N=16):
    """emulation build only: every allocation the call makes fails in turn (ms_emu_fail_alloc_after for the host side, ms_emu_fail_device_alloc_after for device and
    page-locked memory) - the call returns a negative status, never unwinds, and the same context then gives the clean report, before and after ms_interpolate"""
    lib.ms_emu_alloc_count.restype = C.c_long
    lib.ms_emu_fail_alloc_after.argtypes = [C.c_long]
    lib.ms_emu_fail_device_alloc_after.argtypes = [C.c_long]
    sp = ac.spec_mimc(field, N)
    cols = columns(sp["trace"])
    ctx = mk_committed(mk, field, sp["trace"])
    for state in ("trace", "polys"):
        if state == "polys":
            assert ctx.interpolate() == 0
        want = checked(ctx, field, cols, lists(sp))
        n0 = lib.ms_emu_alloc_count()
        assert checked(ctx, field, cols, lists(sp)) == want
        total = lib.ms_emu_alloc_count() - n0
        assert total >= 2                       # the program tables of air_validate and the result vector, at the least
        for k in range(total):
            lib.ms_emu_fail_alloc_after(k)
            rc, rep = ctx.air_check(*lists(sp))
            lib.ms_emu_fail_alloc_after(-1)
            assert rc in (ms.ERR_NOMEM, ms.ERR_HIP) and rep is None and ctx.last_error(), (state, k, rc)
            assert checked(ctx, field, cols, lists(sp)) == want
    # device and page-locked buffers: a fresh context allocates them on its first check
    for k in range(8):
        ctx = mk_committed(mk, field, sp["trace"])
        assert ctx.interpolate() == 0
        lib.ms_emu_fail_device_alloc_after(k)
        rc, rep = ctx.air_check(*lists(sp))
        lib.ms_emu_fail_device_alloc_after(-1)
        assert rc in (0, ms.ERR_NOMEM, ms.ERR_HIP), (k, rc)
        assert (rc == 0) == (rep is not None)
        assert checked(ctx, field, cols, lists(sp)) == want
        if rc == 0:
            break
    assert rc == 0 and k >= 2                   # (the table, the evaluations and the staging area failed in turn before a call got through)


# ---------------------------------------------------------------- 12. launch count
def case_launch_count(mk, field, N=16):
    """before ms_interpolate the check is launches of class air_check only (one, or two where the boundary values get a launch of their own) and no transform;
    after it the passes of ONE forward transform and the same"""
    sp = ac.spec_mimc(field, N)
    ctx = mk_committed(mk, field, sp["trace"])
    (rc, rep), prof = profiled(ctx, lambda: ctx.air_check(*lists(sp)))
    assert rc == 0 and rep["ok"]
    got = launches(prof)
    assert set(got) == {"air_check"} and got["air_check"] in (1, 2)
    before = got["air_check"]
    assert ctx.interpolate() == 0
    (rc, rep), prof = profiled(ctx, lambda: ctx.air_check(*lists(sp)))
    assert rc == 0 and rep["ok"]
    got = launches(prof)
    assert set(got) == {"air_check", "ntt_pass"} and got["air_check"] == before and got["ntt_pass"] >= 1
    assert sum(v["launches"] for v in prof["ntt_pass_variants"].values()) == got["ntt_pass"]
