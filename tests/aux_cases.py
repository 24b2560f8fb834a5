"""Cases of ms_aux_running (build-defined: the running product of a permutation argument / the running sum of a LogUp lookup, built on the GPU from the committed
trace; include/ministark.h), shared by the emulation suite (tests/test_aux_emu.py) and the GPU suite (tests/test_aux_gpu.py).  The stage has no reference counterpart,
so it is held to the big-integer restatement of its definition (tests/pyref_aux.py): row by row with modular inverses at small sizes, by the recurrence without
inversions at the sizes that cross a tile or a carry-chunk boundary.  Field arithmetic is exact: every comparison is bit for bit.  Every case asserts in the
restatement that no denominator vanishes for its seed.  `mk(field, fresh=True)` returns a new mini_stark_amd.Context."""
import contextlib
import ctypes as C
import os

import numpy as np

import mini_stark_amd as ms
import pyref
import pyref_air as ra
import pyref_aux as rx
from common import MODULUS, EXT, SplitMix64
from mini_stark_amd.host import air_expected_validity
from terms_cases import omega_of, fibonacci_proof

ERR_SHAPE, ERR_STATE, ERR_ARG = ms.ERR_SHAPE, ms.ERR_STATE, ms.ERR_ARG
SUM, PRODUCT = ms.AUX_SUM, ms.AUX_PRODUCT
assert (SUM, PRODUCT) == (rx.SUM, rx.PRODUCT)
DEFAULT_TILE = 2048     # rows per workgroup of the tile launch (MS_AUX_TILE's default and upper end); the carry launch takes 256 tile aggregates at a time
CARRY_CHUNK = 256


@contextlib.contextmanager
def tile_env(tile):
    """MS_AUX_TILE for the contexts created inside (the knob is read at ms_create); None: the default"""
    old = os.environ.get("MS_AUX_TILE")
    try:
        if tile is None:
            os.environ.pop("MS_AUX_TILE", None)
        else:
            os.environ["MS_AUX_TILE"] = str(tile)
        yield
    finally:
        if old is None:
            os.environ.pop("MS_AUX_TILE", None)
        else:
            os.environ["MS_AUX_TILE"] = old


def rand_k(rng, p, ext):
    return rng.field(p) if ext == 1 else tuple(rng.field(p) for _ in range(ext))


def rand_trace(rng, p, N, w):
    return [[rng.field(p) for _ in range(w)] for _ in range(N)]


def rand_fractions(rng, p, ext, nfrac, w, nterms=(1, 2, 3)):
    """nfrac fractions of affine forms over w columns; form f has nterms[f % len(nterms)] terms"""
    out, f = [], 0
    for _ in range(nfrac):
        pair = []
        for _side in range(2):
            pair.append((rand_k(rng, p, ext), [(rng.next() % w, rand_k(rng, p, ext)) for _ in range(nterms[f % len(nterms)])]))
            f += 1
        out.append(tuple(pair))
    return out


def commit_trace(ctx, rows):
    t = np.array(rows, dtype=np.uint64)
    rc, _ = ctx.trace_commit(t, t.shape[1])
    assert rc == 0, ctx.last_error()
    return t


def as_tuples(col):
    return [tuple(int(v) for v in r) for r in col]


def as_k(final, ext):
    return (final,) if ext == 1 else tuple(final)


# ---------------------------------------------------------------- 1. the definition, small
def case_definition(mk, field, ext, op, nfrac, N, w=4):
    """column_out and final_out equal the row-by-row restatement; after ms_interpolate the limb columns are polynomials w .. w + ext - 1 = the inverse DFT of the
    limbs, and the trace polynomials are what a context without the call gives.  N = 16: fewer rows than threads; N = 64: one wave."""
    p = MODULUS[field]
    rng = SplitMix64(1000 + 64 * field + 16 * ext + 4 * op + nfrac + N)
    rows = rand_trace(rng, p, N, w)
    fr = rand_fractions(rng, p, ext, nfrac, w)
    want_col, want_final = rx.running(field, ext, op, fr, rows)
    ctx = mk(field, fresh=True)
    commit_trace(ctx, rows)
    assert ctx.aux_count() == 0
    rc, final, col = ctx.aux_running(op, fr, ext, read=True)
    assert rc == 0, ctx.last_error()
    assert as_k(final, ext) == want_final
    assert as_tuples(col) == want_col
    assert ctx.aux_count() == ext
    assert ctx.interpolate() == 0 and ctx.polys_count() == w + ext
    for l in range(ext):
        assert [int(v) for v in ctx.poly_read(w + l)] == pyref.dft(field, [z[l] for z in want_col], inverse=True)
    plain = mk(field, fresh=True)
    commit_trace(plain, rows)
    assert plain.interpolate() == 0 and plain.polys_count() == w
    for j in range(w):
        assert ctx.poly_read(j).tolist() == plain.poly_read(j).tolist()


# ---------------------------------------------------------------- 2. tile and carry-chunk boundaries
# (N, tile settings): with MS_AUX_TILE=256 N = 256 is exactly one tile (no carry launch), 512 the first carry, 2^13 = 32 tiles; 2^17 = 512 tiles is the one size
# <= 2^17 at which the carry launch takes a second chunk of 256 aggregates.  At the default tile: N = tile and N = 2 * tile.
BOUNDARY_SIZES = [256, 512, DEFAULT_TILE, 2 * DEFAULT_TILE, 1 << 13]
CHUNK_SIZE = 256 * CARRY_CHUNK * 2
assert CHUNK_SIZE == 1 << 17


def case_boundaries(mk, field, N, op, nfrac, w=3):
    """ext = E.  The column of the 256-row tile satisfies the recurrence (which determines it), and the column of the default tile equals it bit for bit."""
    p, ext = MODULUS[field], EXT[field]
    rng = SplitMix64(2000 + 7 * field + N + 2 * op + nfrac)
    rows = rand_trace(rng, p, N, w)
    fr = rand_fractions(rng, p, ext, nfrac, w, nterms=(1,))
    got = []
    for tile in (256, None):
        with tile_env(tile):
            ctx = mk(field, fresh=True)
        commit_trace(ctx, rows)
        rc, final, col = ctx.aux_running(op, fr, ext, read=True)
        assert rc == 0, ctx.last_error()
        got.append((as_k(final, ext), col.tolist()))
        ctx.close()
    assert rx.check_recurrence(field, ext, op, fr, rows, as_tuples(got[0][1]), got[0][0])
    assert got[0] == got[1]


# ---------------------------------------------------------------- 3. several columns
def case_several(mk, field, N=64, w=3):
    p, E = MODULUS[field], EXT[field]
    rng = SplitMix64(3000 + field)
    rows = rand_trace(rng, p, N, w)
    fr_a, fr_b = rand_fractions(rng, p, E, 2, w), rand_fractions(rng, p, 1, 3, w)
    col_a, fin_a = rx.running(field, E, PRODUCT, fr_a, rows)
    col_b, fin_b = rx.running(field, 1, SUM, fr_b, rows)
    ctx = mk(field, fresh=True)
    commit_trace(ctx, rows)
    rc, final, _ = ctx.aux_running(PRODUCT, fr_a, E)
    assert rc == 0 and tuple(final) == fin_a and ctx.aux_count() == E
    rc, final, col = ctx.aux_running(SUM, fr_b, 1, read=True)
    assert rc == 0 and (final,) == fin_b and as_tuples(col) == col_b and ctx.aux_count() == E + 1
    assert ctx.interpolate() == 0 and ctx.polys_count() == w + E + 1
    for l in range(E):                                                      # the columns land in call order
        assert [int(v) for v in ctx.poly_read(w + l)] == pyref.dft(field, [z[l] for z in col_a], inverse=True)
    assert [int(v) for v in ctx.poly_read(w + E)] == pyref.dft(field, [z[0] for z in col_b], inverse=True)
    commit_trace(ctx, rows)                                                 # ms_trace_commit resets the count ...
    assert ctx.aux_count() == 0
    assert ctx.interpolate() == 0 and ctx.polys_count() == w
    assert fibonacci_proof(ctx, field) == fibonacci_proof(mk(field, fresh=True), field)   # ... and a proof after it is the plain proof


# ---------------------------------------------------------------- 4. end to end: the column proves
def neg(p, v):
    return (-v) % p if not isinstance(v, tuple) else tuple((-x) % p for x in v)


def k_of(ext, b):
    return b if ext == 1 else (b,) + (0,) * (ext - 1)


def spec_permutation(field, ext, N, rng, spoil=False):
    """columns (a, b), b a shuffle of a: the product of (gamma + a_i) / (gamma + b_i) over all rows is 1"""
    p = MODULUS[field]
    a = [rng.field(p) for _ in range(N)]
    b = list(a)
    for i in range(N - 1, 0, -1):
        j = rng.next() % (i + 1)
        b[i], b[j] = b[j], b[i]
    if spoil:
        b[5] = (b[5] + 1) % p
    gamma = rand_k(rng, p, ext)
    one = k_of(ext, 1)
    return [[x, y] for x, y in zip(a, b)], PRODUCT, [((gamma, [(0, one)]), (gamma, [(1, one)]))]


def spec_logup(field, ext, N, rng):
    """columns (t, f, m): table t (distinct values), looked-up f (every entry a table value), m_i = how often t_i occurs in f:
    sum_i m_i / (gamma - t_i) - 1 / (gamma - f_i) = 0"""
    p = MODULUS[field]
    t = []
    while len(t) < N:
        v = rng.field(p)
        if v not in t:
            t.append(v)
    f = [t[rng.next() % 8] if i % 3 else t[rng.next() % N] for i in range(N)]
    m = [f.count(v) for v in t]
    gamma = rand_k(rng, p, ext)
    m1 = k_of(ext, p - 1)
    return [[x, y, z] for x, y, z in zip(t, f, m)], SUM, [((k_of(ext, 0), [(2, k_of(ext, 1))]), (gamma, [(0, m1)])), ((m1, []), (gamma, [(1, m1)]))]


def prove_column(ctx, field, ext, rows, op, fr, rng, exempt_last=False, blowup=4):
    """trace_commit, the column, interpolate, lde_commit; returns (final, status of ms_mix_air over aux_constraints, r, the program lists)"""
    p = MODULUS[field]
    N, w = len(rows), len(rows[0])
    commit_trace(ctx, rows)
    rc, final, col = ctx.aux_running(op, fr, ext, read=True)
    assert rc == 0, ctx.last_error()
    assert rx.check_recurrence(field, ext, op, fr, rows, as_tuples(col), as_k(final, ext))
    assert ctx.interpolate() == 0 and ctx.polys_count() == w + ext
    rc, _ = ctx.lde_commit(blowup, rng.nonzero(p), ctx.polys_count())
    assert rc == 0, ctx.last_error()
    cons, exempt, boundary = ms.aux_constraints(field, op, fr, ext, w, exempt_last=exempt_last, N=N)
    r = rng.field(p)
    return as_k(final, ext), ctx.mix_air(r, cons, exempt, (), boundary), r, (cons, exempt, [], boundary)


def case_end_to_end(mk, field, ext, which, N=64, blowup=4):
    """(a) permutation / (b) LogUp: final is the identity, so the transition constraint of aux_constraints needs no exemption: ms_mix_air accepts it with the boundary
    z_0 = identity, the validity polynomial is the restatement's, the DEEP-ALI identity holds at a random extension point, FRI starts and folds"""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(4000 + 16 * field + ext + (100 if which == "logup" else 0))
    rows, op, fr = spec_permutation(field, ext, N, rng) if which == "permutation" else spec_logup(field, ext, N, rng)
    w = len(rows[0])
    ctx = mk(field, fresh=True)
    final, rc, r, lists = prove_column(ctx, field, ext, rows, op, fr, rng)
    T = pyref.Tower(field, ext)
    assert final == rx.identity(T, op)
    assert rc == 0, ctx.last_error()
    cons, exempt, _, boundary = lists
    omega = omega_of(ctx, field, N)
    polys = [[int(v) for v in ctx.poly_read(j)] for j in range(w + ext)]
    VL = ra.validity_len(N, cons, exempt, len(boundary))
    want = ra.validity(p, omega, N, polys, r, cons, exempt, [], boundary, VL)
    assert any(want) and [int(v) for v in ctx.validity_read()] == want
    TE = pyref.Tower(field, e)
    z = tuple(rng.field(p) for _ in range(e))
    used = ms.air_rows(cons, boundary)
    assert used == [0, 1]
    rc, ev = ctx.eval_ext(np.array([TE.mul(z, TE.from_base(pow(omega, k, p))) for k in used], dtype=np.uint64))
    assert rc == 0
    rc, expect = air_expected_validity(field, r, lists, N, z, used, ev)
    assert rc == 0 and [int(x) for x in expect] == [int(x) for x in ev[0][w + ext]]
    rc, _root0 = ctx.fri_begin(blowup, (VL * blowup).bit_length() - 1)
    assert rc == 0, ctx.last_error()
    rc, _B = ctx.fri_deep([rng.field(p) for _ in range(e)])
    assert rc == 0
    rc, _root = ctx.fri_fold_commit([rng.field(p) for _ in range(e)])
    assert rc == 0, ctx.last_error()


def case_spoiled_permutation(mk, field, ext, N=64):
    """(c) one entry of the shuffled column changed: final is not 1 and the wrap from row N-1 to row 0 fails, so ms_mix_air refuses the program without exemption
    (MS_ERR_SHAPE) and accepts it with row N-1 exempt - the recurrence itself still holds"""
    rng = SplitMix64(4500 + 16 * field + ext)
    rows, op, fr = spec_permutation(field, ext, N, rng, spoil=True)
    T = pyref.Tower(field, ext)
    ctx = mk(field, fresh=True)
    final, rc, _, _ = prove_column(ctx, field, ext, rows, op, fr, SplitMix64(1))
    assert final != T.one() and rc == ERR_SHAPE
    final, rc, _, _ = prove_column(ctx, field, ext, rows, op, fr, SplitMix64(1), exempt_last=True)
    assert final != T.one() and rc == 0, ctx.last_error()


# ---------------------------------------------------------------- 5. refusals
def raw_aux(ctx, aux, final="buf", column=None):
    """ms_aux_running through the raw ABI: `aux` a flatten_aux dict in which any array may be None (NULL), or None for a null program; final=None: a null final_out"""
    u64p = C.POINTER(C.c_uint64)
    fin = np.zeros(4, dtype=np.uint64)
    fp = None if final is None else fin.ctypes.data_as(u64p)
    if aux is None:
        return ctx.L.ms_aux_running(ctx.h, None, fp, column)
    s, _keep = ms.aux_struct(aux)
    return ctx.L.ms_aux_running(ctx.h, C.byref(s), fp, column)


def case_refusals(mk, field, N=16, w=4):
    p, E = MODULUS[field], EXT[field]
    rng = SplitMix64(5000 + field)
    rows = rand_trace(rng, p, N, w)
    fr = rand_fractions(rng, p, E, 2, w)
    aux = ms.flatten_aux(PRODUCT, fr, E)
    want_col, want_final = rx.running(field, E, PRODUCT, fr, rows)
    u32 = lambda v: np.array(v, dtype=np.uint32)   # noqa: E731
    ctx = mk(field, fresh=True)
    assert raw_aux(ctx, aux) == ERR_STATE                                          # no committed trace
    commit_trace(ctx, rows)

    def arg(**over):
        assert raw_aux(ctx, dict(aux, **over)) == ERR_ARG, sorted(over)
        assert ctx.aux_count() == 0

    def arr(name, at, value):
        b = aux[name].copy()
        b[at] = value
        return {name: b}
    assert raw_aux(ctx, None) == ERR_ARG                                           # null program
    assert raw_aux(ctx, aux, final=None) == ERR_ARG                                # null final_out (column_out may be null: every other call here)
    for name, _t in ms._native.AUX_ARRAYS:
        arg(**{name: None})
    arg(op=2)
    arg(ext=3)
    arg(ext=E + 1)
    arg(ext=0)
    arg(nfrac=0)
    arg(nfrac=5, form_begin=u32([0] * 11), form_const=np.zeros(10 * E, dtype=np.uint64))
    arg(**arr("form_begin", 0, 1))                                                 # malformed form_begin
    arg(**arr("form_begin", 2, int(aux["form_begin"][1]) - 1))
    arg(form_begin=u32([0, 17, 17, 17, 17]), term_col=u32([0] * 17), term_coef=np.ones(17 * E, dtype=np.uint64))      # 17 terms in a form
    ok16 = dict(aux, form_begin=u32([0, 16, 16, 16, 16]), term_col=u32([0] * 16), term_coef=np.ones(16 * E, dtype=np.uint64))
    arg(**arr("term_col", 0, w))                                                   # a column >= w
    arg(**arr("term_coef", 1, p))                                                  # a non-canonical limb
    arg(**arr("form_const", 2, p))
    # none of it left a trace: the stage runs, and gives what the restatement gives; 16 terms in a form are allowed
    rc, final, col = ctx.aux_running(PRODUCT, fr, E, read=True)
    assert rc == 0 and tuple(final) == want_final and as_tuples(col) == want_col and ctx.aux_count() == E
    assert raw_aux(ctx, ok16) in (0, ERR_SHAPE) and ctx.aux_count() in (E, 2 * E)
    # more than 16 limb columns in all
    while ctx.aux_count() + E <= 16:
        assert raw_aux(ctx, aux) == 0
    n = ctx.aux_count()
    assert raw_aux(ctx, aux) == ERR_ARG and ctx.aux_count() == n
    assert ctx.interpolate() == 0 and ctx.polys_count() == w + n
    assert raw_aux(ctx, aux) == ERR_STATE                                          # ms_interpolate already called for this trace
    assert [int(v) for v in ctx.poly_read(w + n - E)] == pyref.dft(field, [z[0] for z in want_col], inverse=True)   # (the last accepted call's column)


def case_zero_denominator(mk, field, N=16, w=3):
    """ext = 1 with gamma = -T_1[3], and ext = E with the same base-field gamma embedded: MS_ERR_SHAPE, the count unchanged, and the next valid call gives the
    column a fresh context gives"""
    p, E = MODULUS[field], EXT[field]
    rng = SplitMix64(5500 + field)
    rows = rand_trace(rng, p, N, w)
    good = rand_fractions(rng, p, E, 1, w)
    want_col, want_final = rx.running(field, E, SUM, good, rows)
    ctx = mk(field, fresh=True)
    commit_trace(ctx, rows)
    gamma = (-rows[3][1]) % p
    for ext in (1, E):
        bad = [((k_of(ext, 1), []), (k_of(ext, gamma), [(1, k_of(ext, 1))])), ((k_of(ext, 5), [(0, k_of(ext, 3))]), (k_of(ext, 7), [(2, k_of(ext, 1))]))]
        assert all((7 + r[2]) % p for r in rows)                                   # (the second denominator vanishes nowhere)
        for op in (SUM, PRODUCT):
            rc, _, _ = ctx.aux_running(op, bad, ext)
            assert rc == ERR_SHAPE and ctx.aux_count() == 0 and ctx.last_error()
    rc, final, col = ctx.aux_running(SUM, good, E, read=True)
    assert rc == 0 and tuple(final) == want_final and as_tuples(col) == want_col and ctx.aux_count() == E
    fresh = mk(field, fresh=True)
    commit_trace(fresh, rows)
    rc, final2, col2 = fresh.aux_running(SUM, good, E, read=True)
    assert rc == 0 and final2 == final and col2.tolist() == col.tolist()


# ---------------------------------------------------------------- 6. emulation build only
def case_alloc_failures(mk, field, lib, N=512, w=3):
    """Every allocation the stage makes fails in turn (ms_emu_fail_alloc_after): a negative status, the count unchanged, and the same context then gives the clean
    result.  N = 512 with 256-row tiles: all three launches."""
    p, E = MODULUS[field], EXT[field]
    lib.ms_emu_alloc_count.restype = C.c_long
    lib.ms_emu_fail_alloc_after.argtypes = [C.c_long]
    rng = SplitMix64(6000 + field)
    rows = rand_trace(rng, p, N, w)
    fr = rand_fractions(rng, p, E, 2, w)
    with tile_env(256):
        ctx = mk(field, fresh=True)
    commit_trace(ctx, rows)
    rc, final, col = ctx.aux_running(PRODUCT, fr, E, read=True)       # (the first call sizes the buffers)
    assert rc == 0 and rx.check_recurrence(field, E, PRODUCT, fr, rows, as_tuples(col), tuple(final))
    commit_trace(ctx, rows)
    n0 = lib.ms_emu_alloc_count()
    assert ctx.aux_running(PRODUCT, fr, E, read=True)[0] == 0
    total = lib.ms_emu_alloc_count() - n0
    assert total >= 4                                                   # the emulated launches' LDS, at the least
    for k in range(total):
        commit_trace(ctx, rows)
        lib.ms_emu_fail_alloc_after(k)
        rc, _, _ = ctx.aux_running(PRODUCT, fr, E, read=True)
        lib.ms_emu_fail_alloc_after(-1)
        assert rc in (ms.ERR_NOMEM, ms.ERR_HIP), (k, rc)
        assert ctx.last_error() and ctx.aux_count() == 0
        rc, final2, col2 = ctx.aux_running(PRODUCT, fr, E, read=True)
        assert rc == 0 and final2 == final and col2.tolist() == col.tolist() and ctx.aux_count() == E, k
    assert fibonacci_proof(ctx, field) == fibonacci_proof(mk(field, fresh=True), field)


def case_sharded_refused(make_ctx, field, N=16, w=3):
    """a context with sharding on (here: a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses the stage"""
    from mini_stark_amd.dist import LocalShard
    p = MODULUS[field]
    rng = SplitMix64(6500 + field)
    rows = rand_trace(rng, p, N, w)
    ctx = make_ctx(field)
    sh = LocalShard(ctx, 32 * N * 4 + (4 << 20))
    commit_trace(ctx, rows)
    rc, _, _ = ctx.aux_running(SUM, rand_fractions(rng, p, 1, 1, w), 1)
    assert rc == ERR_STATE and ctx.aux_count() == 0
    sh.close()
