"""Cases of ms_mix_air_ext (build-defined: ms_mix_air with the combiner r in the extension K; include/ministark.h), shared by the emulation suite
(tests/test_air_ext_emu.py) and the GPU suite (tests/test_air_ext_gpu.py).  The stage is held to the restatement of its definition (tests/pyref_air_ext.py:
pyref_air's unscaled per-constraint quotients combined with the Tower powers of r), to bit-equality with ms_mix_air for a base-field r, and to the defining
formula evaluated in Tower arithmetic at out-of-domain points of K.  `mk(field, fresh=True)` returns a new mini_stark_amd.Context."""
import ctypes as C
import json

import numpy as np

import mini_stark_amd as ms
import air_cases as ac
import pyref_air as ra
import pyref_air_ext as rx
from common import MODULUS, EXT, SplitMix64
from mini_stark_amd.host import air_expected_validity, air_expected_validity_ext
from terms_cases import commit, omega_of, trace_polys

ERR_SHAPE, ERR_STATE, ERR_ARG = ms.ERR_SHAPE, ms.ERR_STATE, ms.ERR_ARG
SPECS = ac.SPECS
validity_len_of = ac.validity_len_of


def lists(sp, **over):
    a = dict(sp, **over)
    return a["cons"], a["exempt"], a["periodic"], a["boundary"]


def mix_ext(ctx, r, sp, **over):
    return ctx.mix_air_ext(r, *lists(sp, **over))


def full_r(rng, field):
    """a combiner with every limb non-zero"""
    return tuple(rng.nonzero(MODULUS[field]) for _ in range(EXT[field]))


def want_validity(field, omega, N, polys, r, sp, **over):
    cons, exempt, periodic, boundary = lists(sp, **over)
    VL = ra.validity_len(N, cons, exempt, len(boundary))
    return VL, rx.validity(field, omega, N, polys, r, cons, exempt, periodic, boundary, VL)


def trimmed(val):
    return max((i + 1 for i, c in enumerate(val) if any(c)), default=0)


def run_fri(ctx, field, rng, blowup, VL, nc):
    """the whole FRI over the validity polynomial with challenges from rng; returns (root0, round-0 info, roots, MSFP bytes)"""
    p, e = MODULUS[field], EXT[field]
    rounds = (VL * blowup).bit_length() - 1
    rc, root0 = ctx.fri_begin(blowup, rounds)
    assert rc == 0, ctx.last_error()
    info = ctx.fri_round_info(0)
    D = 1
    while D < nc * blowup:
        D *= 2
    assert info == (nc, D)
    poly0 = ctx.fri_round_poly(0)
    roots = []
    for _ in range(1, rounds):
        rc, B = ctx.fri_deep([rng.field(p) for _ in range(e)])
        assert rc == 0
        rc, root = ctx.fri_fold_commit([rng.field(p) for _ in range(e)])
        assert rc == 0, ctx.last_error()
        roots.append((B.tolist(), root))
    rc, proof = ctx.fri_query([rng.next(), 5])
    assert rc == 0 and len(proof) > 0
    return root0, info, poly0, roots, proof


def profiled(ctx, stage):
    """(status, launches of air_inv, of mix_air, of mix_air_ext) of `stage` between ms_profile_begin and ms_profile_end"""
    buf = C.create_string_buffer(1 << 15)
    assert ctx.L.ms_profile_begin(ctx.h) == 0
    rc = stage()
    assert ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))) == 0
    prof = json.loads(buf.value.decode())
    return rc, prof["air_inv"]["launches"], prof["mix_air"]["launches"], prof["mix_air_ext"]["launches"]


# ---------------------------------------------------------------- 1. the definition, coefficient for coefficient
def case_definition(mk, field, name, blowup, N=16):
    p, e = MODULUS[field], EXT[field]
    sp = SPECS[name](field, N)
    ctx = mk(field, fresh=True)
    rng = SplitMix64(1400 + blowup)
    omega = omega_of(ctx, field, N)
    commit(ctx, sp["trace"], blowup, rng.nonzero(p))
    polys = trace_polys(field, omega, sp["trace"])
    r = full_r(rng, field)
    # A program of ONE constraint and no boundary constraint (scattered, selector) has the single weight r^0 = 1: by the definition its limbs above limb 0 are
    # zero, whatever r.  Such a spec runs as it is (the zero planes asserted) and again with its constraint listed E times (weights 1, r, .., r^(E-1)), so that
    # every row of the table also runs with every limb plane live.
    single = len(sp["cons"]) + len(sp["boundary"]) == 1
    variants = [{}, {"cons": sp["cons"] * e, "exempt": sp["exempt"] * e}] if single else [{}]
    for over in variants:
        VL, want = want_validity(field, omega, N, polys, r, sp, **over)
        for l in range(e):
            live = any(c[l] for c in want)
            assert live == (l == 0 or not single or bool(over)), l          # every limb plane is live: a dropped limb cannot pass
        assert mix_ext(ctx, r, sp, **over) == 0, ctx.last_error()
        assert validity_len_of(ctx) == VL and ctx.validity_ext() == e
        v = ctx.validity_read()
        assert v.shape == (VL, e)
        assert [tuple(int(x) for x in row) for row in v] == want


# ---------------------------------------------------------------- 2. a base-field r reproduces ms_mix_air bit for bit
def case_base_r(mk, field, name, log_n, blowup, full_fri):
    from pyref import Tower
    p, e = MODULUS[field], EXT[field]
    N = 1 << log_n
    sp = SPECS[name](field, N)
    rng = SplitMix64(1431 + log_n)
    shift, r0 = rng.nonzero(p), rng.nonzero(p)
    T = Tower(field, e)
    z = tuple(rng.field(p) for _ in range(e))
    seed = rng.next()
    outs = []
    for which in ("air", "ext"):
        ctx = mk(field, fresh=True)
        commit(ctx, sp["trace"], blowup, shift)
        if which == "air":
            assert ac.mix(ctx, r0, sp) == 0, ctx.last_error()
            assert ctx.validity_ext() == 1
            val = [int(x) for x in ctx.validity_read()]
        else:
            assert mix_ext(ctx, (r0,) + (0,) * (e - 1), sp) == 0, ctx.last_error()
            assert ctx.validity_ext() == e
            v = ctx.validity_read()
            assert v.shape[1] == e and not v[:, 1:].any()          # the limbs above limb 0 are zero
            val = [int(x) for x in v[:, 0]]
        VL = validity_len_of(ctx)
        assert len(val) == VL and any(val)
        wz = T.mul(z, T.from_base(omega_of(ctx, field, N)))
        rc, ev = ctx.eval_ext(np.array([z, wz], dtype=np.uint64))
        assert rc == 0
        out = [VL, val, ev.tolist()]
        if full_fri:
            nc = max(i + 1 for i, c in enumerate(val) if c)
            root0, info, poly0, roots, proof = run_fri(ctx, field, SplitMix64(seed), blowup, VL, nc)
            out += [root0, info, poly0.tolist(), roots, proof]
        else:
            rc, root0 = ctx.fri_begin(blowup, (VL * blowup).bit_length() - 1)
            assert rc == 0, ctx.last_error()
            out += [root0, ctx.fri_round_info(0)]
        outs.append(out)
    assert outs[0] == outs[1]


# ---------------------------------------------------------------- 3. the definition at out-of-domain points of K
def case_identity(mk, field, name, log_n, blowup):
    """validity(z) = the defining formula's right-hand side at two random z in K: the left side by Horner over the K-valued validity_read, the right side from the
    poly_read columns in Tower arithmetic with inverses in K.  Both sides multiplied out are polynomials of degree < 4N over K: a false accept at one point has
    probability below 4N / |K|."""
    p, e = MODULUS[field], EXT[field]
    N = 1 << log_n
    sp = SPECS[name](field, N)
    ctx = mk(field, fresh=True)
    rng = SplitMix64(1500 + log_n)
    omega = omega_of(ctx, field, N)
    commit(ctx, sp["trace"], blowup, rng.nonzero(p))
    r = full_r(rng, field)
    assert mix_ext(ctx, r, sp) == 0, ctx.last_error()
    polys = [[int(v) for v in ctx.poly_read(j)] for j in range(sp["trace"].shape[1])]
    v = ctx.validity_read()
    cons, exempt, periodic, boundary = lists(sp)
    assert v.shape == (ra.validity_len(N, cons, exempt, len(boundary)), e) and all(v[:, l].any() for l in range(e))
    val = [tuple(int(x) for x in row) for row in v]
    T = rx.tower(field)
    for _ in range(2):
        z = tuple(rng.field(p) for _ in range(e))
        assert any(z[1:])
        assert rx.horner_ext(T, val, z) == rx.rhs_at(field, omega, N, polys, r, cons, exempt, periodic, boundary, z)


# ---------------------------------------------------------------- 4. DEEP-ALI, the host function, a full FRI
def case_deep_and_fri(mk, field, name, blowup, N=16):
    p, e = MODULUS[field], EXT[field]
    sp = SPECS[name](field, N)
    w = sp["trace"].shape[1]
    ctx = mk(field, fresh=True)
    rng = SplitMix64(1600 + blowup)
    omega = omega_of(ctx, field, N)
    commit(ctx, sp["trace"], blowup, rng.nonzero(p))
    r = full_r(rng, field)
    assert mix_ext(ctx, r, sp) == 0, ctx.last_error()
    cons, exempt, periodic, boundary = lists(sp)
    VL = ra.validity_len(N, cons, exempt, len(boundary))
    T = rx.tower(field)
    z = tuple(rng.field(p) for _ in range(e))
    used = ms.air_rows(cons, boundary)
    rows = sorted(set(used) | {2})
    pts = [T.mul(z, T.from_base(pow(omega, k, p))) for k in rows]
    rc, ev = ctx.eval_ext(np.array(pts, dtype=np.uint64))
    assert rc == 0
    assert ev.shape == (len(rows), w + 1, e)
    vz = [int(x) for x in ev[0][w]]
    # the constraint polynomials' values are untouched by the validity polynomial's own launch
    polys = [[int(v) for v in ctx.poly_read(j)] for j in range(w)]
    for k in range(len(rows)):
        for j in range(w):
            assert tuple(int(x) for x in ev[k][j]) == rx.horner_base(T, polys[j], pts[k])
    rc, want = air_expected_validity_ext(field, r, (cons, exempt, periodic, boundary), N, z, rows, ev)
    assert rc == 0 and [int(x) for x in want] == vz
    assert tuple(vz) == rx.rhs_at(field, omega, N, polys, r, cons, exempt, periodic, boundary, z)
    val = [tuple(int(x) for x in row) for row in ctx.validity_read()]
    assert tuple(vz) == rx.horner_ext(T, val, z)
    # the other rows' values are Horner over the K-valued polynomial too
    for k in range(1, len(rows)):
        assert tuple(int(x) for x in ev[k][w]) == rx.horner_ext(T, val, pts[k])
    # a changed boundary value moves the expected value; so does a changed limb of r; a base-field r gives the base-field entry's value
    poly, row, value = boundary[-1]
    rc, other = air_expected_validity_ext(field, r, (cons, exempt, periodic, boundary[:-1] + [(poly, row, (value + 1) % p)]), N, z, rows, ev)
    assert rc == 0 and [int(x) for x in other] != vz
    r2 = r[:-1] + ((r[-1] + 1) % p,)
    rc, other = air_expected_validity_ext(field, r2, (cons, exempt, periodic, boundary), N, z, rows, ev)
    assert rc == 0 and [int(x) for x in other] != vz
    rc, a = air_expected_validity_ext(field, (r[0],) + (0,) * (e - 1), (cons, exempt, periodic, boundary), N, z, rows, ev)
    rc2, b = air_expected_validity(field, r[0], (cons, exempt, periodic, boundary), N, z, rows, ev)
    assert rc == 0 and rc2 == 0 and a.tolist() == b.tolist()
    rc, _ = air_expected_validity_ext(field, r[:-1] + (p,), (cons, exempt, periodic, boundary), N, z, rows, ev)
    assert rc == ERR_ARG
    # ---- a full FRI over the K-valued polynomial; round 0's polynomial is validity_read trimmed
    nc = trimmed(val)
    assert nc > 0
    _root0, _info, poly0, _roots, _proof = run_fri(ctx, field, rng, blowup, VL, nc)
    assert [tuple(int(x) for x in row) for row in poly0] == val[:nc]


# ---------------------------------------------------------------- 5. refusals and state
def raw_mix_air_ext(ctx, r, air):
    s, _keep = ms.air_struct(air)
    if r is None:
        return ctx.L.ms_mix_air_ext(ctx.h, None, C.byref(s))
    rr = np.ascontiguousarray(r, dtype=np.uint64)
    return ctx.L.ms_mix_air_ext(ctx.h, rr.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(s))


def case_refusals(mk, field, N=16, blowup=4):
    p, e = MODULUS[field], EXT[field]
    sp = SPECS["mimc"](field, N)
    air = ms.flatten_air(*lists(sp))
    ctx = mk(field, fresh=True)
    rng = SplitMix64(1066)
    r = full_r(rng, field)
    assert ctx.validity_ext() == 0
    rc, _ = ctx.trace_commit(sp["trace"], 2)
    assert rc == 0 and ctx.interpolate() == 0
    assert raw_mix_air_ext(ctx, r, air) == ERR_STATE                                # before ms_lde_commit
    assert ctx.validity_ext() == 0
    rc, _ = ctx.lde_commit(blowup, rng.nonzero(p), 2)
    assert rc == 0
    assert raw_mix_air_ext(ctx, None, air) == ERR_ARG                               # null r
    for l in range(e):
        assert raw_mix_air_ext(ctx, r[:l] + (p,) + r[l + 1:], air) == ERR_ARG      # a limb equal to p
    assert ctx.L.ms_mix_air_ext(ctx.h, np.ascontiguousarray(r, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)), None) == ERR_ARG   # null program
    assert raw_mix_air_ext(ctx, r, dict(air, coef=None)) == ERR_ARG                 # ms_mix_air's own conditions, through the shared validation
    assert ctx.validity_ext() == 0 and validity_len_of(ctx) == 0
    # none of it left a trace
    omega = omega_of(ctx, field, N)
    _, want = want_validity(field, omega, N, trace_polys(field, omega, sp["trace"]), r, sp)
    assert raw_mix_air_ext(ctx, r, air) == 0, ctx.last_error()
    assert [tuple(int(x) for x in row) for row in ctx.validity_read()] == want
    # ms_polys_* and ms_trace_commit clear it
    assert ctx.polys_lincomb([1], [0]) == 0
    assert ctx.validity_ext() == 0
    rc, _ = ctx.trace_commit(sp["trace"], 2)
    assert rc == 0 and ctx.validity_ext() == 0


def case_shape_refusal_then_both(mk, field, N=16, blowup=4):
    """a trace that breaks a constraint on a non-exempt row: MS_ERR_SHAPE; afterwards the same context runs ms_mix_air and ms_mix_air_ext correctly"""
    p, e = MODULUS[field], EXT[field]
    sc = SPECS["scattered"](field, N)
    rng = SplitMix64(1067)
    shift, r, r0 = rng.nonzero(p), full_r(rng, field), rng.nonzero(p)
    ctx = mk(field, fresh=True)
    omega = omega_of(ctx, field, N)
    polys = trace_polys(field, omega, sc["trace"])
    assert not ra.is_exact(p, omega, N, polys, 1, sc["cons"], [[3, N - 1]])
    commit(ctx, sc["trace"], blowup, shift)
    assert mix_ext(ctx, r, sc, exempt=[[3, N - 1]]) == ERR_SHAPE
    assert ctx.validity_ext() == 0
    _, want1 = ac.want_validity(field, omega, N, polys, r0, sc)
    assert ac.mix(ctx, r0, sc) == 0, ctx.last_error()
    assert ctx.validity_ext() == 1 and [int(v) for v in ctx.validity_read()] == want1
    assert mix_ext(ctx, r, sc, exempt=[[N // 2, N - 1]]) == ERR_SHAPE
    assert ctx.validity_ext() == 1 and [int(v) for v in ctx.validity_read()] == want1      # as if the call had not been made
    _, want = want_validity(field, omega, N, polys, r, sc)
    assert mix_ext(ctx, r, sc) == 0, ctx.last_error()
    assert ctx.validity_ext() == e and [tuple(int(x) for x in row) for row in ctx.validity_read()] == want
    # a wrong boundary value
    sp = SPECS["mimc"](field, N)
    poly, row, value = sp["boundary"][1]
    wrong = [sp["boundary"][0], (poly, row, (value + 1) % p), sp["boundary"][2]]
    ctx = mk(field, fresh=True)
    commit(ctx, sp["trace"], blowup, shift)
    assert mix_ext(ctx, r, sp, boundary=wrong) == ERR_SHAPE
    assert mix_ext(ctx, r, sp) == 0, ctx.last_error()
    # the LDE domain cannot decide exactness (d = 3 at blowup 2), as for ms_mix_air
    ctx = mk(field, fresh=True)
    commit(ctx, sp["trace"], 2, shift)
    assert ac.mix(ctx, r0, sp) == ERR_SHAPE and mix_ext(ctx, r, sp) == ERR_SHAPE


def case_switching(mk, field, N=16, blowup=4):
    """ms_mix_air_ext, ms_mix_air, ms_mix_air_ext on one LDE: each gives what a fresh context gives, ms_validity_ext follows (E, 1, E); ms_mix then puts it back to 1"""
    p, e = MODULUS[field], EXT[field]
    sp = SPECS["mimc"](field, N)
    rng = SplitMix64(1068)
    shift, r, r0 = rng.nonzero(p), full_r(rng, field), rng.nonzero(p)
    z = np.array([[rng.field(p) for _ in range(e)]], dtype=np.uint64)

    def state(ctx):
        rc, ev = ctx.eval_ext(z)
        assert rc == 0
        VL = validity_len_of(ctx)
        v = ctx.validity_read()
        rc, root0 = ctx.fri_begin(blowup, (VL * blowup).bit_length() - 1)
        assert rc == 0, ctx.last_error()
        return ctx.validity_ext(), VL, v.tolist(), ev.tolist(), root0, ctx.fri_round_info(0)
    fresh = []
    for which in ("ext", "air"):
        c = mk(field, fresh=True)
        commit(c, sp["trace"], blowup, shift)
        assert (mix_ext(c, r, sp) if which == "ext" else ac.mix(c, r0, sp)) == 0
        fresh.append(state(c))
    assert fresh[0][0] == e and fresh[1][0] == 1 and fresh[0][2] != fresh[1][2]
    ctx = mk(field, fresh=True)
    commit(ctx, sp["trace"], blowup, shift)
    assert mix_ext(ctx, r, sp) == 0 and state(ctx) == fresh[0]
    assert ac.mix(ctx, r0, sp) == 0 and state(ctx) == fresh[1]
    assert mix_ext(ctx, r, sp) == 0 and state(ctx) == fresh[0]
    assert ctx.mix(r0) == 0 and ctx.validity_ext() == 1 and validity_len_of(ctx) == N and ctx.validity_read().shape == (N,)
    rc, _ = ctx.fri_begin(blowup, 3)
    assert rc == 0, ctx.last_error()


def case_store_growth(mk, field, N=16, blowup=4):
    """VL = 2N on a context of 7 polynomials: the E * 2 slots of the K-valued polynomial do not fit the 8-polynomial store, which grows (and moves); the constraint
    polynomials are unchanged afterwards"""
    p, e = MODULUS[field], EXT[field]
    sp = SPECS["mimc"](field, N)
    rng = SplitMix64(1069)
    ctx = mk(field, fresh=True)
    omega = omega_of(ctx, field, N)
    commit(ctx, sp["trace"], blowup, rng.nonzero(p), lincombs=[([rng.field(p), rng.field(p)], [0, 1]) for _ in range(5)])
    assert ctx.polys_count() == 7 and 7 + 2 * e > 8
    before = [ctx.poly_read(j).tolist() for j in range(7)]
    r0 = rng.nonzero(p)
    assert ac.mix(ctx, r0, sp) == 0                       # an earlier base-field validity polynomial sits behind the constraint polynomials
    r = full_r(rng, field)
    VL, want = want_validity(field, omega, N, [[int(v) for v in c] for c in before], r, sp)
    assert VL == 2 * N
    assert mix_ext(ctx, r, sp) == 0, ctx.last_error()
    assert [tuple(int(x) for x in row) for row in ctx.validity_read()] == want
    assert [ctx.poly_read(j).tolist() for j in range(7)] == before
    assert [tuple(int(x) for x in row) for row in ctx.validity_read()] == want


def case_sharded_refused(make_ctx, field, N=16, blowup=4):
    """a context with sharding on (a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses the stage, whether or not its LDE is large enough to be sharded"""
    from mini_stark_amd.dist import LocalShard
    sp = SPECS["fib_bounded"](field, N)
    ctx = make_ctx(field)
    sh = LocalShard(ctx, 32 * N * blowup + (4 << 20))
    commit(ctx, sp["trace"], blowup, 3)
    assert mix_ext(ctx, (5,) + (1,) * (EXT[field] - 1), sp) == ERR_STATE
    assert ctx.validity_ext() == 0
    sh.close()


# ---------------------------------------------------------------- 6. one launch; the boundary inverse table is shared with ms_mix_air
def case_one_launch(mk, field, N=16, blowup=4):
    p = MODULUS[field]
    sp = SPECS["fib_bounded"](field, N)
    rng = SplitMix64(1700)
    r, r0 = full_r(rng, field), rng.nonzero(p)
    for first in ("ext", "air"):
        ctx = mk(field, fresh=True)
        commit(ctx, sp["trace"], blowup, rng.nonzero(p))
        built = 0
        for which in (first, "air" if first == "ext" else "ext", first):
            stage = (lambda: mix_ext(ctx, r, sp)) if which == "ext" else (lambda: ac.mix(ctx, r0, sp))
            rc, n_inv, n_air, n_ext = profiled(ctx, stage)
            assert rc == 0, ctx.last_error()
            assert (n_air, n_ext) == ((0, 1) if which == "ext" else (1, 0))
            built += n_inv
        assert built == 1                                  # built by whichever stage came first, found by the other
        rc, n_inv, n_air, n_ext = profiled(ctx, lambda: mix_ext(ctx, r, sp, boundary=[]))
        assert (rc, n_inv, n_air, n_ext) == (0, 0, 0, 1)
