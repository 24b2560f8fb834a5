"""Directed inputs through the transform kernels, shared by tests/test_ntt_directed_emu.py and tests/test_ntt_directed_gpu.py: ms_ntt and ms_coset_lde on vectors
whose VALUES sit on the corners of the field arithmetic (tests/arith_cases.py has the operations one by one; here they run inside every NTT tile, where the
butterflies take sums and differences of edge values and multiply them by twiddles), against oracle.ntt / intt / coset_lde at every size, tests/pyref.py at
small sizes and closed forms computed with Python's pow: impulse -> character, constant -> scaled impulse, character -> impulse.

Families per field and size (c over 1, 2^32 - 1 mod p, p - 1): constants c; impulses c delta_j, j in {0, 1, 5, n/2, n-1}; alternating (c, 0); characters c w^(k i),
k in {1, 3, n/2 + 1}; antipodal x[i + n/2] = p - x[i]; x[i + n/2] = 2^64 - x[i] mod p (half sums on the wrap of a 64-bit word); the cycle
x[i] = edge[(7 i + 13 (i >> 9)) mod len] through the edge set of arith_cases, and the same with stride 11.  From 2^18 points on only the four families that find a
missing correction (REDUCED): edge cycle, antipodal, half sums, one character.
`profiled` brackets runs with ms_profile_begin / _end, so that a test can assert which kernel instances its sizes reached (ntt_pass_variants)."""
import concurrent.futures
import ctypes as C
import functools
import json
import re

import numpy as np

import arith_cases as ac
import pyref
from common import MODULUS
from oracle import oracle as orc

REDUCED_FROM = 18      # log2 of the transform size from which only REDUCED runs
REDUCED = ("edge cycle 7", "antipodal", "half sums 2^64", "character k=3 c=p-1")


def edge(field):
    return ac.gl_edge() if field == 0 else ac.bb_edge()


def coefs(field):
    p = MODULUS[field]
    return (("1", 1), ("2^32-1", (2**32 - 1) % p), ("p-1", p - 1))


@functools.lru_cache(None)
def powers(field, n, k):
    """w_n^(k i), i < n, as an object array of Python integers (by doubling)"""
    p = MODULUS[field]
    w = pow(pyref.root_of_unity(field, n), k, p)
    a = np.array([1], dtype=object)
    while len(a) < n:
        a = np.concatenate([a, a * pow(w, len(a), p) % p])
    return a


def edge_cycle(field, n, stride):
    e = edge(field)
    i = np.arange(n, dtype=np.int64)
    return np.array(e, dtype=np.uint64)[(stride * i + 13 * (i >> 9)) % len(e)]


@functools.lru_cache(None)
def families(field, log_n, reduced):
    """[(name, vector)] of the size; every vector canonical"""
    p, n = MODULUS[field], 1 << log_n
    out = []
    for cn, c in coefs(field):
        out.append((f"constant c={cn}", np.full(n, c, dtype=np.uint64)))
        for j in sorted({0, 1 % n, 5 % n, n // 2, n - 1}):
            v = np.zeros(n, dtype=np.uint64); v[j] = c
            out.append((f"impulse j={j} c={cn}", v))
        v = np.zeros(n, dtype=np.uint64); v[0::2] = c
        out.append((f"alternating c={cn}", v))
        for k in (1, 3, n // 2 + 1):
            out.append((f"character k={k} c={cn}", (powers(field, n, k % n) * c % p).astype(np.uint64)))
    h = n // 2
    half = [int(x) for x in edge_cycle(field, h, 7)]
    out.append(("antipodal", np.array(half + [(p - x) % p for x in half], dtype=np.uint64)))
    out.append(("half sums 2^64", np.array(half + [(2**64 - x) % p for x in half], dtype=np.uint64)))
    out.append(("edge cycle 7", edge_cycle(field, n, 7)))
    out.append(("edge cycle 11", edge_cycle(field, n, 11)))
    if reduced:
        out = [(name, v) for name, v in out if name in REDUCED]
        assert len(out) == len(REDUCED)
    return tuple(out)


def oracle_map(f, vectors):
    """f over the vectors on a few threads: the oracle's transforms are plain functions of their arguments and run outside the interpreter's lock"""
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        return np.stack(list(ex.map(f, vectors)))


def is_reduced(log_size):
    return log_size >= REDUCED_FROM


@functools.lru_cache(None)
def transform_refs(field, log_n):
    """(names, inputs, oracle.ntt of each, oracle.intt of each): computed once, shared by every context and build that runs the size, never written to"""
    fam = families(field, log_n, is_reduced(log_n))
    a = np.stack([v for _, v in fam])
    fwd = oracle_map(lambda v: orc.ntt(field, v), a)
    inv = oracle_map(lambda v: orc.intt(field, v), a)
    for x in (a, fwd, inv):
        x.setflags(write=False)
    return [name for name, _ in fam], a, fwd, inv


@functools.lru_cache(None)
def lde_refs(field, log_n, shift):
    fam = families(field, log_n, is_reduced(log_n + 3))
    a = np.stack([v for _, v in fam])
    out = oracle_map(lambda v: orc.coset_lde(field, v, shift, 8 << log_n), a)
    a.setflags(write=False); out.setflags(write=False)
    return [name for name, _ in fam], a, out


def same(got, want, names, what):
    for i, name in enumerate(names):
        bad = np.nonzero(got[i] != want[i])[0]
        assert len(bad) == 0, f"{what}, {name}: {len(bad)} of {got.shape[1]} outputs differ, first at {bad[0]}: got {int(got[i][bad[0]]):#x} want {int(want[i][bad[0]]):#x}"


def check_closed_forms(field, log_n, names, a, fwd, inv):
    """what the transforms of the structured families must be, from Python's pow alone (no oracle): applied to the OUTPUT OF THE LIBRARY"""
    p, n = MODULUS[field], 1 << log_n
    cs = dict(coefs(field))
    ninv = pow(n, p - 2, p)
    for i, name in enumerate(names):
        kind = name.split(" ")[0]
        if kind not in ("constant", "impulse", "character"):
            continue
        c = cs[name.split("c=")[1]]
        if kind == "constant":       # -> n c delta_0 ; inverse: c delta_0
            wf = np.zeros(n, dtype=np.uint64); wf[0] = n * c % p
            wi = np.zeros(n, dtype=np.uint64); wi[0] = c
        elif kind == "character":    # c w^(k i) -> n c delta_(-k) ; inverse: c delta_k
            k = int(name.split("k=")[1].split(" ")[0]) % n
            wf = np.zeros(n, dtype=np.uint64); wf[(n - k) % n] = n * c % p
            wi = np.zeros(n, dtype=np.uint64); wi[k] = c
        else:                        # c delta_j -> c w^(i j) ; inverse: c / n w^(-i j)
            j = int(name.split("j=")[1].split(" ")[0])
            if log_n > 14 and j not in (1, n - 1):
                continue
            wf = (powers(field, n, j) * c % p).astype(np.uint64)
            wi = (powers(field, n, (n - j) % n) * (c * ninv % p) % p).astype(np.uint64)
        assert (fwd[i] == wf).all(), f"closed form, forward, {name}, 2^{log_n}"
        assert (inv[i] == wi).all(), f"closed form, inverse, {name}, 2^{log_n}"


def case_transform(ctx, field, log_n):
    """forward, inverse and round trip of every family of the size in one batch"""
    names, a, want_f, want_i = transform_refs(field, log_n)
    rc, fwd = ctx.ntt(a)
    assert rc == 0, ctx.last_error()
    same(fwd, want_f, names, f"field {field} forward 2^{log_n}")
    rc, inv = ctx.ntt(a, inverse=True)
    assert rc == 0, ctx.last_error()
    same(inv, want_i, names, f"field {field} inverse 2^{log_n}")
    rc, back = ctx.ntt(fwd, inverse=True)
    assert rc == 0, ctx.last_error()
    same(back, a, names, f"field {field} round trip 2^{log_n}")
    check_closed_forms(field, log_n, names, a, fwd, inv)
    if log_n <= 10:      # the definition itself, O(n^2): every family up to 2^5, the value-driven ones at 2^10
        for i, name in enumerate(names):
            if log_n <= 5 or name in REDUCED[:3]:
                v = [int(x) for x in a[i]]
                assert [int(x) for x in fwd[i]] == pyref.dft(field, v), (name, log_n)
                if log_n <= 5:
                    assert [int(x) for x in inv[i]] == pyref.dft(field, v, inverse=True), (name, log_n)


def case_lde(ctx, field, log_n):
    """the families as COEFFICIENTS, evaluated on shift <w_(8 n)> for shift 1 (no scaling), 7 and p - 1 (every odd coefficient negated)"""
    p = MODULUS[field]
    for shift in (1, 7, p - 1):
        names, a, want = lde_refs(field, log_n, shift)
        rc, out = ctx.coset_lde(a, shift, 8 << log_n)
        assert rc == 0, ctx.last_error()
        same(out, want, names, f"field {field} lde 2^{log_n} x 8 shift {shift}")
        if log_n <= 3:
            for i in range(len(names)):
                assert [int(x) for x in out[i]] == pyref.coset_eval(field, [int(x) for x in a[i]], shift, 8 << log_n), (names[i], shift)


def profiled(ctx, run):
    """runs `run()` between ms_profile_begin and ms_profile_end: {NTT pass kernel instance: launches}"""
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    buf = C.create_string_buffer(1 << 17)
    try:
        run()
    finally:
        rc = ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf)))
    assert rc == 0
    return {k: v["launches"] for k, v in json.loads(buf.value.decode())["ntt_pass_variants"].items()}


def reached(variants, prefix):
    return sum(n for name, n in variants.items() if name.startswith(prefix))


def merge(into, variants):
    for k, v in variants.items():
        into[k] = into.get(k, 0) + v
    return into


# ---------------------------------------------------------------- sizes, and the kernel instance each was chosen to select
# (regular expressions on the instance names of ntt_pass_variants = the kernel names a profiler reports; %s: false = forward, true = inverse)
NTT_SIZES = {0: {3: r"msntt::PassKernel<GL, %s, 256>", 5: r"msntt::PassKernel<GL, %s, 256>", 10: r"msntt::PassKernel<GL, %s, 256>",      # single pass
                 11: r"msntt::PassKernelK<GL, %s, 6, 256>", 13: r"msntt::PassKernelK<GL, %s, 7, 256>",                                     # round-1 two-pass
                 14: r"msntt::PassKernel2<GL, GLT, %s, 7, 3, 256, 2, [01]>",                                                              # sign-bit class, two sub-rounds
                 16: r"msntt::PassKernel2<GL, GLM, %s, 8, 3, 256, 3, [01]>", 18: r"msntt::PassKernel2<GL, GLM, %s, 9, 3, 512, 3, [01]>",  # exec-masked class, three sub-rounds
                 20: r"msntt::PassKernel2<GL, GLM, %s, 10, 3, 512, 3, [01]>"},
             1: {3: r"msntt::PassKernel<BB, %s, 256>", 10: r"msntt::PassKernel<BB, %s, 256>", 13: r"msntt::PassKernelK<BB, %s, 7, 256>",
                 14: r"msntt::PassKernel2<BB, BB, %s, 7, 4, 256, 2, [01]>", 16: r"msntt::PassKernel2<BB, BB, %s, 8, 4, 256, 2, [01]>",
                 20: r"msntt::PassKernel2<BB, BB, %s, 10, 4, 512, 3, [01]>"}}
# coefficients -> blowup 8: 2^14, 2^15, 2^16 are the instances behind the virtual zero-padding pass (mode 2)
LDE_SIZES = {0: {3: r"msntt::PassKernel<GL, false, 256>", 5: r"msntt::PassKernel<GL, false, 256>", 10: r"msntt::PassKernel<GL, false, 512>", 11: r"msntt::PassKernel<GL, false, 512>",
                 14: r"msntt::PassKernel2<GL, GLT, false, 7, 3, 256, 2, 2>", 15: r"msntt::PassKernel2<GL, GLM, false, 8, 3, 256, 3, 2>", 16: r"msntt::PassKernel2<GL, GLM, false, 8, 3, 256, 3, 2>"},
             1: {3: r"msntt::PassKernel<BB, false, 256>", 10: r"msntt::PassKernel<BB, false, 512>",
                 14: r"msntt::PassKernel2<BB, BB, false, 7, 3, 256, 2, 2>", 16: r"msntt::PassKernel2<BB, BB, false, 8, 3, 256, 2, 2>"}}
# MS_NTT_V2_REGPASS=2 (+ MS_NTT_V2=2: BabyBear too) on fresh contexts: 2^7 x 2^7 tiles and the last 2^K points of every output in registers
REG_NTT_SIZES = (15, 16, 17, 18, 19)                    # K = 1 .. 5
REG_LDE_SIZES = {12: 0, 14: 0, 15: 1, 16: 2}            # coefficients -> K of the register pass behind the virtual pass (0: the plan has none at this size)


def arith_name(field):
    return "GL, GLM" if field == 0 else "BB, BB"


def assert_reached(variants, pattern):
    assert any(re.fullmatch(pattern, name) and n > 0 for name, n in variants.items()), f"no launch of {pattern} among {sorted(variants)}"


def case_transform_reaches(ctx, field, log_n, pattern):
    """the directed transforms of one size, and the kernel instance the size stands for: a plan change that moves the size elsewhere fails here"""
    v = profiled(ctx, lambda: case_transform(ctx, field, log_n))
    for inv in ("false", "true"):
        assert_reached(v, pattern % inv)
    return v


def case_lde_reaches(ctx, field, log_n, pattern):
    v = profiled(ctx, lambda: case_lde(ctx, field, log_n))
    assert_reached(v, pattern)
    return v


def case_register_pass_transform(mk_fresh, field, log_n):
    """random (parity_cases.case_ntt) and directed input through RegPassKernel<.., K = log_n - 14>, forward and inverse, on a context created under the test knobs"""
    import parity_cases as pc
    ctx = mk_fresh(field)
    v = profiled(ctx, lambda: (pc.case_ntt(lambda f, fresh=False: ctx, field, log_n, batch=1), case_transform(ctx, field, log_n)))
    for inv in ("false", "true"):
        assert_reached(v, r"msntt::RegPassKernel<%s, %s, %d>" % (arith_name(field), inv, log_n - 14))
    if field == 0:
        assert_reached(v, r"msntt::PassKernel2<GL, GLT, (false|true), 7, 3, 256, 2, [01]>")
    return v


def case_register_pass_lde(mk_fresh, field, log_n):
    import parity_cases as pc
    ctx = mk_fresh(field)
    v = profiled(ctx, lambda: (pc.case_coset_lde(lambda f, fresh=False: ctx, field, log_n, 8), case_lde(ctx, field, log_n)))
    if REG_LDE_SIZES[log_n]:
        assert_reached(v, r"msntt::RegPassKernel<%s, false, %d>" % (arith_name(field), REG_LDE_SIZES[log_n]))
    return v
