"""Structured-input parity cases shared by the emulation suite (tests/test_structured_emu.py) and the GPU suite (tests/test_structured_gpu.py): proofs whose
validity polynomial is low-degree, sparse or zero, and proofs whose challenges sit on the edges of the field (0, 1, p - 1, domain points, zero limbs, repeated
queries) - the inputs on which the data-dependent parts of the prover (trimmed lengths, domain sizes derived from them, ragged even / odd halves, first-match
leaf lookup among duplicate codeword values) take another branch than on a Fibonacci or random trace with SplitMix64 challenges.  The library (HIP build, or the
emulation build of the same kernel code) against the CPU oracle: the same list of (stage, status, value), bit for bit.  tests/test_oracle.py pins the oracle to
tests/pyref.py on the same kind of input.  `mk(field)` returns a mini_stark_amd.Context."""
import ctypes as C
import functools
import json

import numpy as np

import parity_cases as pc
from common import MODULUS, EXT, SplitMix64, fibonacci_trace_fast, fibonacci_closures
from oracle import oracle as orc

# name -> support of every trace column's coefficient vector (N = rows)
SUPPORTS = {
    "zero": lambda N: [],
    "const": lambda N: [0],
    "deg1": lambda N: [0, 1],
    "len5": lambda N: list(range(5)),
    "len2049": lambda N: list(range(2049)),          # only where N > 2049: one coefficient more than a scan block
    "half+3": lambda N: list(range(N // 2 + 3)),
    "even": lambda N: list(range(0, N, 2)),
    "odd": lambda N: list(range(1, N, 2)),
    "mult4": lambda N: list(range(0, N, 4)),
    "lowhalf_even": lambda N: list(range(0, N // 2, 2)),
    "mono_top": lambda N: [N - 1],
    "mono_mid": lambda N: [N // 2],
    "gap": lambda N: [0, 1, 2, N // 2, N - 3],
}
MODES = ("random", "alpha0", "basez")
SHRINKS_UNDER_ALPHA0 = ("gap", "odd", "mono_top")        # alpha = 0 keeps the even half only: the next round is shorter than a generic fold leaves it
EVEN_IN_X = ("even", "mult4", "lowhalf_even")            # f(x) = f(-x): every query of window 0 opens two equal values
# the reduced list of the 2^11-row runs: (support, mode)
REDUCED = (("even", "random"), ("odd", "alpha0"), ("gap", "alpha0"), ("half+3", "random"), ("const", "random"), ("zero", "random"))
# 2^14 rows: a find-first launch of its own, tree levels above the subtree threshold, a multi-block degree kernel, a multi-level scan
LARGE = (("even", "random"), ("odd", "alpha0"), ("gap", "alpha0"), ("half+3", "random"), ("len2049", "random"))


def names_for(N):
    return [n for n in SUPPORTS if n != "len2049" or N > 2049]


def trace_from_support(field, N, support, seed, w=3):
    """Column c is the transform of a coefficient vector that is zero except at `support`, where it holds seeded non-zero field elements (another seed per column).
    The Fibonacci closures are linear combinations, so every constraint polynomial and the validity polynomial keep the support."""
    cols = []
    for c in range(w):
        coef = np.zeros(N, dtype=np.uint64)
        if len(support):
            v = pc.rand_field(field, (len(support),), seed=seed + 1000 * c)
            v[v == 0] = 1
            coef[np.asarray(support, dtype=np.int64)] = v
        cols.append(orc.ntt(field, coef))
    return np.ascontiguousarray(np.stack(cols, axis=1))


def E(field, *limbs):
    """zero-padding to the extension degree"""
    return [int(v) for v in limbs] + [0] * (EXT[field] - len(limbs))


def random_challenges(field, seed, mode="random", nq=2):
    """Every challenge of one proof, explicit: shift, r, the OOD points, per-round z and alpha (round i takes entry (i - 1) mod length), betas."""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(seed)
    ch = {"shift": rng.nonzero(p), "r": rng.field(p), "ood": [[rng.field(p) for _ in range(e)] for _ in range(2)]}
    ch["z"] = [[rng.field(p) for _ in range(e)] for _ in range(40)]
    ch["alpha"] = [[rng.field(p) for _ in range(e)] for _ in range(40)]
    ch["betas"] = [rng.next() for _ in range(nq)]
    if mode == "alpha0":
        ch["alpha"] = [[0] * e]
    elif mode == "basez":    # the kernels' evaluation-domain fold must fall back to the transform
        ch["z"] = [E(field, z[0]) for z in ch["z"]]
    else:
        assert mode == "random"
    return ch


def drive_explicit(sess, field, trace, blowup, rounds, ch, read_big=True):
    """parity_cases.drive with every challenge given (`ch`: random_challenges' keys) and every stage's status RECORDED: returns the list of
    (stage, status, value) up to and including the first non-zero status.  `sess` is an oracle Session or a mini_stark_amd Context."""
    N, w = trace.shape
    omega = orc.root_of_unity(field, N)
    out = []

    def step(name, rc, value=None):
        out.append((name, int(rc), value if rc == 0 else None))
        return rc == 0
    rc, root = sess.trace_commit(trace, 2 * w)
    if not step("trace_root", rc, root) or not step("interpolate", sess.interpolate()):
        return out
    for k, (sc, idx) in enumerate(fibonacci_closures(field, N, omega)):
        if not step(f"lincomb{k}", sess.polys_lincomb(sc, idx)):
            return out
    if read_big:
        for i in range(sess.polys_count()):
            step(f"poly{i}", 0, sess.poly_read(i).tolist())
    rc, root = sess.lde_commit(blowup, ch["shift"], 2 * w)
    if not step("lde_root", rc, root):
        return out
    if read_big:
        step("lde", 0, sess.lde_read().tolist())
    if not step("mix", sess.mix(ch["r"])):
        return out
    if read_big:
        step("validity", 0, sess.validity_read().tolist())
    rc, ev = sess.eval_ext(np.array(ch["ood"], dtype=np.uint64))
    if not step("ood", rc, ev.tolist()):
        return out
    rc, root = sess.fri_begin(blowup, rounds)
    if not step("fri_root0", rc, root):
        return out
    for i in range(1, rounds):
        rc, B = sess.fri_deep(ch["z"][(i - 1) % len(ch["z"])])
        if not step(f"B{i}", rc, B.tolist()):
            return out
        rc, root = sess.fri_fold_commit(ch["alpha"][(i - 1) % len(ch["alpha"])])
        if not step(f"fri_root{i}", rc, root):
            return out
    for i in range(rounds):
        step(f"round_info{i}", 0, tuple(sess.fri_round_info(i)))
        if read_big:
            step(f"round_poly{i}", 0, sess.fri_round_poly(i).tolist())
            step(f"round_cw{i}", 0, sess.fri_round_codeword(i).tolist())
    rc, proof = sess.fri_query(ch["betas"])
    step("fri_proof", rc, proof)
    return out


def compare(got, want, what=""):
    for (ka, sa, va), (kb, sb, vb) in zip(got, want):
        assert ka == kb, f"{what}: stage {ka} where the oracle is at {kb}"
        assert sa == sb, f"{what}: status {sa} of {ka}, the oracle's is {sb}"
        assert va == vb, f"{what}: stage output {ka} differs from the oracle's"
    assert len(got) == len(want), f"{what}: {len(got)} stages, the oracle has {len(want)}"


def oracle_round0(field, trace, blowup, r):
    """(ncoef, D) of FRI round 0 from the oracle: what the validity polynomial's trimmed length makes of the domain (fri.rs:74)"""
    N, w = trace.shape
    o = orc.Session(field)
    assert o.trace_commit(trace, 2 * w)[0] == 0 and o.interpolate() == 0
    for sc, idx in fibonacci_closures(field, N, orc.root_of_unity(field, N)):
        assert o.polys_lincomb(sc, idx) == 0
    assert o.mix(r) == 0 and o.fri_begin(blowup, 1)[0] == 0
    info = o.fri_round_info(0)
    o.close()
    return info


def window0_records(proof, e, nq):
    """The nq records of window 0 of an MSFP blob (include/ministark.h): (y1, y2, leaf index of path 1, leaf index of path 2)."""
    u = lambda off, n=1: list(np.frombuffer(proof, dtype="<u8", count=n, offset=off).astype(object))
    off, recs = 0, []
    for _ in range(nq):
        pts = u(off, 6 * e)
        off += 48 * e
        qlen = u(off)[0]
        off += 8 + 8 * e * qlen
        idx = []
        for _ in range(2):
            idx.append(u(off)[0])
            off += 8 + 16 * e
            off += 8 + 64 * u(off)[0]
        recs.append((pts[e:2 * e], pts[3 * e:4 * e], idx[0], idx[1]))
    return recs


@functools.lru_cache(maxsize=None)
def trace_of(field, log_n, name):
    N = 1 << log_n
    return trace_from_support(field, N, SUPPORTS[name](N), seed=7 * log_n + 100 * list(SUPPORTS).index(name) + field)


@functools.lru_cache(maxsize=None)
def oracle_structured(field, log_n, name, mode, blowup=8, read_big=True):
    """The oracle's side of one structured case, computed once and shared: (trace, challenges, rounds, stage list).  rounds = log2(D0) with D0 from the oracle's
    round 0, so that the query phase runs.  The preconditions are asserted here, on the oracle's outputs only: a case cannot quietly stop exercising what it is for."""
    N = 1 << log_n
    trace = trace_of(field, log_n, name)
    ch = random_challenges(field, seed=1 + 31 * log_n + 1000 * list(SUPPORTS).index(name) + 7 * MODES.index(mode) + field, mode=mode)
    nc0, D0 = oracle_round0(field, trace, blowup, ch["r"])
    ch["betas"] += [0, 1, 3, D0 // 2, D0 - 1, D0, D0 + 1, 2 * N * blowup]
    rounds = D0.bit_length() - 1
    want = drive_explicit(orc.Session(field), field, trace, blowup, rounds, ch, read_big=read_big)
    assert all(s == 0 for _, s, _ in want) and want[-1][0] == "fri_proof", [(k, s) for k, s, _ in want if s]
    o = {k: v for k, _, v in want}
    support = SUPPORTS[name](N)
    ncoef = [o[f"round_info{i}"][0] for i in range(rounds)]
    assert o["round_info0"] == (nc0, D0) and nc0 == (max(support) + 1 if support else 0), (name, o["round_info0"])
    assert [o[f"round_info{i}"][1] for i in range(rounds)] == [D0 >> i for i in range(rounds)]
    if mode == "alpha0" and name in SHRINKS_UNDER_ALPHA0:
        assert any(ncoef[i + 1] < (ncoef[i] + 1) // 2 - 1 for i in range(rounds - 1)), (name, ncoef)
    if name in EVEN_IN_X:
        recs = window0_records(o["fri_proof"], EXT[field], len(ch["betas"]))
        assert all(y1 == y2 and i1 == i2 for y1, y2, i1, i2 in recs), (name, recs)
    return trace, ch, rounds, want


def case_structured(ctx, field, log_n, name, mode, blowup=8, read_big=True):
    trace, ch, rounds, want = oracle_structured(field, log_n, name, mode, blowup, read_big)
    got = drive_explicit(ctx, field, trace, blowup, rounds, ch, read_big=read_big)
    compare(got, want, f"field {field}, 2^{log_n} rows, support {name}, {mode}")


@functools.lru_cache(maxsize=None)
def oracle_generic(field, log_n, blowup=8):
    trace = fibonacci_trace_fast(field, 1 << log_n)
    return trace, pc.drive(orc.Session(field), field, trace, blowup, 2, seed=77, read_big=False)


def case_generic(ctx, field, log_n, blowup=8):
    """parity_cases.case_prove without the big read-backs, the oracle's side computed once: the generic proof between two structured ones on the same context"""
    trace, want = oracle_generic(field, log_n, blowup)
    got = pc.drive(ctx, field, trace, blowup, 2, seed=77, read_big=False)
    assert len(got) == len(want)
    for (ka, va), (kb, vb) in zip(got, want):
        assert ka == kb and va == vb, f"stage output {ka} of the generic proof differs from the oracle's"


def case_config_rounds_then_generic(ctx, field, log_n=6, name="len5", blowup=8):
    """The config's own round count, ceil_log2((N - 1) * blowup + 1), on a low-degree trace: round 0's domain is smaller than N * blowup, so the commit phase runs out
    of domain (a one-element domain is no full tree: merkle.rs:93-104) - library and oracle stop at the same stage with the same status.  The SAME context then
    produces the oracle's proof for a Fibonacci trace: nothing of the abandoned proof (length word, pending launch words, side stream) leaks into it."""
    N = 1 << log_n
    trace = trace_of(field, log_n, name)
    ch = random_challenges(field, seed=900 + field)
    ch["betas"] += [3, 2 * N * blowup]
    rounds = int(orc.lib().or_ceil_log2_k(C.c_uint64((N - 1) * blowup + 1), C.c_uint64(2)))
    want = drive_explicit(orc.Session(field), field, trace, blowup, rounds, ch, read_big=False)
    assert want[-1][1] != 0 and want[-1][0].startswith("fri_root") and want[-1][0] != "fri_root0", want[-1][:2]   # abandoned in the middle of the commit phase
    got = drive_explicit(ctx, field, trace, blowup, rounds, ch, read_big=False)
    compare(got, want, f"field {field}, config rounds on support {name}")
    case_generic(ctx, field, log_n, blowup)


def edge_challenges(field, log_n, blowup, which):
    """Challenges on the edges of the field for a Fibonacci proof of 2^log_n rows; `which` selects the (shift, r) pair."""
    p, e = MODULUS[field], EXT[field]
    N = 1 << log_n
    D = N * blowup
    gD, wN = orc.root_of_unity(field, D), orc.root_of_unity(field, N)
    X = lambda *l: E(field, *l)
    z = [X(0), X(1), X(p - 1), X(gD), X(pow(gD, 5, p)), X(wN), X(0, 1), [p - 1] * e]
    if e == 4:
        z.append([0, 0, 5, p - 2])       # first two limbs zero
    z.append(X(12345))
    z = z[3 * which:] + z[:3 * which]    # short proofs have fewer rounds than the list has entries: the four proofs start at different places
    alpha = [X(0), X(1), [p - 1] * e, X(0, 1), X(2), X(p - 1)]
    shift, r = [(1, 0), (p - 1, 1), (gD, p - 1), (3, 12345)][which]
    ood = [X(0), X(1), X(p - 1), X(wN), X(0, 1), [p - 1] * e, X(12345)]
    betas = [0, 1, D - 1, D, D + 1, D // 2, D // 2 + 1, 2**64 - 1, 2**63, 7, 7, 7] + list(range(30))
    return {"shift": shift, "r": r, "ood": ood, "z": z, "alpha": alpha, "betas": betas}


@functools.lru_cache(maxsize=None)
def oracle_edge(field, log_n, blowup, which, read_big):
    trace = fibonacci_trace_fast(field, 1 << log_n)
    ch = edge_challenges(field, log_n, blowup, which)
    assert len(ch["betas"]) == 42 and len(ch["ood"]) == 7
    nc0, D0 = oracle_round0(field, trace, blowup, ch["r"])
    assert D0 == blowup << log_n
    rounds = D0.bit_length() - 1
    nz = len(ch["z"])
    assert len({(3 * k + i) % nz for k in range(4) for i in range(rounds - 1)}) == nz and rounds - 1 >= len(ch["alpha"])   # every listed z and alpha is used
    want = drive_explicit(orc.Session(field), field, trace, blowup, rounds, ch, read_big=read_big)
    return trace, ch, rounds, want


def case_edge_challenges(mk, field, log_n, blowup=8, read_big=False):
    """The Fibonacci trace with z, alpha, shift, r, the OOD points and the betas at 0, 1, p - 1, domain points, elements with zero limbs, repeated queries."""
    ctx = mk(field)
    for which in range(4):
        trace, ch, rounds, want = oracle_edge(field, log_n, blowup, which, read_big)
        got = drive_explicit(ctx, field, trace, blowup, rounds, ch, read_big=read_big)
        compare(got, want, f"field {field}, 2^{log_n} rows, edge challenges, (shift, r) #{which}")


def fri_tail_launches(ctx, run):
    """runs `run()` between ms_profile_begin and ms_profile_end; the number of fused-tail launches (csrc/fri_tail.hpp) the profile counted"""
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    try:
        run()
    finally:
        rc = ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf)))
    ctx.check(rc)
    return json.loads(buf.value.decode()).get("fri_tail", {}).get("launches", 0)
