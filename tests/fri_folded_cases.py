"""Cases of the folded FRI (ms_fri_begin_folded, ms_fri_fold_folded, ms_fri_fold_final, ms_fri_query_folded, msh_fri_folded_verify; include/ministark.h - build-defined,
no reference counterpart), shared by the emulation suite (tests/test_fri_folded_emu.py) and the GPU suite (tests/test_fri_folded_gpu.py).  Expected values:
tests/pyref_fri_folded.py, from round 0's codeword on; every comparison is exact.  The verifying side is checked twice: msh_fri_folded_verify (the host library) and
pyref_fri_folded.verify_msff must agree on every blob, whole or tampered, and name the same step.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set; `d` is the ms_digest_id."""
import ctypes as C
import struct

import numpy as np

import mini_stark_amd as ms
import deep_cases as dc
import open_cases as oc
import pyref
import pyref_fri_folded as rf
import pyref_open as ro
from common import MODULUS, EXT, SplitMix64, fibonacci_trace
from mini_stark_amd.host import fri_folded_verify
from parity_cases import drive

SHA = ro.SHA256
LATENCY = oc.LATENCY
DIGESTS = oc.DIGESTS
ctx_of = oc.ctx_of
_u64p = C.POINTER(C.c_uint64)
SHAPES = ((8, 2), (64, 8), (1 << 10, 2))
BIG = (1 << 13, 8)
SOURCES = ("mix", "air_ext", "deep")


def tuples(a):
    return [tuple(int(x) for x in row) for row in np.asarray(a).tolist()]


# ---------------------------------------------------------------- round 0's polynomial, three ways
def install(ctx, field, kind, N, blowup, seed=3):
    """'mix': the validity polynomial of ms_mix (base-field source); 'air_ext': of ms_mix_air_ext (all E limbs live); 'deep': an installed DEEP polynomial"""
    p, e = MODULUS[field], EXT[field]
    if kind == "mix":
        oc.prepare(ctx, field, fibonacci_trace(field, N), blowup, seed=seed + N)
        return
    trace, cons, exempt, periodic, boundary = dc.fib_spec(field, N, seed=100 + seed)
    c = trace.shape[1]
    rng = SplitMix64(5000 + seed + N)
    dc.commit(ctx, trace, blowup, rng.nonzero(p))
    assert ctx.mix_air_ext(dc.full_ext(rng, field), cons, exempt, periodic, boundary) == 0, ctx.last_error()
    assert ctx.validity_ext() == e
    if kind == "air_ext":
        return
    m = e * dc.vl_of(ctx) // N
    assert ctx.validity_commit(m)[0] == 0, ctx.last_error()
    rows = ms.air_rows(cons, boundary)
    zs = dc.shifted_points(field, dc.full_ext(rng, field), ctx.root_of_unity(N), rows)
    lists = [list(range(c)) + (list(range(c, c + m)) if k == 0 else []) for k in range(len(rows))]
    assert ctx.deep_compose(zs, lists, dc.full_ext(rng, field)) == 0, ctx.last_error()
    assert ctx.deep_len() == N


def max_rounds(D0, blowup, k):
    return ((D0 // blowup).bit_length() - 1) // k


def challenges(field, n, seed):
    p, e, rng = MODULUS[field], EXT[field], SplitMix64(seed)
    return [tuple(rng.field(p) for _ in range(e)) for _ in range(n)]


def commit_phase(ctx, field, blowup, k, R=None, seed=7, alphas=None):
    """ms_fri_begin_folded, R - 1 committed folds, the final fold (R: the most the domain allows unless given): what the verifier is given, and the final polynomial"""
    rc, root = ctx.fri_begin_folded(blowup, k)
    assert rc == 0, ctx.last_error()
    nb, D0 = ctx.fri_round_info(0)
    assert nb == D0 // blowup
    R = max_rounds(D0, blowup, k) if R is None else R
    assert R >= 1
    alphas = challenges(field, R, seed) if alphas is None else [tuple(a) for a in (alphas(D0) if callable(alphas) else alphas)][:R]
    S = dict(field=field, blowup=blowup, k=k, R=R, D0=D0, roots=[root], alphas=alphas)
    for i in range(R - 1):
        rc, root = ctx.fri_fold_folded(alphas[i])
        assert rc == 0, ctx.last_error()
        S["roots"].append(root)
        assert ctx.fri_round_info(i + 1) == ((D0 >> (k * (i + 1))) // blowup, D0 >> (k * (i + 1)))
    rc, fin = ctx.fri_fold_final(alphas[R - 1])
    assert rc == 0, ctx.last_error()
    S["final"] = tuples(fin)
    assert len(S["final"]) == (D0 >> (k * R)) // blowup
    return S


def sample(m, seed, count=512):
    """the first, the last, workgroup edges (256 threads) and random outputs of a launch with m outputs"""
    if m <= count:
        return list(range(m))
    rng = np.random.default_rng(seed)
    pick = {0, 1, m - 1, m - 2, m // 2, m // 2 - 1}
    for wg in (1, 2, m // 256 // 2, m // 256 - 1):
        pick |= {wg * 256 - 1, wg * 256}
    pick |= {int(x) for x in rng.integers(0, m, count - len(pick))}
    return sorted(x for x in pick if 0 <= x < m)


# ---------------------------------------------------------------- 1. the fold against both restatements
def check_fold(ctx, d, field, S, whole=True, trees=False):
    """every committed codeword and the final polynomial against pyref from round 0's codeword (whole vectors), or - `whole` False - 512 outputs of every fold from
    the codeword it folded; returns (codewords, pyref's trees if asked)"""
    k, R, blowup = S["k"], S["R"], S["blowup"]
    T = rf.tower(field)
    p = MODULUS[field]
    dev = [tuples(ctx.fri_round_codeword(i)) for i in range(R)]
    assert [len(c) for c in dev] == [S["D0"] >> (k * i) for i in range(R)]
    if whole:
        P = rf.prove(field, d, dev[0], blowup, k, S["alphas"], trees=trees)
        for i in range(R):
            assert dev[i] == P["cws"][i], f"round {i} is not the Lagrange fold of round {i - 1}"
        assert not P["high"] and S["final"] == P["final"]
        for i in range(R - 1):                       # the second statement: coefficient split and forward evaluation
            assert rf.fold_split(field, dev[i], k, S["alphas"][i]) == dev[i + 1], f"round {i + 1} is not the split fold of round {i}"
        last = rf.fold_split(field, dev[R - 1], k, S["alphas"][R - 1])
        assert rf.interpolate(field, last)[:len(S["final"])] == S["final"]
        return dev, P
    DR = S["D0"] >> (k * R)
    gR = pyref.root_of_unity(field, DR)
    for i in range(R):
        m = len(dev[i]) >> k
        at = sample(m, seed=i)
        got = rf.fold_lagrange(field, dev[i], k, S["alphas"][i], at)
        if i + 1 < R:
            assert got == [dev[i + 1][b] for b in at], f"round {i + 1}"
            if len(dev[i]) <= 1 << 12:
                assert rf.fold_split(field, dev[i], k, S["alphas"][i]) == dev[i + 1]
        else:
            assert got == [pyref.peval(T, S["final"], T.from_base(pow(gR, b, p))) for b in at], "final polynomial"
    return dev, None


def case_fold(make, d, field, N, blowup, k, kind, extra=0, whole=True):
    ctx = ctx_of(make, d, field, extra)
    install(ctx, field, kind, N, blowup)
    if kind == "mix":                                  # round 0 is ms_fri_begin's: the same codeword
        assert ctx.fri_begin(blowup, 1)[0] == 0
        legacy0 = ctx.fri_round_codeword(0)
    S = commit_phase(ctx, field, blowup, k, seed=31 + k)
    if kind == "mix":
        assert S["D0"] == N * blowup and (ctx.fri_round_codeword(0) == legacy0).all()
    if (N, blowup) == (8, 2) and kind == "mix" and k == 3:
        assert S["R"] == 1
    if (N, blowup) == (1 << 10, 2) and kind == "mix" and k == 3:   # log2(D_0 / blowup) = 10 is no multiple of 3: the final polynomial has two coefficients
        assert len(S["final"]) == 2
    assert len(S["final"]) == 1 << (((S["D0"] // blowup).bit_length() - 1) % k)
    check_fold(ctx, d, field, S, whole=whole)
    return ctx, S


# ---------------------------------------------------------------- 2. edge challenges
def edge_alphas(field, k):
    """per pattern a function D_0 -> the rounds' challenges: 0, 1, p - 1 in limb 0, a base-field alpha, a point of the round's own domain (alpha / x = 1 for one
    output), all limbs p - 1"""
    p, e = MODULUS[field], EXT[field]
    base = lambda v: (lambda D0: [(v,) + (0,) * (e - 1)] * 64)   # noqa: E731
    pats = {"zero": base(0), "one": base(1), "minus_one": base(p - 1), "base": base(SplitMix64(91).nonzero(p)), "all_minus_one": lambda D0: [(p - 1,) * e] * 64}
    pats["domain_point"] = lambda D0: [(pow(pyref.root_of_unity(field, D0 >> (k * i)), 5 % max(1, D0 >> (k * (i + 1))), p),) + (0,) * (e - 1) for i in range(64) if D0 >> (k * i) >= 1]
    return pats


def case_edge_alphas(make, d, field, k, N=64, blowup=8):
    ctx = ctx_of(make, d, field)
    install(ctx, field, "air_ext", N, blowup)
    for name, alphas in edge_alphas(field, k).items():
        S = commit_phase(ctx, field, blowup, k, alphas=alphas)
        check_fold(ctx, d, field, S)


# ---------------------------------------------------------------- 3. trees and blob
def beta_sets(D0):
    big = (1 << 63) + 12345
    return [[0, D0 - 1, big, D0, 7, 7], [D0 + 1], [(j * 0x9E3779B97F4A7C15) % (1 << 64) for j in range(33)]]


def check_blob(ctx, d, S, leaves, nodes, betas):
    """the MSFF bytes: header | final | the ms_tree_open outputs, and pyref's blob"""
    field, k, R = S["field"], S["k"], S["R"]
    e = EXT[field]
    blob = ctx.fri_query_folded(betas)
    want = bytearray(struct.pack("<7Q", rf.MAGIC, e, k, R, len(betas), S["D0"], len(S["final"])))
    for c in S["final"]:
        want += struct.pack("<%dQ" % e, *c)
    pos = rf.positions(betas, S["D0"], k, R)
    for i in range(R):
        want += ctx.tree_open(ms.TREE_FRI, pos[i + 1], i)
    assert blob == bytes(want)
    assert blob == rf.msff_blob(e, k, leaves, nodes, S["final"], betas)
    return blob


def case_trees_and_blob(make, d, field, N, blowup, k, extra=0, whole=True, kind="mix"):
    ctx = ctx_of(make, d, field, extra)
    install(ctx, field, kind, N, blowup)
    S = commit_phase(ctx, field, blowup, k, seed=41 + k)
    dev, _ = check_fold(ctx, d, field, S, whole=whole)
    leaves, nodes = [], []
    for i in range(S["R"]):
        lv, nd = rf.coset_tree(d, dev[i], k)
        assert bytes(nd[-1]) == S["roots"][i], f"root of round {i}"
        leaves.append(lv); nodes.append(nd)
    a = 1 << k
    for i in (0, S["R"] - 1):                          # ms_tree_open on a coset-leaf tree: every group of the last round, a few of the first
        groups = len(dev[i]) // a
        ix = list(range(groups)) if groups <= 64 else oc.index_lists(groups)[3]
        oc.check_paths(ctx, d, field, ctx.tree_open(ms.TREE_FRI, ix, i), leaves[i], EXT[field], a, nodes[i], S["roots"][i], ix)
    for betas in beta_sets(S["D0"]):
        blob = check_blob(ctx, d, S, leaves, nodes, betas)
        assert verify_both(d, S, betas, blob) == (True, "")
    return ctx, S


# ---------------------------------------------------------------- 4. the verifier
def verify_both(d, S, betas, blob, **over):
    """(accepted, step) on which the host library and pyref must agree, with any of the verifier's inputs replaced"""
    V = dict(S); V.update(over)
    rc, why = fri_folded_verify(d, V["field"], True, V["blowup"], V["k"], V["roots"], V["alphas"], betas, blob)
    ok, step = rf.verify_msff(V["field"], d, True, V["blowup"], V["k"], V["roots"], V["alphas"], betas, blob)
    assert rc in (0, 1) and (rc == 1) == ok, (rc, ok, why, step)
    assert ok or why.startswith(step + ": "), (why, step)
    return ok, step


def case_verifier(make, d, field, k=2, N=64, blowup=8):
    ctx = ctx_of(make, d, field)
    e, p, a = EXT[field], MODULUS[field], 1 << k
    install(ctx, field, "deep", N, blowup)
    assert ctx.fri_begin_folded(blowup, k)[0] == 0, ctx.last_error()
    D0 = ctx.fri_round_info(0)[1]
    R = max(2, max_rounds(D0, blowup, k) - 1)          # (one fold short of the most where that leaves two rounds: a final polynomial of a coefficients)
    S = commit_phase(ctx, field, blowup, k, R=R, seed=51)
    assert len(S["final"]) >= (2 if k < 3 else 1)
    betas = [9, (1 << 63) + 40, D0 - 1]
    nq = len(betas)
    blob = ctx.fri_query_folded(betas)
    assert verify_both(d, S, betas, blob) == (True, "")
    nfinal = len(S["final"])
    heights = [(D0 >> (k * (i + 1))).bit_length() - 1 for i in range(R)]
    psize = [16 + a * e * 8 + 64 * h for h in heights]
    sect = [56, 56 + nfinal * e * 8]                   # section boundaries: the header's end, the final polynomial's, every round's paths'
    for i in range(R):
        sect.append(sect[-1] + nq * psize[i])
    assert sect[-1] == len(blob)
    pos = rf.positions(betas, D0, k, R)

    def flip(at, bit=0):
        b = bytearray(blob); b[at] ^= 1 << bit
        return bytes(b)

    def rejected(b, step, betas_=betas, **over):
        ok, got = verify_both(d, S, betas_, b, **over)
        assert not ok and got == step, (got, step)
    for w in range(7):                                 # every header word
        rejected(flip(8 * w), "header")
    rejected(flip(56), "final polynomial")             # a final-polynomial limb: the first, the last, one made non-canonical
    rejected(flip(sect[1] - 8), "final polynomial")
    rejected(blob[:56] + struct.pack("<Q", p) + blob[64:], "final polynomial")
    for i in (1, R - 1):                               # round i, query 0: a limb of the slot the fold of round i - 1 lands in, a limb of another slot, a non-canonical one
        p0 = sect[1 + i]
        slot = pos[i][0] // (D0 >> (k * (i + 1)))
        other = (slot + 1) % a
        rejected(flip(p0 + 8 + slot * e * 8), "round %d opening" % i)
        rejected(flip(p0 + 8 + other * e * 8 + 8 * (e - 1)), "round %d opening" % i)
        rejected(blob[:p0 + 8] + struct.pack("<Q", p) + blob[p0 + 16:], "round %d opening" % i)
        rejected(flip(p0), "round %d opening" % i)                                  # the leaf_index word
        rejected(flip(p0 + 8 + a * e * 8), "round %d opening" % i)                  # the height word
    lv = sect[1] + 16 + a * e * 8                      # round 0, query 0: the two digests of one level swapped, a sibling digest
    assert heights[0] >= 2
    swapped = blob[:lv] + blob[lv + 32:lv + 64] + blob[lv:lv + 32] + blob[lv + 64:]
    rejected(swapped, "round 0 opening")
    rejected(flip(lv + 64 + 5), "round 0 opening")
    for i in range(R):                                 # a root, an alpha
        roots = list(S["roots"]); roots[i] = bytes(32)
        rejected(blob, "round %d opening" % i, roots=roots)
        al = list(S["alphas"]); al[i] = ((al[i][0] + 1) % p,) + al[i][1:]
        rejected(blob, "round %d fold" % (i + 1) if i + 1 < R else "final polynomial", alphas=al)
    rejected(blob, "round 0 opening", betas_=[10] + betas[1:])      # a beta
    rejected(blob, "header", betas_=betas[:-1])
    for cut in sect[:-1]:                              # a truncation at every section boundary, and inside a section; a trailing byte
        rejected(blob[:cut], "header")
    rejected(blob[:-1], "header")
    rejected(blob[:40], "header")
    rejected(blob + b"\0", "header")
    al = list(S["alphas"]); al[0] = (p,) + al[0][1:]    # a challenge that is no field element: a malformed argument, not a verdict
    rc, why = fri_folded_verify(d, field, True, blowup, k, S["roots"], al, betas, blob)
    assert rc < 0 and "canonical" in why
    rejected(blob, "header", blowup=2 * blowup)        # another rate: nfinal is no longer D_R / blowup
    rejected(blob, "header", k=k % 3 + 1)
    rejected(blob, "header", roots=S["roots"][:-1], alphas=S["alphas"][:-1])
    # a blob made by pyref's prover from a round 0 that is NOT of low degree (a random vector): honest trees, honest folds - the final polynomial cannot fit
    rng = SplitMix64(77)
    c0 = [tuple(rng.field(p) for _ in range(e)) for _ in range(D0)]
    P = rf.prove(field, d, c0, blowup, k, S["alphas"])
    assert P["high"]
    bad = rf.msff_blob(e, k, P["leaves"], P["nodes"], P["final"], betas)
    ok, step = verify_both(d, S, betas, bad, roots=P["roots"])
    assert not ok and (step == "final polynomial" or step.endswith("fold")), step
    # ... and from a low-degree one it is accepted
    good = tuples(ctx.fri_round_codeword(0))
    P = rf.prove(field, d, good, blowup, k, S["alphas"])
    assert not P["high"] and P["roots"] == S["roots"]
    assert rf.msff_blob(e, k, P["leaves"], P["nodes"], P["final"], betas) == blob


# ---------------------------------------------------------------- 5. state and refusals
def raw_begin(ctx, blowup, k, root=True):
    r = (C.c_uint8 * 32)()
    return ctx.L.ms_fri_begin_folded(ctx.h, C.c_size_t(blowup), C.c_int(k), r if root else None)


def raw_fold(ctx, alpha, root=True):
    a = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.uint64)
    r = (C.c_uint8 * 32)()
    return ctx.L.ms_fri_fold_folded(ctx.h, None if a is None else a.ctypes.data_as(_u64p), r if root else None)


def raw_final(ctx, alpha, cap, want_n=True, out=True):
    a = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.uint64)
    buf = np.full(max(1, cap), 0xABABABAB, dtype=np.uint64)
    n = C.c_size_t(0xDEAD)
    rc = ctx.L.ms_fri_fold_final(ctx.h, None if a is None else a.ctypes.data_as(_u64p), buf.ctypes.data_as(_u64p) if out else None, C.c_size_t(cap),
                                 C.byref(n) if want_n else None)
    return rc, n.value, buf


def raw_query(ctx, betas, nq, out, cap, want_len=True):
    b = None if betas is None else np.ascontiguousarray(betas, dtype=np.uint64)
    ln = C.c_size_t(0xDEAD)
    rc = ctx.L.ms_fri_query_folded(ctx.h, None if b is None else b.ctypes.data_as(_u64p), C.c_int(nq), out, C.c_size_t(cap), C.byref(ln) if want_len else None)
    return rc, ln.value


def legacy_calls(ctx, field):
    """the legacy FRI calls that folded mode refuses, raw: [(name, rc)]"""
    e = EXT[field]
    z = np.arange(1, e + 1, dtype=np.uint64)
    B = np.zeros(2 * e, dtype=np.uint64)
    root = (C.c_uint8 * 32)()
    buf = (C.c_uint8 * 4096)()
    ln = C.c_size_t(0)
    zp, L, h = z.ctypes.data_as(_u64p), ctx.L, ctx.h
    return [("fri_deep", L.ms_fri_deep(h, zp, B.ctypes.data_as(_u64p))), ("fri_fold_commit", L.ms_fri_fold_commit(h, zp, root)),
            ("fri_query", L.ms_fri_query(h, zp, C.c_int(1))), ("fri_query_into", L.ms_fri_query_into(h, zp, C.c_int(1), None, C.c_size_t(0), C.byref(ln))),
            ("fri_proof_read", L.ms_fri_proof_read(h, buf)), ("fri_proof_read_async", L.ms_fri_proof_read_async(h, buf)), ("fri_proof_wait", L.ms_fri_proof_wait(h)),
            ("fri_query_index", L.ms_fri_query_index(h, zp, C.c_int(1), None, C.c_size_t(0), C.byref(ln))),
            ("query_linked", L.ms_query_linked(h, zp, C.c_int(1), None, C.c_size_t(0), C.byref(ln))),
            ("fri_round_poly_read", L.ms_fri_round_poly_read(h, C.c_int(0), B.ctypes.data_as(_u64p)))]


def case_refusals(make, d, field, k=2, N=64, blowup=8):
    """every MS_ERR_* of the four entry points at its site, between the steps of a commit phase whose outputs are those of a context that was never refused"""
    p, e, a = MODULUS[field], EXT[field], 1 << k
    ctx, fresh = ctx_of(make, d, field), ctx_of(make, d, field)
    trace = fibonacci_trace(field, N)
    assert ctx.trace_commit(trace, 6)[0] == 0
    al = challenges(field, 8, seed=5)
    assert raw_begin(ctx, blowup, k) == ms.ERR_STATE                                  # no validity polynomial yet
    assert raw_fold(ctx, al[0]) == ms.ERR_STATE                                       # the three calls outside folded mode
    assert raw_final(ctx, al[0], 64)[0] == ms.ERR_STATE
    assert raw_query(ctx, [1], 1, None, 0)[0] == ms.ERR_STATE
    for c in (ctx, fresh):
        install(c, field, "mix", N, blowup)
    want = commit_phase(fresh, field, blowup, k, alphas=al)
    betas = [3, 1 << 40]
    want_blob = fresh.fri_query_folded(betas)
    R = want["R"]
    assert R >= 2
    assert ctx.L.ms_fri_begin_folded(None, C.c_size_t(blowup), C.c_int(k), (C.c_uint8 * 32)()) == ms.ERR_ARG
    for bad_k in (0, 4, -1):
        assert raw_begin(ctx, blowup, bad_k) == ms.ERR_ARG
    assert raw_begin(ctx, 0, k) == ms.ERR_ARG
    assert raw_begin(ctx, blowup, k, root=False) == ms.ERR_ARG
    assert raw_begin(ctx, 1 << (pyref.FIELDS[field]["adicity"] - 2), k) == ms.ERR_SHAPE        # D_0 above the two-adicity
    assert raw_begin(ctx, 1 << pyref.FIELDS[field]["adicity"], k) == ms.ERR_SHAPE              # ... and a blowup no domain can hold with a fold (refused without the degree scan)
    assert raw_fold(ctx, al[0]) == ms.ERR_STATE                                       # (the refused begins started nothing)
    # legacy FRI under way: the new calls are refused, the legacy ones work
    assert ctx.fri_begin(blowup, 2)[0] == 0
    assert raw_fold(ctx, al[0]) == ms.ERR_STATE and raw_final(ctx, al[0], 64)[0] == ms.ERR_STATE and raw_query(ctx, [1], 1, None, 0)[0] == ms.ERR_STATE
    rc, root0 = ctx.fri_begin_folded(blowup, k)
    assert rc == 0 and root0 == want["roots"][0]
    assert raw_begin(ctx, blowup, 7) == ms.ERR_ARG                                    # a refused begin leaves the commit phase under way as it is
    for name, rc in legacy_calls(ctx, field):
        assert rc == ms.ERR_STATE, name
    assert ctx.fri_proof_size() == 0
    assert raw_query(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE                       # before ms_fri_fold_final
    assert raw_fold(ctx, None) == ms.ERR_ARG
    assert raw_fold(ctx, al[0], root=False) == ms.ERR_ARG
    assert raw_fold(ctx, [p] + [0] * (e - 1)) == ms.ERR_ARG                           # not canonical
    for i in range(R - 1):
        rc, root = ctx.fri_fold_folded(al[i])
        assert rc == 0 and root == want["roots"][i + 1]
    assert max_rounds(want["D0"], blowup, k) == R
    assert raw_fold(ctx, al[R - 1]) == ms.ERR_SHAPE                                   # D_(i+1) < a * blowup: only the final fold is left
    assert ctx.fri_round_info(R - 1)[1] == want["D0"] >> (k * (R - 1))
    nfinal = len(want["final"])
    assert raw_final(ctx, None, 64)[0] == ms.ERR_ARG
    assert raw_final(ctx, [p] * e, 64)[0] == ms.ERR_ARG
    assert raw_final(ctx, al[R - 1], 64, want_n=False)[0] == ms.ERR_ARG
    assert raw_final(ctx, al[R - 1], 5, out=False)[0] == ms.ERR_ARG                   # null coeffs with a capacity
    assert raw_final(ctx, al[R - 1], 0, out=False)[:2] == (0, nfinal)                 # the size query
    rc, n, buf = raw_final(ctx, al[R - 1], nfinal * e - 1)
    assert (rc, n) == (ms.ERR_ARG, nfinal) and (buf == 0xABABABAB).all()              # one word short: nothing written
    assert raw_query(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE
    rc, n, buf = raw_final(ctx, al[R - 1], nfinal * e + 3)
    assert (rc, n) == (0, nfinal) and tuples(buf[:nfinal * e].reshape(-1, e)) == want["final"] and (buf[nfinal * e:] == 0xABABABAB).all()
    assert raw_final(ctx, al[R - 1], 64)[0] == ms.ERR_STATE                           # a second final fold, a fold after it
    assert raw_fold(ctx, al[0]) == ms.ERR_STATE
    size = len(want_blob)
    qb = (C.c_uint8 * (size + 8))(*([0xAB] * (size + 8)))
    untouched = bytes(qb)
    assert raw_query(ctx, betas, 2, None, 0) == (0, size)
    assert raw_query(ctx, betas, 2, qb, size - 1) == (ms.ERR_ARG, size)
    assert raw_query(ctx, None, 2, qb, size)[0] == ms.ERR_ARG
    assert raw_query(ctx, betas, 2, qb, size, want_len=False)[0] == ms.ERR_ARG
    assert raw_query(ctx, betas, 2, None, size)[0] == ms.ERR_ARG
    assert raw_query(ctx, betas, 0, qb, size)[0] == ms.ERR_ARG
    assert raw_query(ctx, [7] * 4097, 4097, None, 0)[0] == ms.ERR_ARG
    assert raw_query(ctx, [7] * 4096, 4096, None, 0)[0] == 0
    assert bytes(qb) == untouched
    assert ctx.fri_query_folded(betas) == want_blob and ctx.fri_query_folded(betas) == want_blob
    for name, rc in legacy_calls(ctx, field):
        assert rc == ms.ERR_STATE, name
    assert oc.raw_open(ctx, ms.TREE_FRI, R, [0], 1, None, 0)[0] == ms.ERR_ARG         # round R is not committed
    # whatever clears the FRI state clears the mode
    assert ctx.mix(5) == 0
    assert raw_query(ctx, betas, 2, None, 0)[0] == ms.ERR_STATE and raw_fold(ctx, al[0]) == ms.ERR_STATE
    assert ctx.L.ms_fri_proof_wait(ctx.h) == 0
    # D_0 < a * blowup: a constant trace has D_0 = blowup
    const = ctx_of(make, d, field)
    oc.prepare(const, field, np.full((16, 3), 5, dtype=np.uint64), blowup, seed=8)
    assert raw_begin(const, blowup, 1) == ms.ERR_SHAPE and "no fold" in const.last_error()
    assert const.fri_begin(blowup, 1)[0] == 0 and const.fri_round_info(0)[1] == blowup


def case_sharded(ctx):
    """a context with sharding on (a one-rank world, MS_SHARD_WORLD1=1 set by the caller) refuses ms_fri_begin_folded, as ms_tree_open does"""
    from mini_stark_amd.dist import LocalShard
    sh = LocalShard(ctx, 4 << 20)
    oc.prepare(ctx, 0, fibonacci_trace(0, 64), 8, seed=3)
    assert raw_begin(ctx, 8, 2) == ms.ERR_STATE and "sharding" in ctx.last_error()
    sh.close()


def case_switching(make, d, field, N=64, blowup=8):
    """ms_fri_begin after a folded FRI and the reverse on one context; the headline legacy flow gives the same bytes before and after a folded FRI"""
    trace = fibonacci_trace(field, 32)
    ctx = ctx_of(make, d, field)
    before = drive(ctx, field, trace, 4, 2, seed=41)
    install(ctx, field, "mix", N, blowup)
    fresh = ctx_of(make, d, field)
    install(fresh, field, "mix", N, blowup)
    Rl = 4
    legacy = oc.commit_phase(fresh, field, blowup, Rl, seed=9)
    legacy_blob = fresh.fri_query_index([5, 77])
    folded = {}
    for k in (1, 3):
        folded[k] = commit_phase(fresh, field, blowup, k, seed=10)
        folded[k]["blob"] = fresh.fri_query_folded([5, 77])
    for k in (3, 1):
        S = commit_phase(ctx, field, blowup, k, seed=10)                              # folded, then legacy, then folded with another arity
        assert (S["roots"], S["final"]) == (folded[k]["roots"], folded[k]["final"]) and ctx.fri_query_folded([5, 77]) == folded[k]["blob"]
        S2 = oc.commit_phase(ctx, field, blowup, Rl, seed=9)
        assert S2["roots"] == legacy["roots"] and S2["Bs"] == legacy["Bs"] and ctx.fri_query_index([5, 77]) == legacy_blob
        assert ctx.fri_query([5, 77])[0] == 0
    after = drive(ctx, field, trace, 4, 2, seed=41)
    assert [n for n, _ in after] == [n for n, _ in before]
    for (n, x), (_, y) in zip(after, before):
        assert x == y, f"stage output {n} differs after a folded FRI on the same context"


# ---------------------------------------------------------------- 7. launches
def case_launch_count(make, d, field, N=1 << 10, blowup=8, k=3):
    ctx = ctx_of(make, d, field)
    install(ctx, field, "mix", N, blowup)
    al = challenges(field, 16, seed=3)
    assert ctx.fri_begin_folded(blowup, k)[0] == 0
    count = lambda prof: {n: v["launches"] for n, v in prof.items() if isinstance(v, dict) and v.get("launches")}   # noqa: E731
    (rc, _), prof = oc.profile(ctx, lambda: ctx.fri_fold_folded(al[0]))
    got = count(prof)
    assert rc == 0 and got.pop("fold") == 1 and got and set(got) <= {"leaf_hash", "inner_hash"}, prof     # one fold launch plus the tree's
    R = max_rounds(ctx.fri_round_info(0)[1], blowup, k)
    for i in range(1, R - 1):
        assert ctx.fri_fold_folded(al[i])[0] == 0
    assert ctx.fri_fold_final(al[R - 1])[0] == 0
    betas = list(range(1, 33))
    blob, prof = oc.profile(ctx, lambda: ctx.fri_query_folded(betas))
    assert count(prof) == {"merkle_path": 1}, prof                                    # ONE launch, whatever R and nq
    assert blob == ctx.fri_query_folded(betas)
