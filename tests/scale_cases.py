"""Cases of the linked and the staged flow AT THE SIZES THE LARGE KERNELS RUN (ms_mix_air_ext, ms_validity_commit, ms_deep_evals, ms_deep_compose, the FRI commit phase over an
E-limb round 0, ms_query_linked, ms_aux_running_staged / ms_lde_commit_stage; include/ministark.h), shared by the emulation suite (tests/test_scale_emu.py) and the GPU suite
(tests/test_scale_gpu.py).  The suites of the single stages stop at N = 64 .. 1024, where every FRI round is one fused launch, every transform a single-pass plan and
every tree one subtree launch; here the WHOLE output of every stage answers to an independent reference at

  A: N = 2^11, L = D_0 = 2^14   the first cooperative NTT plan (the size-L inverse transform of ms_mix_air_ext); every round after round 0 still one fused launch
  B: N = 2^13, L = D_0 = 2^16   round 0 an E-limb transform on the 2^16 tiles, round 0 -> 1 unfused, LDE / validity trees of 2^16 groups (a level launch in front of the subtrees)
  C: N = 2^16, L = D_0 = 2^19   (GPU only) the workgroup fold with an E-limb source from round 0 on, four unfused rounds, FRI trees with level launches, cooperative forward plans

all at blowup 8.  References: oracle.ntt / intt / coset_lde (the C++ oracle), pyref_open.tree_nodes (hashlib / pyref_blake3 / pyref_keccak), pyref.Tower big-integer
arithmetic, pyref_deep, pyref_air_ext, pyref_aux.  Every comparison is exact; the only probabilistic checks are polynomial identities at random points, whose number is
computed from the degree for a false accept below 2^-60.  Nothing of the product is imported but the entry points under test.
`make(field, flags, env=None)` returns a fresh mini_stark_amd.Context created with `flags` while the variables of `env` are set; `d` is the ms_digest_id."""
import operator
import re
from fractions import Fraction

import numpy as np

import mini_stark_amd as ms
import deep_cases as dc
import linked_cases as lc
import open_cases as oc
import pyref
import pyref_air_ext as rx
import pyref_aux as rax
import pyref_deep as rd
import pyref_open as ro
import staged_cases as sc
from common import MODULUS, EXT, SplitMix64
from oracle import oracle

SHA, BLAKE3, KECCAK = ro.SHA256, ro.BLAKE3, ro.KECCAK256
BLOWUP = 8
LATENCY = oc.LATENCY
SHAPES = {"A": 1 << 11, "B": 1 << 13, "C": 1 << 16}
# the thresholds of the build (csrc/ctx.hpp, csrc/poly.hpp, csrc/merkle.hpp) the profile assertions restate: a change of one of them fails the test that names the shape
FRI_TAIL_MAX, SUBTREE_PARENTS, SUBTREE_LEVELS, SCAN_BLOCK = 1 << 15, 16384, 9, 2048
BOUND = Fraction(1, 1 << 60)


def launches(prof):
    return {k: v["launches"] for k, v in prof.items() if isinstance(v, dict) and v.get("launches")}


def points_for(per_point):
    """the smallest k with per_point^k < 2^-60 (per_point: the false accept of one random point, a Fraction)"""
    assert 0 < per_point < 1
    k, acc = 1, per_point
    while acc >= BOUND:
        k, acc = k + 1, acc * per_point
    return k


# ---------------------------------------------------------------- evaluation by the definition sum_k c_k z^k: one table of powers per point, one dot product per limb plane
def power_planes(T, z, n):
    """z^0 .. z^(n-1) in K as E lists of n integers (limb planes)"""
    planes, acc, z = [[] for _ in range(T.e)], T.one(), tuple(z)
    for _ in range(n):
        for l in range(T.e):
            planes[l].append(acc[l])
        acc = T.mul(acc, z)
    return planes


def at_point(p, col, planes):
    """a polynomial with base-field coefficients (Python integers, lowest first, at most as many as the table holds) at the table's point: E limbs"""
    assert len(col) <= len(planes[0])
    return tuple(sum(map(operator.mul, col, plane)) % p for plane in planes)


def ext_at_point(T, limb_cols, planes):
    """a K-valued polynomial given as its E limb planes: sum_l u_l * (plane l at the point), u_l the basis of K over the base field"""
    acc = T.zero()
    for l, col in enumerate(limb_cols):
        u = tuple(1 if i == l else 0 for i in range(T.e))
        acc = T.add(acc, T.mul(u, at_point(T.p, col, planes)))
    return acc


def base_horner(p, col, x):
    acc = 0
    for c in reversed(col):
        acc = (acc * x + c) % p
    return acc


def rhs_at(field, omega, N, cols, r, air, z):
    """pyref_air_ext.rhs_at (the defining formula of ms_mix_air_ext at z in K, inverses in K) with the factors P_j(z w^row) taken from tables of powers instead of one
    Horner per factor; no periodic columns.  Held to pyref_air_ext.rhs_at itself on shape A."""
    cons, exempt, periodic, boundary = air
    assert not periodic
    p, T = MODULUS[field], rx.tower(field)
    tables, seen = {}, {}

    def factor(poly, row):
        if (poly, row) not in seen:
            if row not in tables:
                tables[row] = power_planes(T, T.mul(tuple(z), T.from_base(pow(omega, row, p))), N)
            seen[(poly, row)] = at_point(p, cols[poly], tables[row])
        return seen[(poly, row)]
    den = T.sub(T.pow(tuple(z), N), T.one())
    assert not T.is_zero(den)
    acc, rp = T.zero(), T.one()
    for terms, rows in zip(cons, exempt):
        ct = T.zero()
        for coef, factors in terms:
            m = T.from_base(coef)
            for poly, row in factors:
                m = T.mul(m, factor(poly, row))
            ct = T.add(ct, m)
        for rho in rows:
            ct = T.mul(ct, T.sub(tuple(z), T.from_base(pow(omega, rho, p))))
        acc = T.add(acc, T.mul(rp, ct))
        rp = T.mul(rp, tuple(r))
    acc = T.mul(acc, T.inv(den))
    for poly, row, value in boundary:
        num = T.sub(factor(poly, 0), T.from_base(value))
        acc = T.add(acc, T.mul(rp, T.mul(num, T.inv(T.sub(tuple(z), T.from_base(pow(omega, row, p)))))))
        rp = T.mul(rp, tuple(r))
    return acc


def next_round_poly(T, poly, alpha, z, B):
    """(fold(poly, alpha) - B(alpha)) / (x - z) by exact synthetic division over K, trimmed; poly: limb tuples, lowest coefficient first"""
    n = len(poly)
    m = (n + 1) // 2
    folded = [T.add(poly[2 * k], T.mul(alpha, poly[2 * k + 1])) if 2 * k + 1 < n else poly[2 * k] for k in range(m)]
    if not folded:
        return []
    folded[0] = T.sub(folded[0], T.add(B[0], T.mul(B[1], alpha)))
    q, carry = [None] * (m - 1), T.zero()
    for k in range(m - 1, 0, -1):
        carry = T.add(folded[k], T.mul(carry, z))
        q[k - 1] = carry
    assert T.is_zero(T.add(folded[0], T.mul(carry, z))), "B is not (even(z), odd(z)): the division leaves a remainder"
    return pyref.trim(T, q)


# ---------------------------------------------------------------- the launches a shape stands for
def inner_launches(ngroups, subtree_parents=SUBTREE_PARENTS):
    """inner_hash launches of a binary tree over `ngroups` leaf groups: one per level of more than `subtree_parents` parents, then subtree launches of up to 9 levels"""
    levels, subtrees, n = 0, 0, ngroups
    while n > 1 and n // 2 > subtree_parents:
        levels, n = levels + 1, n // 2
    while n > 1:
        subtrees, n = subtrees + 1, n >> min(SUBTREE_LEVELS, n.bit_length() - 1)
    return levels, subtrees


def scan_launches(m):
    """suffix_horner launches of a scan over m elements: 2 levels - 1"""
    levels, n = 1, (m + SCAN_BLOCK - 1) // SCAN_BLOCK
    while n > 1:
        levels, n = levels + 1, (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    return 2 * levels - 1


# The cooperative NTT instances a shape reaches (ntt_pass_variants: the kernel names a profiler reports), per field and log2 L.  MIX: the size-L inverse transform with
# batch E inside ms_mix_air_ext, cooperative from L = 2^14 on (the sign-bit class GLT with two sub-rounds on shape A, the exec-masked class GLM with three from 2^16).
# FORWARD: the coefficient -> blowup-8 evaluations of ms_lde_commit, ms_validity_commit and round 0.  They are zero-padded transforms of N coefficients, which are
# cooperative (mode 2, behind the virtual pass) from N = 2^14 coefficients on: on shapes A and B they run PassKernel / PassKernelK, and only shape C reaches them.
COOP_MIX = {(0, 14): r"msntt::PassKernel2<GL, GLT, true, 7, 3, 256, 2, [01]>", (0, 16): r"msntt::PassKernel2<GL, GLM, true, 8, 3, 256, 3, [01]>",
            (0, 19): r"msntt::PassKernel2<GL, GLM, true, (9|10), 3, 512, 3, [01]>",
            (1, 14): r"msntt::PassKernel2<BB, BB, true, 7, 4, 256, 2, [01]>", (1, 16): r"msntt::PassKernel2<BB, BB, true, 8, 4, 256, 2, [01]>",
            (1, 19): r"msntt::PassKernel2<BB, BB, true, (9|10), 4, 512, [23], [01]>"}
COOP_FORWARD = {(0, 19): r"msntt::PassKernel2<GL, GLM, false, .*", (1, 19): r"msntt::PassKernel2<BB, BB, false, .*"}


def assert_reached(prof, pattern):
    variants = prof["ntt_pass_variants"]
    assert any(re.fullmatch(pattern, name) and v["launches"] > 0 for name, v in variants.items()), (pattern, sorted(variants))


def check_commit_profile(field, prof, infos):
    """the commit phase ran the kernel classes its domains stand for"""
    got = launches(prof)
    R = len(infos)
    fused = [i for i in range(1, R) if infos[i - 1][1] <= FRI_TAIL_MAX]
    unfused = [i for i in range(1, R) if infos[i - 1][1] > FRI_TAIL_MAX]
    D0 = infos[0][1]
    assert got.get("fri_tail", 0) == len(fused), (got, fused)
    assert got.get("fold", 0) == 2 * len(unfused), got                      # the coefficient fold and the pointwise codeword fold of every unfused round
    assert got.get("degree", 0) == 1 + len(unfused), got                    # D' is scanned by ms_fri_begin
    assert got.get("suffix_horner", 0) == sum(scan_launches((infos[i - 1][0] + 1) // 2) for i in unfused), got
    want_inner = [inner_launches(infos[i][1] // 2) for i in [0] + unfused]
    assert got.get("inner_hash", 0) == sum(a + b for a, b in want_inner), (got, want_inner)
    if D0 <= FRI_TAIL_MAX:
        assert not unfused and "fold" not in got
    else:
        assert unfused and fused and all(k in got for k in ("fold", "suffix_horner", "degree"))
    return got


# ---------------------------------------------------------------- the stages, driven by hand
def beta_set(D0):
    """a position whose partner wraps (b >= D_0 / 2), repeated; one that does not; one above 2^63"""
    return [D0 // 2 + 1, 5, D0 // 2 + 1, 2**63 + 12345]


def drive(ctx, d, field, N, name="cubic", profile=True):
    """ms_trace_commit -> ms_interpolate -> ms_lde_commit -> ms_mix_air_ext (r in K) -> ms_validity_commit -> ms_deep_evals -> ms_deep_compose -> the FRI commit phase down
    to a domain of 8 points -> ms_query_linked, as deep_cases.build_proof drives them: a dict of everything the calls returned.  `profile`: the LDE commitment, the
    mix stage, the validity commitment and the commit phase run between ms_profile_begin and ms_profile_end (False: not at all - the side stream of MS_FLAG_LATENCY is off under it)"""
    p, e = MODULUS[field], EXT[field]
    trace, cons, exempt, periodic, boundary = dc.SPECS[name](field, N, seed=101)
    c, L = trace.shape[1], N * BLOWUP
    rng = SplitMix64(5001)
    P = dict(field=field, d=d, N=N, c=c, L=L, trace=trace, air=(cons, exempt, periodic, boundary), shift=rng.nonzero(p))
    prof = oc.profile if profile else (lambda _ctx, fn: (fn(), None))
    rc, P["trace_root"] = ctx.trace_commit(trace, c)
    assert rc == 0 and ctx.interpolate() == 0, ctx.last_error()
    (rc, P["lde_root"]), P["prof_lde"] = prof(ctx, lambda: ctx.lde_commit(BLOWUP, P["shift"], c))
    assert rc == 0, ctx.last_error()
    P["r"] = dc.full_ext(rng, field)
    rc, P["prof_mix"] = prof(ctx, lambda: ctx.mix_air_ext(P["r"], cons, exempt, periodic, boundary))
    assert rc == 0, ctx.last_error()
    P["VL"] = dc.vl_of(ctx)
    P["m"] = m = e * P["VL"] // N
    (rc, P["val_root"]), P["prof_val"] = prof(ctx, lambda: ctx.validity_commit(m))
    assert rc == 0, ctx.last_error()
    P["z"] = z = dc.full_ext(rng, field)
    P["rows"] = rows = ms.air_rows(cons, boundary)
    P["zs"] = dc.shifted_points(field, z, ctx.root_of_unity(N), rows)
    P["lists"] = [list(range(c)) + (list(range(c, c + m)) if k == 0 else []) for k in range(len(rows))]
    rc, ev = ctx.deep_evals(P["zs"], P["lists"])
    assert rc == 0, ctx.last_error()
    P["evals"] = dc.tuples(ev)
    P["gamma"] = dc.full_ext(rng, field)
    assert ctx.deep_compose(P["zs"], P["lists"], P["gamma"]) == 0, ctx.last_error()
    P["R"] = R = L.bit_length() - 1 - 2                                      # D_(R-1) = L / 2^(R-1) = 8
    P["S"], P["prof_fri"] = prof(ctx, lambda: oc.commit_phase(ctx, field, BLOWUP, R, seed=6001))
    P["infos"] = [ctx.fri_round_info(i) for i in range(R)]
    P["betas"] = beta_set(P["S"]["D0"])
    P["mslq"] = ctx.query_linked(P["betas"])
    return P


def pinned(P):
    """what a knob must leave alone: every root, the evaluations, the B values, the round shapes and the query phase's bytes"""
    return dict(trace_root=P["trace_root"], lde_root=P["lde_root"], val_root=P["val_root"], evals=P["evals"], roots=P["S"]["roots"], Bs=P["S"]["Bs"], infos=P["infos"],
                mslq=P["mslq"])


def case_stage_ledger(make, d, field, N, flags=0, env=None, name="cubic", roots_only=False):
    """every intermediate of `drive` read back and checked whole; returns `drive`'s dict (closed context).  roots_only: the commitments, the profile and the query
    phase only (the other digests of shape B: the field arithmetic does not depend on the digest)"""
    p, e = MODULUS[field], EXT[field]
    T = rd.tower(field)
    ctx = oc.ctx_of(make, d, field, extra=flags, env=env)
    P = drive(ctx, d, field, N, name)
    c, m, L, shift, trace = P["c"], P["m"], P["L"], P["shift"], P["trace"]
    cons, exempt, periodic, boundary = P["air"]
    rng = SplitMix64(7001 + N)
    small = N <= SHAPES["A"]
    # ---- trace and LDE
    polys = [ctx.poly_read(j) for j in range(c)]
    for j in range(c):
        assert np.array_equal(polys[j], oracle.intt(field, trace[:, j])), j
    lde = ctx.lde_read()
    assert lde.shape == (L, c)
    for j in range(c):
        assert np.array_equal(lde[:, j], oracle.coset_lde(field, polys[j], shift, L)), j
    lde_nodes = ro.tree_nodes(d, lde.reshape(-1, 1), 1, c)
    assert bytes(lde_nodes[-1]) == P["lde_root"]
    # ---- validity polynomial: chunk columns, tree, openings
    v = ctx.validity_read()
    assert v.shape == (P["VL"], e) and ctx.validity_ext() == e and all(v[:, l].any() for l in range(e))
    chunks = [np.ascontiguousarray(v[k * N:(k + 1) * N, l]) for k in range(P["VL"] // N) for l in range(e)]
    assert len(chunks) == m
    vmat = np.ascontiguousarray(np.stack([oracle.coset_lde(field, col, shift, L) for col in chunks], axis=1))
    val_nodes = ro.tree_nodes(d, vmat.reshape(-1, 1), 1, m)
    assert bytes(val_nodes[-1]) == P["val_root"]
    for ix in oc.index_lists(L):
        oc.check_paths(ctx, d, field, ctx.tree_open(ms.TREE_VALIDITY, ix), vmat.reshape(-1, 1), 1, m, val_nodes, P["val_root"], ix)
    cols = [col.tolist() for col in polys] + [col.tolist() for col in chunks]     # F_0 .. F_(c+m-1) as Python integers
    if small:
        assert cols[c:] == rd.chunk_columns(dc.val_rows(ctx), e, N)
    # ---- every round: codeword = NTT of the polynomial, root = tree of the codeword (ext = E, lpn = 2)
    S, R, infos = P["S"], P["R"], P["infos"]
    D0 = S["D0"]
    assert D0 == L and infos[R - 1][1] == 8 and [D for _, D in infos] == [D0 >> i for i in range(R)]
    rpolys, cws, fnodes = [], [], []
    for i in range(R):
        nc, D = infos[i]
        f = ctx.fri_round_poly(i)
        assert f.shape == (nc, e) and (nc == 0 or f[nc - 1].any())           # exactly the trimmed length
        cw = ctx.fri_round_codeword(i)
        assert cw.shape == (D, e)
        for l in range(e):
            padded = np.zeros(D, dtype=np.uint64)
            padded[:nc] = f[:, l]
            assert np.array_equal(cw[:, l], oracle.ntt(field, padded)), (i, l)
        nodes = ro.tree_nodes(d, cw, e, 2)
        assert bytes(nodes[-1]) == S["roots"][i], i
        rpolys.append(f); cws.append(cw); fnodes.append(nodes)
    assert all(cws[0][:, l].any() for l in range(e)) and 0 < infos[0][0] <= N - 1   # an E-limb round 0
    # ---- profile
    check_commit_profile(field, P["prof_fri"], infos)
    for prof in (P["prof_lde"], P["prof_val"]):                              # trees of L leaf groups
        assert launches(prof).get("inner_hash", 0) == sum(inner_launches(L)), launches(prof)
    assert (inner_launches(L)[0] > 0) == (L // 2 > SUBTREE_PARENTS)          # from shape B on: a level launch in front of the subtree launches
    logL = L.bit_length() - 1
    assert_reached(P["prof_mix"], COOP_MIX[field, logL])
    assert launches(P["prof_mix"]).get("mix_air_ext") == 1
    for key in ("prof_lde", "prof_val", "prof_fri"):
        if (field, logL) in COOP_FORWARD:
            assert_reached(P[key], COOP_FORWARD[field, logL])
        else:                                                                # a plan change that makes these cooperative earlier belongs in the table above
            assert not any(name.startswith("msntt::PassKernel2<") for name in P[key]["ntt_pass_variants"]), (key, sorted(P[key]["ntt_pass_variants"]))
    # ---- query phase: the definition, and every path cut from the reference trees
    betas = P["betas"]
    assert betas[0] % D0 >= D0 // 2 and betas[0] == betas[2]
    assert P["mslq"] == lc.by_definition(ctx, betas, D0, L)
    sec = lc.rl.split_mslq(P["mslq"])
    assert sec is not None
    rows = rd.link_rows(betas, D0, L)
    assert sec[0] == ro.msfi_blob(e, cws, fnodes, rpolys[-1], betas)
    assert sec[1] == b"".join(ro.path_at(lde.reshape(-1, 1), 1, c, lde_nodes, g) for g in rows)
    assert sec[2] == b"".join(ro.path_at(vmat.reshape(-1, 1), 1, m, val_nodes, g) for g in rows)
    if roots_only:
        ctx.close()
        return P
    # ---- validity polynomial: its definition at random points of K (both sides multiplied out have degree < 4N)
    omega = ctx.root_of_unity(N)
    assert omega == pyref.root_of_unity(field, N)
    vplanes = [v[:, l].tolist() for l in range(e)]
    for k in range(points_for(Fraction(4 * N, p**e))):
        zz = dc.full_ext(rng, field)
        want = rhs_at(field, omega, N, cols, P["r"], P["air"], zz)
        assert ext_at_point(T, vplanes, power_planes(T, zz, P["VL"])) == want
        if small and k == 0:
            assert want == rx.rhs_at(field, omega, N, cols[:c], P["r"], cons, exempt, periodic, boundary, zz)
            assert want == rx.horner_ext(T, dc.tuples(v), zz)
    # ---- DEEP evaluations
    tables = [power_planes(T, zt, N) for zt in P["zs"]]
    assert P["evals"] == [at_point(p, cols[j], tables[t]) for t, lst in enumerate(P["lists"]) for j in lst]
    if small:
        assert P["evals"] == rd.deep_evals(field, cols, P["zs"], P["lists"])
    # ---- DEEP polynomial: D'(y) = D(shift y) is the composition of the columns' values at x = shift y, at random base-field y off the coset.  Multiplied by the
    # prod_t (x - z_t) both sides are polynomials of degree < N + npts
    f0 = [rpolys[0][:, l].tolist() for l in range(e)]
    npts = points_for(Fraction(N + len(P["zs"]), p))
    assert npts >= (2 if field == 0 else 4)
    for _ in range(npts):
        y = rng.nonzero(p)
        while pow(y, L, p) == 1:
            y = rng.nonzero(p)
        x = shift * y % p
        got = tuple(base_horner(p, plane, y) for plane in f0)
        assert got == rd.composition_at(field, [base_horner(p, col, x) for col in cols], P["evals"], P["zs"], P["lists"], P["gamma"], x)
    # ---- every round: B = (even(z), odd(z)); the next polynomial is the exact quotient
    for i in range(R - 1):
        f = dc.tuples(rpolys[i])
        z, alpha = S["zs"][i], S["alphas"][i]
        planes = power_planes(T, z, (len(f) + 1) // 2)
        even = ext_at_point(T, [rpolys[i][0::2, l].tolist() for l in range(e)], planes)
        odd = ext_at_point(T, [rpolys[i][1::2, l].tolist() for l in range(e)], planes)
        assert S["Bs"][i] == (even, odd), i
        if small and i == 0:
            assert even == pyref.peval(T, f[0::2], z) and odd == pyref.peval(T, f[1::2], z)
        assert dc.tuples(rpolys[i + 1]) == next_round_poly(T, f, alpha, z, S["Bs"][i]), i
    # the sampled verifiers accept what the ledger pinned
    Q = dict(P, msfi=sec[0], lde_open=sec[1], val_open=sec[2], blowup=BLOWUP)
    assert dc.fri_ok(Q) == 1 and dc.link(Q) == (1, "", "")
    ctx.close()
    return P


# ---------------------------------------------------------------- knob invariance
KNOBS = {"tail_off": (0, {"MS_FRI_TAIL_MAX": "0"}), "fold_wg": (0, {"MS_FOLD_SMALL_MAX": "0"}), "transform": (0, {"MS_FRI_POINTWISE": "0"}),
         "levels": (0, {"MS_TREE_SUBTREE_PARENTS": "0"}), "latency": (LATENCY, None)}


def case_knob(make, d, field, N, knob, base):
    """the state of `drive` under one setting: every root, B, round shape and the MSLQ bytes are the default context's (`base`: the ledger's dict), and the profile shows
    the launches the knob is meant to move.  MS_FOLD_SMALL_MAX=0 swaps FriFoldEvalKernel for FriFoldWgKernel inside the class "fold": the profile counts both alike,
    so only the unchanged counts are asserted there.  MS_FLAG_LATENCY runs WITHOUT the profile: under it the coefficient side stays on the context's stream."""
    flags, env = KNOBS[knob]
    ctx = oc.ctx_of(make, d, field, extra=flags, env=env)
    P = drive(ctx, d, field, N, profile=knob != "latency")
    ctx.close()
    assert pinned(P) == pinned(base), knob
    if knob == "latency":
        return
    R, infos = P["R"], P["infos"]
    got, ref = launches(P["prof_fri"]), launches(base["prof_fri"])
    folding = sum(1 for i in range(1, R) if infos[i - 1][0] >= 3)            # rounds with a coefficient side (m >= 2)
    if knob == "tail_off":
        assert "fri_tail" not in got and ref["fri_tail"] > 0
        assert got["fold"] == (R - 1) + folding and got["degree"] == 1 + folding and got["fold"] > ref["fold"]
    elif knob == "fold_wg":
        assert got == ref
    elif knob == "transform":
        assert "fri_tail" not in got and got["fold"] == folding              # no pointwise fold at all: every codeword by transform
        assert got["ntt_pass"] > ref["ntt_pass"] and got["ntt_pass"] >= R
    elif knob == "levels":
        assert got["inner_hash"] > ref["inner_hash"]
        for key in ("prof_lde", "prof_val"):
            assert launches(P[key])["inner_hash"] > launches(base[key])["inner_hash"], key
        assert {k: n for k, n in got.items() if k != "inner_hash"} == {k: n for k, n in ref.items() if k != "inner_hash"}


# ---------------------------------------------------------------- the staged tree
def case_staged_ledger(make, d, field, N, which="permutation"):
    """ms_aux_running_staged / ms_lde_commit_stage: the running column satisfies the recurrence of its definition, its polynomials are the inverse transform of its limbs,
    its LDE columns their coset evaluation, and the MS_TREE_LDE_STAGED root is the tree over those columns alone"""
    p, e = MODULUS[field], EXT[field]
    rows, _main, op, fr = sc.CASES[which](field, N, 700 + N + field)
    w, L = len(rows[0]), N * BLOWUP
    shift = SplitMix64(800 + N).nonzero(p)
    ctx = oc.ctx_of(make, d, field)
    out, root0, root1 = sc.staged(ctx, rows, [(op, fr)], BLOWUP, shift)
    final, col = out[0]
    assert rax.check_recurrence(field, e, op, fr, rows, [tuple(x) for x in col], final)
    assert tuple(final) == tuple(sc.k_of(field, 1 if op == sc.PRODUCT else 0))   # the argument closes
    colarr = np.array(col, dtype=np.uint64)
    polys = [ctx.poly_read(w + l) for l in range(e)]
    for l in range(e):
        assert np.array_equal(polys[l], oracle.intt(field, colarr[:, l])), l
    lde = ctx.lde_read()
    assert lde.shape == (L, w + e)
    for l in range(e):
        assert np.array_equal(lde[:, w + l], oracle.coset_lde(field, polys[l], shift, L)), l
    values = np.ascontiguousarray(lde[:, w:]).reshape(-1, 1)
    nodes = ro.tree_nodes(d, values, 1, e)
    assert bytes(nodes[-1]) == root1 != root0
    nodes0 = ro.tree_nodes(d, np.ascontiguousarray(lde[:, :w]).reshape(-1, 1), 1, w)
    assert bytes(nodes0[-1]) == root0
    for ix in oc.index_lists(L):
        oc.check_paths(ctx, d, field, ctx.tree_open(ms.TREE_LDE_STAGED, ix), values, 1, e, nodes, root1, ix)
    ctx.close()
