"""CPU tests: the oracle against the reference's own KATs / fixtures, against
hashlib, and against the independent big-int restatement in tests/pyref.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import pyref
from common import GL_P, BB_P, MODULUS, EXT, SplitMix64, fibonacci_trace, fibonacci_closures
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
L = orc.lib()
import ctypes as C


# ---- src/util.rs:50-96 ------------------------------------------------------
def test_util_is_power_of_two():
    for v in (0, 1, 2, 32, 128, 512, 1024):
        assert L.or_is_power_of_two(C.c_uint64(v))
    for v in (24, 48):
        assert not L.or_is_power_of_two(C.c_uint64(v))


def test_util_logarithm_of_two_k():
    f = lambda n, b: L.or_logarithm_of_two_k(C.c_uint64(n), C.c_uint64(b))
    NOT2, NOT2K = -1, -2
    assert f(32, 2) == 5 and f(6, 2) == NOT2
    assert f(256, 4) == 4 and f(12, 4) == NOT2 and f(32, 4) == NOT2K
    assert f(512, 8) == 3 and f(15, 8) == NOT2 and f(16, 8) == NOT2K
    assert f(256, 16) == 2 and f(48, 16) == NOT2 and f(64, 16) == NOT2K


def test_util_ceil_log2_k():
    f = lambda n, b: L.or_ceil_log2_k(C.c_uint64(n), C.c_uint64(b))
    assert f(2, 2) == 1 and f(21, 2) == 5 and f(32, 2) == 5
    assert f(4, 4) == 2 and f(3, 4) == 2 and f(13, 4) == 4 and f(21, 4) == 6


# ---- src/starks.rs:341-374 ----------------------------------------------------
def test_num_queries_kats():
    assert orc.num_queries(0, 1, 4, 128)[0] == orc.ERR_SHAPE  # <20 bits panics
    assert orc.num_queries(0, 20, 4, 129) == (0, 1, 3)
    assert orc.num_queries(0, 20, 2, 9) == (0, 1, 10)
    assert orc.num_queries(0, 128, 4, 129) == (0, 3, 19)
    assert orc.num_queries(0, 256, 4, 513) == (0, 5, 32)


# ---- src/merkle.rs:384-481 ------------------------------------------------------
LEAFS16 = np.arange(16, dtype=np.uint64)


def test_merkle_not_full_tree_errors():
    rc, _, _ = orc.merkle_build(np.arange(3, dtype=np.uint64), 1, 2, 2)
    assert rc == orc.ERR_SHAPE
    rc, _, _ = orc.merkle_build(np.zeros(0, dtype=np.uint64), 1, 2, 2)
    assert rc == orc.ERR_SHAPE


@pytest.mark.parametrize("lpn,ic,nnodes", [(2, 2, 15), (4, 2, 7), (4, 4, 5), (16, 16, 1)])
def test_merkle_node_calculation(lpn, ic, nnodes):
    rc, nodes, root = orc.merkle_build(LEAFS16, 1, lpn, ic)
    assert rc == 0 and len(nodes) == nnodes and bytes(nodes[-1]) == root


def test_merkle_parent_index():
    two = {1: 16, 4: 18, 9: 20, 13: 22, 16: 24, 18: 25, 20: 26, 22: 27, 24: 28, 25: 28, 26: 29, 27: 29, 28: 30, 29: 30}
    for i, parent in two.items():
        assert orc.merkle_parent_idx(16, 2, 2, i) == (0, parent)
    two_four = {1: 16, 4: 17, 9: 18, 13: 19, 16: 20, 17: 20, 18: 21, 19: 21, 20: 22, 21: 22}
    for i, parent in two_four.items():
        assert orc.merkle_parent_idx(16, 4, 2, i) == (0, parent)
    assert orc.merkle_parent_idx(16, 4, 2, 23)[0] == orc.ERR_OUT_OF_RANGE
    assert orc.merkle_parent_idx(16, 4, 2, 22)[0] == orc.ERR_OUT_OF_RANGE  # root


@pytest.mark.parametrize("lpn,plen", [(2, 3), (4, 2)])
def test_merkle_check_proof(lpn, plen):
    rc, nodes, root = orc.merkle_build(LEAFS16, 1, lpn, 2)
    rc, path = orc.merkle_prove(LEAFS16, [7], 1, lpn, 2)
    assert rc == 0
    neigh = np.frombuffer(path[8:8 + 8 * lpn], dtype=np.uint64)
    assert 7 in neigh
    nlev = int(np.frombuffer(path[8 + 8 * lpn:16 + 8 * lpn], dtype=np.uint64)[0])
    assert nlev == plen
    assert orc.merkle_check_proof(root, path, 1, lpn, 2)
    bad = bytearray(path); bad[-1] ^= 1
    assert not orc.merkle_check_proof(root, bytes(bad), 1, lpn, 2)
    assert orc.merkle_prove(LEAFS16, [99], 1, lpn, 2)[0] == orc.ERR_LEAF_NOT_FOUND


# ---- golden vectors produced by the reference's scripts/merkle_tree.py --------
def test_merkle_script_golden_roots():
    g = json.load(open(os.path.join(HERE, "golden", "merkle_script_roots.json")))
    t = g["tree"]
    for v in g["vectors"]:
        leafs = np.array([int(x) for x in v["leafs"]], dtype=np.uint64)
        rc, nodes, root = orc.merkle_build(leafs, 1, t["leafs_per_node"], t["inner_children"], t["zero_as_empty"])
        assert rc == 0
        assert [bytes(n).hex() for n in nodes[:8]] == v["leaf_digests"], v["name"]
        assert root.hex() == v["root"], v["name"]


def test_sha256_vs_hashlib():
    rng = np.random.default_rng(1)
    for n in list(range(0, 130)) + [191, 192, 1000]:
        m = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert orc.sha256(m) == hashlib.sha256(m).digest()


# ---- field constants (src/field.rs:44-45,73-74) -----------
def test_roots_of_unity():
    assert orc.modulus(0) == GL_P and orc.modulus(1) == BB_P
    assert orc.root_of_unity(0, 1 << 32) == 1753635133440165772
    assert orc.root_of_unity(1, 1 << 27) == 291241980  # quirk Q8, not 440564289
    for f in (0, 1):
        for k in (1, 4, 5, 20, 23, 24, 27):
            w = orc.root_of_unity(f, 1 << k)
            assert w == pyref.root_of_unity(f, 1 << k)
            assert pow(w, 1 << k, MODULUS[f]) == 1 and pow(w, 1 << (k - 1), MODULUS[f]) == MODULUS[f] - 1


@pytest.mark.parametrize("field,ext", [(0, 1), (0, 2), (1, 1), (1, 2), (1, 4)])
def test_ext_arithmetic_vs_bigint(field, ext):
    T = pyref.Tower(field, ext)
    rng = SplitMix64(7 + field * 10 + ext)
    p = MODULUS[field]
    for _ in range(50):
        a = [rng.field(p) for _ in range(ext)]
        b = [rng.field(p) for _ in range(ext)]
        assert tuple(int(x) for x in orc.ext_mul(field, ext, a, b)) == T.mul(tuple(a), tuple(b))
        if any(a):
            ai = orc.ext_inv(field, ext, a)
            assert T.mul(tuple(a), tuple(int(x) for x in ai)) == T.one()
    if field == 1 and ext == 4:
        # v^2 == (2013265910 + u)  (src/field.rs:98)
        v = (0, 0, 1, 0)
        assert tuple(int(x) for x in orc.ext_mul(1, 4, v, v)) == (2013265910, 1, 0, 0)


def test_display_strings():
    assert orc.display(1, [0]) == b"" and orc.display(1, [0], 0) == b"0"
    assert orc.display(1, [GL_P - 1, 5]) == b"184467440694145843205"
    assert orc.display(2, [3, 0]) == b"QuadExtField(3 +  * u)"
    assert orc.display(4, [1, 2, 3, 4]) == b"QuadExtField(QuadExtField(1 + 2 * u) + QuadExtField(3 + 4 * u) * u)"
    assert orc.display(2, [1, 2, 3, 4]).decode() == pyref.display((1, 2)) + pyref.display((3, 4))


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_ntt_vs_definition(field, n):
    rng = SplitMix64(n + field)
    a = [rng.field(MODULUS[field]) for _ in range(n)]
    assert list(map(int, orc.ntt(field, a))) == pyref.dft(field, a)
    assert list(map(int, orc.intt(field, a))) == pyref.dft(field, a, inverse=True)
    assert list(map(int, orc.intt(field, orc.ntt(field, a)))) == a


@pytest.mark.parametrize("field", [0, 1])
def test_coset_lde_vs_definition(field):
    rng = SplitMix64(3)
    p = MODULUS[field]
    coeffs = [rng.field(p) for _ in range(8)]
    shift = rng.nonzero(p)
    assert list(map(int, orc.coset_lde(field, coeffs, shift, 32))) == pyref.coset_eval(field, coeffs, shift, 32)


def test_intt_property_air_rs_306():
    """src/air.rs:306-321: trace_polys[c].evaluate(domain.element(i)) == trace[i][c]."""
    N = 16
    t = fibonacci_trace(0, N)
    s = orc.Session(0)
    assert s.trace_commit(t, 6)[0] == 0 and s.interpolate() == 0
    g = orc.root_of_unity(0, N)
    for c in range(3):
        poly = [int(x) for x in s.poly_read(c)]
        for i in range(N):
            x = pow(g, i, GL_P)
            acc = 0
            for cf in reversed(poly):
                acc = (acc * x + cf) % GL_P
            assert acc == int(t[i, c])


def run_both(field, N, blowup, nq_fri, seed, zae=1, trace=None, challenges=None, rounds=None):
    """Drives oracle Session and PyProver with identical inputs; returns per-stage outputs.  `trace`: another N x 3 trace than the Fibonacci one; `challenges`:
    explicit values (structured_cases.random_challenges' keys: shift, r, ood, per-round z and alpha, betas) instead of the draws from SplitMix64(seed); `rounds`:
    another FRI round count than the config's."""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(seed)
    ch = challenges or {}
    t = fibonacci_trace(field, N) if trace is None else trace
    omega = orc.root_of_unity(field, N)
    cl = fibonacci_closures(field, N, omega)
    o = orc.Session(field, zae)
    y = pyref.PyProver(field, bool(zae))
    out = []
    rc, root = o.trace_commit(t, 6)
    assert rc == 0
    out.append((root, y.trace_commit(t, 6)))
    assert o.interpolate() == 0
    y.interpolate()
    for sc, idx in cl:
        assert o.polys_lincomb(sc, idx) == 0
        y.lincomb(sc, idx)
    for i in range(6):
        out.append((list(map(int, o.poly_read(i))), y.polys[i]))
    shift = rng.nonzero(p)
    shift = ch.get("shift", shift)
    rc, root = o.lde_commit(blowup, shift, 6)
    assert rc == 0
    out.append((root, y.lde_commit(blowup, shift, 6)))
    out.append((o.lde_read().tolist(), y.lde))
    r = rng.field(p)
    r = ch.get("r", r)
    assert o.mix(r) == 0
    y.mix(r)
    out.append((list(map(int, o.validity_read())), y.validity))
    zs = [[rng.field(p) for _ in range(e)] for _ in range(2)]
    zs = ch.get("ood", zs)
    rc, ev = o.eval_ext(np.array(zs, dtype=np.uint64))
    assert rc == 0
    out.append((ev.tolist(), [[list(v) for v in row] for row in y.eval_ext(zs)]))
    if rounds is None:
        rounds = int(L.or_ceil_log2_k(C.c_uint64((N - 1) * blowup + 1), C.c_uint64(2)))
    rc, root = o.fri_begin(blowup, rounds)
    assert rc == 0
    out.append((root, y.fri_begin(blowup, rounds)))
    for i in range(1, rounds):
        z = [rng.field(p) for _ in range(e)]
        if "z" in ch:
            z = ch["z"][(i - 1) % len(ch["z"])]
        rc, B = o.fri_deep(z)
        assert rc == 0
        By = y.fri_deep(z)
        out.append((B.reshape(2, e).tolist(), [list(b) for b in By]))
        al = [rng.field(p) for _ in range(e)]
        if "alpha" in ch:
            al = ch["alpha"][(i - 1) % len(ch["alpha"])]
        rc, root = o.fri_fold_commit(al)
        assert rc == 0
        out.append((root, y.fri_fold_commit(al)))
    for i in range(rounds):
        out.append((o.fri_round_poly(i).tolist(), [list(c) for c in y.rounds[i]["poly"]]))
        out.append((o.fri_round_info(i)[1], y.rounds[i]["D"]))
    betas = [rng.next() for _ in range(nq_fri)] + [3, 2 * N * blowup]  # small + wrap-around cases (Q6)
    betas = ch.get("betas", betas)
    rc, proof = o.fri_query(betas)
    assert rc == 0
    out.append((proof, y.serialise_fri(y.fri_query(betas))))
    return out


@pytest.mark.parametrize("field,N,blowup", [(0, 16, 2), (0, 8, 8), (1, 8, 2), (1, 16, 4)])
def test_prove_oracle_vs_bigint(field, N, blowup):
    for i, (a, b) in enumerate(run_both(field, N, blowup, 2, seed=1234 + N)):
        assert a == b, f"stage output {i} differs"


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["zero", "const", "deg1", "len5", "half+3", "even", "odd", "mono_top", "gap"])
def test_prove_oracle_vs_bigint_structured(field, name):
    """The oracle against the big-integer restatement where the validity polynomial is low-degree, sparse or zero (tests/structured_cases.py) - trimmed lengths,
    the domain sizes they give, ragged even / odd halves, a fold that vanishes, equal values under two leaves - with random alpha, alpha = 0 and base-field z."""
    import structured_cases as sc
    N, blowup = 16, 4
    trace = sc.trace_from_support(field, N, sc.SUPPORTS[name](N), seed=50 + field)
    for mode in sc.MODES:
        ch = sc.random_challenges(field, seed=60 + sc.MODES.index(mode), mode=mode)
        _, D0 = sc.oracle_round0(field, trace, blowup, ch["r"])
        ch["betas"] = ch["betas"][:1] + [0, 3, D0 // 2 + 1, D0, 2 * N * blowup]
        for i, (a, b) in enumerate(run_both(field, N, blowup, 0, seed=1, trace=trace, challenges=ch, rounds=D0.bit_length() - 1)):
            assert a == b, f"{mode}: stage output {i} differs"


def test_fri_roundtrip_fri_rs_426():
    """src/fri.rs:426-454: coeffs 0..3 over GoldilocksFp2, rounds 3, blowup 2, prove -> verify."""
    for field, ext in [(0, 2), (0, 1), (1, 4)]:
        p = MODULUS[field]
        s = orc.Session(field, 1, ext=ext)
        # load validity = [0,1,2,3] through the session: trace_commit + interpolate path is
        # base-only, so feed coefficients as a 4x1 "trace" whose INTT we overwrite via lincomb.
        t = np.array([[0], [1], [2], [3]], dtype=np.uint64)
        ev = orc.ntt(field, t[:, 0])  # evaluations whose INTT is 0,1,2,3
        assert s.trace_commit(ev.reshape(4, 1), 1)[0] == 0
        assert s.interpolate() == 0
        assert list(map(int, s.poly_read(0))) == [0, 1, 2, 3]
        assert s.mix(1) == 0
        rounds, rng = 3, SplitMix64(99)
        rc, root0 = s.fri_begin(2, rounds)
        roots, zs, Bs, als = [root0], [], [], []
        for _ in range(1, rounds):
            z = [rng.field(p) for _ in range(ext)]
            rc, B = s.fri_deep(z); assert rc == 0
            al = [rng.field(p) for _ in range(ext)]
            rc, root = s.fri_fold_commit(al); assert rc == 0
            zs += z; Bs += list(map(int, B)); als += al; roots.append(root)
        betas = [rng.next()]
        rc, proof = s.fri_query(betas); assert rc == 0
        # the verifier checks round i's openings against commits[i] = root of round i
        # (fri.rs:237 uses commits[i] read from the transcript = rounds 1..)
        ok = orc.fri_verify(field, ext, rounds, betas, zs, Bs, als, b"".join(roots), proof)
        assert ok == 1
        bad = bytearray(proof); bad[8 * ext] ^= 1  # corrupt y1
        assert orc.fri_verify(field, ext, rounds, betas, zs, Bs, als, b"".join(roots), bytes(bad)) == 0


def test_oracle_matches_committed_proof_digests():
    """tests/golden/oracle_proof_digests.json (generated by tests/golden/gen_oracle_proof_digests.py from this oracle, not from the
    reference): every stage output of nine small proofs is frozen."""
    import importlib.util
    import json
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("gen_digests", os.path.join(here, "golden", "gen_oracle_proof_digests.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(here, "golden", "oracle_proof_digests.json")))
    for f, n, b, s in gen.CASES:
        assert gen.digest_of(f, n, b, s) == want[f"{f}-{n}-{b}-{s}"], (f, n, b, s)


def test_oracle_openmp_matches_single_thread():
    """or_set_threads only changes how the oracle's independent loops are scheduled: same bytes out."""
    import parity_cases as pc
    from common import fibonacci_trace_fast
    for field, log_n in ((0, 13), (1, 12)):
        tr = fibonacci_trace_fast(field, 1 << log_n)
        one = pc.drive(orc.Session(field), field, tr, 8, 1, seed=4, read_big=False)
        orc.set_threads(4)
        try:
            many = pc.drive(orc.Session(field), field, tr, 8, 1, seed=4, read_big=False)
        finally:
            orc.set_threads(1)
        assert one == many
