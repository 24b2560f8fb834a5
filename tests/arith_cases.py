"""Field-arithmetic corners, shared by tests/test_arith_emu.py (the emulation build) and tests/test_arith_gpu.py (the HIP build): ms_arith_selftest
(`op` = operation | class << 8, include/ministark.h) under every arithmetic class of csrc/field.hpp - GL compare + select, GLT sign bits through
v_bitop3_b32, GLM exec-masked inline asm, BB Montgomery - and the extension towers, against Python integers and tests/pyref.py: Tower.

The corrections that make a result canonical sit on branches that uniform operands take with probability about 2^-32, so the operands here are DIRECTED:
all pairs of an edge set, and the (lo, hi) words of their full products.  How often each branch of each operation is taken is counted from the big-integer
computation alone (coverage(), never from the code under test) and asserted, so that a change of the edge set cannot hollow the tests silently.
`mk(field)` returns a mini_stark_amd.Context."""
import collections
import ctypes as C
import functools
import itertools

import numpy as np

import pyref
from common import MODULUS

P, Q = MODULUS[0], MODULUS[1]
M64, M32, EPS = (1 << 64) - 1, (1 << 32) - 1, (1 << 32) - 1
ERR_ARG = -5
GL_CLASSES = {1: "GL", 2: "GLT", 3: "GLM"}


# ---------------------------------------------------------------- operands
@functools.lru_cache(None)
def gl_edge():
    v = [0, 1, 2, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**33 - 1, 2**63 - 1, 2**63, 2**63 + 1, 0x7FFFFFFF80000000, 0x7FFFFFFF80000001,
         0x80000000FFFFFFFF, 0xFFFFFFFE00000000, 0xFFFFFFFE00000001, 0xFFFFFFFE00000002, 0xFFFFFFFEFFFFFFFF, 0xFFFFFFFF00000000, P - 2, P - 1]
    for k in range(1, 64):
        v += [2**k - 1, 2**k, P - 2**k, P - 2**k + 1, P - 2**k - 1]
    return tuple(x % P for x in v)      # 338 entries; a few values occur twice (2^31 - 1, 2^32 - 1, 2^63 ...), which costs nothing and keeps the count of pairs


@functools.lru_cache(None)
def bb_edge():
    R = (1 << 32) % Q
    # the list of parity_cases.case_arith_selftest (the Montgomery constants of the table multiply among them) ...
    v = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, 1 << 30, (1 << 30) - 1, 0x77FFFFFF, 0x78000000, 0x78000001 % Q, 1172168163,
         R, R * R % Q, Q - R, (1 << 31) % Q, pow(R, -1, Q), Q - pow(R, -1, Q), (Q - 1) * pow(R, -1, Q) % Q]
    for k in range(1, 31):   # ... and every power of two from both ends
        v += [2**k - 1, 2**k, Q - 2**k, Q - 2**k + 1, Q - 2**k - 1]
    return tuple(dict.fromkeys(x % Q for x in v))


def all_pairs(vals):
    return [x for x in vals for _ in vals], [y for _ in vals for y in vals]


@functools.lru_cache(None)
def rand_words(n, seed):
    """n uniform 64-bit words as Python integers"""
    rng = np.random.RandomState(seed)
    w = rng.randint(0, 1 << 32, size=n, dtype=np.int64).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, size=n, dtype=np.int64).astype(np.uint64)
    return tuple(int(x) for x in w)


def rand_field(p, n, seed):
    return [x % p for x in rand_words(n, seed)]


def u64(v):
    return np.array(v, dtype=np.uint64)


# ---------------------------------------------------------------- branch predicates, from integers alone
def add_class(a, b):
    s = a + b
    return "carry" if s >> 64 else ("ge_p" if s >= P else "neither")


def sub_class(a, b):
    return "lt" if a < b else ("eq" if a == b else "gt")


def reduce_class(lo, hi):
    """(borrow of lo - hi_hi)(carry of + hi_lo * EPS)(r >= p) of a 128-bit value: GL / GLT::reduce128's three decisions.  Reachable: 000 001 010 101 110.
    011: a wrapped sum is below hi_lo * EPS <= (2^32 - 1)^2 < p.  100, 111: a borrowed lo - hi_hi + 2^64 is at least p, so r >= p exactly when the sum does not wrap."""
    hh, hl = hi >> 32, hi & EPS
    A = (lo - hh) & M64
    s = A + hl * EPS
    return "%d%d%d" % (lo < hh, s >> 64, (s & M64) >= P)


REDUCE_CLASSES = ("000", "001", "010", "101", "110")


def words(x):
    return x & M64, x >> 64


def wrap_class(s):
    return "wrap" if s >> 64 else ("ge_p" if s >= P else "neither")


def fold_small_class(a, b):
    """A + h EPS with h < 2^31: wrapped / >= p / neither.  (">= p" needs A >= 2^63 + 2^31, since h EPS <= (2^31 - 1)(2^32 - 1): with A's top bit clear the sum stays below
    2^64 - 2^32 - 2^31 + 1 < p.  So entry 2 of GLT::fold_small's truth table 0x74 - A's top bit clear, r's set, t's clear - is never selected, and a table 0x70 computes
    the same function on every input the contract allows: no test can tell the two apart.)"""
    return wrap_class(a + (b & 0x7FFFFFFF) * EPS)


def mul_x32_class(z):
    return wrap_class(((z & M32) << 32) + (z >> 32) * EPS)


def mul_x64_class(z):
    return "borrow" if (z & M32) * EPS < (z >> 32) else "none"


BB_MU = 0x77FFFFFF      # -1 / p mod 2^32


def bb_t(x):
    """the intermediate t of BB::redc(x) (t < 2 p; the result is t or t - p)"""
    m = (x & M32) * BB_MU & M32
    assert (x + m * Q) & M32 == 0
    return (x + m * Q) >> 32


@functools.lru_cache(None)
def bb_montgomery_pairs():
    """Pairs (a, b) whose FIRST reduction in BB::mul (x = a b) has t = 0, p - 1 (the largest t that takes no correction), p + 1 (the smallest reachable one that
    takes it) and residues around them, built from MU and R: t == x / R (mod p), so x = t R mod p + j p for the j >= 0 that makes x a product of two
    canonical values, and t grows with j by one p at most.
    t = p and t = 2 p - 1 are UNREACHABLE from canonical operands, in every reduction of the library: t == 0 (mod p) needs p | x, and x = a b with a, b < p prime
    is then 0 (t = 0); and t <= ((p - 1)^2 + (2^32 - 1) p) >> 32 < 1.47 p < 2 p - 1 (bb_coverage asserts both)."""
    R = (1 << 32) % Q
    out = [(0, 0), (0, Q - 1), (Q - 1, 0), (0, 1)]
    for rho in (Q - 1, 1, 2, Q - 2, 3):
        x0 = rho * R % Q
        for b in range(1, 96):
            j = (-x0 * pow(Q, -1, b)) % b if b > 1 else 0
            for jj in (j, j + b):
                x = x0 + jj * Q
                if x % b == 0 and x // b < Q:
                    out.append((x // b, b))
                    out.append((b, x // b))
    # the same products in front of the ONE reduction of mul_tw(a, to_tw(b)), x = a (b R mod p): b / R in b's place
    Ri = pow(R, -1, Q)
    return tuple(out + [(a, b * Ri % Q) for a, b in out])


# ---------------------------------------------------------------- coverage (reference only)
@functools.lru_cache(None)
def gl_coverage():
    """{operation: Counter of branch classes} over the DIRECTED inputs of the Goldilocks cases"""
    a, b = gl_pairs()
    cov = {"add": collections.Counter(add_class(x, y) for x, y in zip(a, b)),
           "add_exact": collections.Counter("s=p" if x + y == P else "s=2^64" for x, y in zip(a, b) if x + y in (P, 1 << 64)),
           "sub": collections.Counter(sub_class(x, y) for x, y in zip(a, b)),
           "mul": collections.Counter(reduce_class(*words(x * y)) for x, y in zip(a, b)),
           "reduce128_raw": collections.Counter(reduce_class(x, y) for x, y in zip(*reduce_inputs())),
           "fold_small": collections.Counter(fold_small_class(x, y) for x, y in zip(a, b)),
           "mul_x32": collections.Counter(mul_x32_class(z) for z in single_operands()),
           "mul_x64": collections.Counter(mul_x64_class(z) for z in single_operands())}
    return cov


@functools.lru_cache(None)
def single_operands():
    """the edge set, extended for mul_x32 (an operation of ONE operand: 338 inputs).  z0 2^32 + z1 EPS = (z0 + z1) 2^32 - z1 lies in [p, 2^64) exactly when
    z0 + z1 = 2^32 (then it is 2^64 - z1), which five of the edge values satisfy: 32 more do here, and their neighbours z0 + z1 = 2^32 +- 1 on either side"""
    z1s = [1, 2, 3, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFD, 0xFFFFFFFE] + [1 << k for k in range(2, 31)]
    extra = [(z1 << 32 | ((1 << 32) - z1 + d)) % P for z1 in dict.fromkeys(z1s) for d in (0, -1, 1) if (1 << 32) - z1 + d < 1 << 32]
    return tuple(dict.fromkeys(gl_edge() + tuple(extra)))


@functools.lru_cache(None)
def gl_pairs():
    """all pairs of the edge set, and the pairs that hit the exact boundaries of add and sub whatever the set holds: a + b = 2^64, 2^64 - 1, p, p - 1, p + 1"""
    a, b = all_pairs(gl_edge())
    for x in dict.fromkeys(gl_edge()):
        for s in (1 << 64, (1 << 64) - 1, P, P - 1, P + 1):
            if 0 <= s - x < P:
                a.append(x); b.append(s - x)
    return tuple(a), tuple(b)


@functools.lru_cache(None)
def reduce_inputs():
    """raw (lo, hi) of operation 12: all pairs of the edge set as they are, and the words of the full products of all pairs"""
    a, b = gl_pairs()
    pw = [words(x * y) for x, y in zip(a, b)]
    return a + tuple(w[0] for w in pw), b + tuple(w[1] for w in pw)


@functools.lru_cache(None)
def bb_coverage():
    e = bb_edge()
    a, b = all_pairs(e)
    a, b = a + [x for x, _ in bb_montgomery_pairs()], b + [y for _, y in bb_montgomery_pairs()]
    t1 = [bb_t(x * y) for x, y in zip(a, b)]
    ttw = [bb_t(x * ((y << 32) % Q)) for x, y in zip(a, b)]
    cov = {"mul_t": collections.Counter(), "mul_tw_t": collections.Counter()}
    for name, ts in (("mul_t", t1), ("mul_tw_t", ttw)):
        for t in ts:
            cov[name]["t>=p" if t >= Q else "t<p"] += 1
            if t in (0, Q - 1, Q, Q + 1, 2 * Q - 1):
                cov[name]["t=" + {0: "0", Q - 1: "p-1", Q: "p", Q + 1: "p+1", 2 * Q - 1: "2p-1"}[t]] += 1
    cov["add"] = collections.Counter("ge_p" if x + y >= Q else "neither" for x, y in zip(a, b))
    cov["sub"] = collections.Counter(sub_class(x, y) for x, y in zip(a, b))
    return cov


def case_coverage():
    """Every reachable branch class of every operation occurs often enough among the directed inputs: 256 times for add and the products, 16 for the operations of
    one operand (and for a = b of sub, which the set's diagonal gives 338 times).  Measured (printed below; run with -s):
      Goldilocks  add            carry 59585, s >= p without carry 8975, neither 47157; s = p 624, s = 2^64 296   (the 338^2 pairs alone: 59329 / 8079 / 46836)
                  sub            a < b 57460, a = b 379, a > b 57878
                  mul, mul_tw    000 62596, 001 6959, 010 40495, 101 585, 110 5082      (borrow, carry, r >= p; the 338^2 pairs alone: at least 569)
                  reduce128 raw  000 114671, 001 10975, 010 84349, 101 4120, 110 17319;  011, 100 and 111 unreachable (reduce_class) and absent
                  fold_small     wrapped 37924, >= p 4059, neither 73734
                  mul_x32        wrapped 158, >= p 37, neither 230          mul_x64  borrow 65, none 360
      BabyBear    add            s >= p 14716, neither 11841                sub  a < b 13449, a = b 160, a > b 12948
                  mul (first reduction)  t < p 23368, t >= p 3189, t = 0 321, t = p - 1 258, t = p + 1 191
                  mul_tw                 t < p 20479, t >= p 6078, t = 0 321, t = p - 1 204, t = p + 1 165;  t = p and t = 2 p - 1 unreachable (bb_montgomery_pairs)"""
    assert len(gl_edge()) == 338
    a, b = all_pairs(gl_edge())      # the set itself, pinned by its counts: 338^2 pairs before gl_pairs() adds the exact boundaries
    plain = collections.Counter(add_class(x, y) for x, y in zip(a, b))
    assert (plain["ge_p"], plain["carry"], plain["neither"]) == (8079, 59329, 46836)
    assert min(collections.Counter(reduce_class(*words(x * y)) for x, y in zip(a, b)).values()) == 569
    cov = gl_coverage()
    for name, c in sorted(cov.items()):
        print("goldilocks", name, dict(sorted(c.items())))
    assert set(cov["add"]) == {"carry", "ge_p", "neither"} and min(cov["add"].values()) >= 256
    assert cov["add_exact"]["s=p"] >= 16 and cov["add_exact"]["s=2^64"] >= 16
    assert set(cov["sub"]) == {"lt", "eq", "gt"} and min(cov["sub"].values()) >= 256
    for name in ("mul", "reduce128_raw"):
        assert set(cov[name]) == set(REDUCE_CLASSES), (name, cov[name])     # the three unreachable ones (reduce_class) do not occur
        assert min(cov[name].values()) >= 256, (name, cov[name])
    assert min(cov["mul"].values()) >= 569
    assert set(cov["fold_small"]) == {"wrap", "ge_p", "neither"} and min(cov["fold_small"].values()) >= 256
    assert set(cov["mul_x32"]) == {"wrap", "ge_p", "neither"} and min(cov["mul_x32"].values()) >= 16, cov["mul_x32"]
    assert set(cov["mul_x64"]) == {"borrow", "none"} and min(cov["mul_x64"].values()) >= 16, cov["mul_x64"]
    bb = bb_coverage()
    for name, c in sorted(bb.items()):
        print("babybear", name, dict(sorted(c.items())))
    for name in ("mul_t", "mul_tw_t"):
        c = bb[name]
        assert c["t=0"] >= 16 and c["t<p"] >= 256 and c["t>=p"] >= 256, (name, c)
        assert c["t=p"] == 0 and c["t=2p-1"] == 0          # unreachable: bb_montgomery_pairs
    for name in ("mul_t", "mul_tw_t"):
        assert bb[name]["t=p-1"] >= 16 and bb[name]["t=p+1"] >= 16, bb[name]
    assert ((Q - 1)**2 + M32 * Q) >> 32 < 2 * Q - 1
    assert min(bb["add"].values()) >= 256 and min(bb["sub"]["lt"], bb["sub"]["gt"]) >= 256 and bb["sub"]["eq"] >= 16
    return cov, bb


# ---------------------------------------------------------------- references (computed once, shared by the classes)
GL_REF = {0: lambda x, y: (x + y) % P, 1: lambda x, y: (x - y) % P, 2: lambda x, y: x * y % P, 3: lambda x, y: x * y % P,
          4: lambda x, y: (x << 32) % P, 5: lambda x, y: (x << 64) % P, 6: lambda x, y: (x << (y % 96)) % P, 7: lambda x, y: (x + ((y & 0x7FFFFFFF) << 64)) % P,
          12: lambda x, y: (x + (y << 64)) % P, 13: lambda x, y: (x << (y % 96)) % P, 14: lambda x, y: pow(x, P - 2, P)}
BB_REF = {0: lambda x, y: (x + y) % Q, 1: lambda x, y: (x - y) % Q, 2: lambda x, y: x * y % Q, 3: lambda x, y: x * y % Q,
          14: lambda x, y: pow(x, Q - 2, Q), 15: lambda x, y: x * y % Q | x << 32}


@functools.lru_cache(None)
def gl_case(op, nrand):
    """(a, b, expected) of one Goldilocks operation: the directed inputs, then nrand random ones"""
    e = gl_edge()
    if op in (0, 1, 2, 3, 7):
        a, b = (list(v) for v in gl_pairs())
    elif op in (4, 5, 14):
        a = list(single_operands()); b = [0] * len(a)
    elif op in (6, 13):
        a = [x for x in e for _ in range(96)]; b = [s for _ in e for s in range(96)]
    elif op == 12:
        a, b = (list(v) for v in reduce_inputs())
    if op == 12:      # raw words: any 64-bit pattern, canonical or not
        a, b = a + list(rand_words(nrand, 100 + op)), b + list(rand_words(nrand, 200 + op))
    else:
        a, b = a + rand_field(P, nrand, 100 + op), b + (rand_field(P, nrand, 200 + op) if op < 6 else list(rand_words(nrand, 200 + op)))
    if op == 14:
        a = a[:len(single_operands()) + min(nrand, 1 << 12)]; b = b[:len(a)]       # (a big-integer pow per element)
    f = GL_REF[op]
    return u64(a), u64(b), u64([f(x, y) for x, y in zip(a, b)])


@functools.lru_cache(None)
def bb_case(op, nrand):
    e = bb_edge()
    a, b = all_pairs(e)
    a, b = a + [x for x, _ in bb_montgomery_pairs()], b + [y for _, y in bb_montgomery_pairs()]
    a, b = a + rand_field(Q, nrand, 300 + op), b + rand_field(Q, nrand, 400 + op)
    f = BB_REF[op]
    return u64(a), u64(b), u64([f(x, y) for x, y in zip(a, b)])


def run_case(ctx, what, op, cls, case):
    a, b, want = case
    got = ctx.arith_selftest(op, a, b, cls=cls)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"{what} op {op} class {cls}: {len(bad)} of {len(a)} mismatches, first at {bad[0]}: a={int(a[bad[0]]):#x} b={int(b[bad[0]]):#x} "
                           f"got {int(got[bad[0]]):#x} want {int(want[bad[0]]):#x}")


def case_gl_pairs(mk, cls, op, nrand):
    """operations 0-3 of one Goldilocks class on all pairs of the edge set and on random pairs"""
    run_case(mk(0), "goldilocks " + GL_CLASSES[cls], op, cls, gl_case(op, nrand))


def case_gl_single(mk, cls, nrand):
    """mul_x32, mul_x64 and fold_small of the sign-bit / exec-masked classes, and the class's shift by every exponent 0..95 (GLT / GLM: the chains of the butterflies;
    GL: GL::mul_pow2, the FRI fold's form)"""
    for op in ((6,) if cls == 1 else (4, 5, 6, 7)):
        run_case(mk(0), "goldilocks " + GL_CLASSES[cls], op, cls, gl_case(op, nrand))


def case_gl_reduce128(mk, cls, nrand):
    run_case(mk(0), "goldilocks " + GL_CLASSES[cls], 12, cls, gl_case(12, nrand))


def case_gl_own(mk, nrand):
    """the round-1 shift form by every exponent and the inversion chain (0 -> 0), as class 0 and as class 1: the same code either way"""
    for cls in (0, 1):
        for op in (13, 14):
            run_case(mk(0), "goldilocks GL's own", op, cls, gl_case(op, nrand))


def case_class0_is_glm(mk, nrand):
    """class 0 keeps its meaning: operations 0-7 give what class 3 gives (and what the integers give)"""
    for op in range(8):
        run_case(mk(0), "goldilocks class 0", op, 0, gl_case(op, nrand))


def case_bb(mk, nrand):
    for op in (0, 1, 2, 3, 14, 15):
        c = bb_case(op, nrand if op != 14 else min(nrand, 1 << 12))
        run_case(mk(1), "babybear", op, 0, c)


# ---------------------------------------------------------------- extension towers
def ext_core(field):
    p = MODULUS[field]
    s = 32 if field == 0 else 16
    return [0, 1, 2, 2**s - 1, 2**s, p - 2**s, p - 2, p - 1, (p - 1) // 2]


@functools.lru_cache(None)
def ext_elements(field):
    """Fp2: all 81 elements over the 9-value core; Fp4: the elements with one non-zero limb, the all-(p-1) element and a seeded sample of the rest, 256 in all"""
    core = ext_core(field)
    if field == 0:
        return tuple(itertools.product(core, repeat=2))
    p = MODULUS[field]
    fixed = [tuple(v if k == j else 0 for k in range(4)) for j in range(4) for v in core[1:]] + [(p - 1,) * 4, (0,) * 4]
    rest = [t for t in itertools.product(core, repeat=4) if t not in set(fixed)]
    rng = np.random.RandomState(4)
    pick = rng.choice(len(rest), size=256 - len(fixed), replace=False)
    return tuple(fixed + [rest[i] for i in sorted(pick)])


@functools.lru_cache(None)
def ext_case(field, op, nrand):
    p, e = MODULUS[field], pyref.FIELDS[field]["ext"]
    T = pyref.Tower(field, e)
    els = ext_elements(field)
    a, b = all_pairs(els)
    ra, rb = rand_field(p, nrand * e, 500 + op), rand_field(p, nrand * e, 600 + op)
    a += [tuple(ra[i * e:(i + 1) * e]) for i in range(nrand)]
    b += [tuple(rb[i * e:(i + 1) * e]) for i in range(nrand)]
    T2 = pyref.Tower(field, 2)
    halves = lambda x: (x[:2], x[2:])
    f = {32: T.mul, 33: T.mul, 34: T.add, 35: T.sub, 36: lambda x, y: tuple(v * y[0] % p for v in x),
         37: lambda x, y: sum((T2.mul(h, g) for h, g in zip(halves(x), halves(y))), ()),
         38: lambda x, y: sum((T2.mul(T.nr4, h) for h in halves(x)), ())}[op]
    want = [f(x, y) for x, y in zip(a, b)]
    flat = lambda v: u64([limb for el in v for limb in el])
    return flat(a), flat(b), flat(want)


def ext_ops(field):
    return (32, 33, 34, 35, 36) + ((37, 38) if field == 1 else ())


def case_ext(mk, field, op, nrand=1 << 12):
    classes = (0, 1) if field == 0 else (0,)
    for cls in classes:
        run_case(mk(field), f"field {field} extension", op, cls, ext_case(field, op, nrand))


# ---------------------------------------------------------------- refusals
def case_refusals(mk, field):
    """what ms_arith_selftest refuses with MS_ERR_ARG before anything is launched, and that the context computes after each refusal"""
    ctx = mk(field)
    e = ctx.e
    buf = np.ones(4 * e, dtype=np.uint64)
    out = np.zeros(4 * e, dtype=np.uint64)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_uint64))
    w = lambda op, cls=0: op | cls << 8
    if field == 0:
        bad = [(w(0, 4), 4), (w(2, 255), 4), (w(0, 1 << 20), 4), (w(12, 0), 4), (w(12, 3), 4), (w(4, 1), 4), (w(5, 1), 4), (w(7, 1), 4), (w(13, 2), 4), (w(14, 3), 4),
               (w(8, 2), 4), (w(32, 2), 4), (w(36, 3), 4), (w(15), 4), (w(16), 4), (w(31), 4), (w(37), 4), (w(38), 4), (w(39), 4), (w(255), 4), (-1, 4),
               (w(32), 3), (w(34, 1), 1), (w(36), 2 * e + 1)]
    else:
        bad = [(w(0, 1), 4), (w(2, 3), 4), (w(32, 1), 4), (w(14, 2), 4)] + [(w(op), 4) for op in list(range(4, 14)) + [16, 31, 39, 255]] + [(-1, 4),
               (w(32), 6), (w(37), 2), (w(38), 4 * e - 1)]
    for word, n in bad:
        assert ctx.L.ms_arith_selftest(ctx.h, C.c_int(word), ptr(buf), ptr(buf), ptr(out), C.c_size_t(n)) == ERR_ARG, (word & 0xFF, word >> 8, n)
        assert ctx.last_error()
        assert int(ctx.arith_selftest(0, [1], [2])[0]) == 3
    p = MODULUS[field]
    assert ctx.L.ms_arith_selftest(ctx.h, C.c_int(0), ptr(u64([p])), ptr(buf), ptr(out), C.c_size_t(1)) == ERR_ARG      # operands stay canonical ...
    assert ctx.L.ms_arith_selftest(ctx.h, C.c_int(32), ptr(buf), ptr(u64([1] * (e - 1) + [p])), ptr(out), C.c_size_t(e)) == ERR_ARG
    if field == 0:                                                                                                        # ... except the raw words of operation 12
        assert int(ctx.arith_selftest(12, [M64], [M64], cls=1)[0]) == (M64 + (M64 << 64)) % P
