"""The throughput form of the FRI evaluation-domain fold (csrc/poly.hpp FriFoldWgKernel: one inversion per workgroup, octet layout on Goldilocks' roots of unity,
base-field source in the first fold), shared by the emulation suite (test_fold_eval_emu.py) and the GPU suite (test_fold_eval_gpu.py).

Anchor: the library's own transform path.  A context created with MS_FRI_POINTWISE=0 computes the codeword of every round >= 1 by NTT of the round polynomial
(which the full-proof tests pin to the oracle); the context under test folds pointwise, with MS_FOLD_SMALL_MAX=0 (the throughput kernel at every size) and
MS_FRI_TAIL_MAX=0 (no fused rounds).  Field arithmetic is exact: every codeword and every root must be EQUAL.

`make(field, env)` returns a fresh mini_stark_amd.Context created while the variables of `env` are set."""
import numpy as np

from common import MODULUS, EXT, SplitMix64, fibonacci_trace_fast, fibonacci_closures
from oracle import oracle as orc

UNDER_TEST = {"MS_FOLD_SMALL_MAX": "0", "MS_FRI_TAIL_MAX": "0"}
TRANSFORM = {"MS_FOLD_SMALL_MAX": "0", "MS_FRI_TAIL_MAX": "0", "MS_FRI_POINTWISE": "0"}
# (log2 rows, blowup, round-0 domain).  Every proof folds D0 -> D0/2 -> ... -> 2, so the largest one alone passes through every smaller previous-domain size with an
# extension-field source; the small ones put the FIRST fold (base-field source) at each size where the kernel changes its path:
# 2^4: m_out = 8, exactly one octet per position; 2^5, 2^6: a few lanes of one wave; 2^9: one workgroup, partly filled (32 of 256 threads); 2^13: 512 positions = two
# workgroups (the largest also on the item layout's multi-workgroup grid for BabyBear: 4096 outputs = two workgroups of 2048).
SIZES = [(1, 8, 16), (2, 8, 32), (3, 8, 64), (6, 8, 512), (10, 8, 8192), (3, 2, 16)]


def env_ctx(make_plain):
    """make(field, env) from make_plain(field): the knobs are read at ms_create, so they are set around the creation only."""
    import os

    def make(field, env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return make_plain(field)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    return make


class PinnedShard:
    """A one-rank world (MS_SHARD_WORLD1=1 at ms_create) whose exchange buffers are page-locked host memory of the library (ms_pinned_alloc: mapped into the device's
    address space) and whose collectives are memmove's between them - the library synchronises its stream before it calls back.  No torch, no second process."""

    def __init__(self, ctx, cap):
        import ctypes as C
        self.C, self.ctx, self.cap = C, ctx, cap
        self.send, self.recv = ctx.pinned_alloc(cap), ctx.pinned_alloc(cap)
        assert self.send and self.recv
        ctx.set_shard(0, 1, self.send, self.recv, cap, self._exchange)

    def _exchange(self, op, nbytes):
        C = self.C
        if op in (0, 1, 5):          # all-to-all / all-gather / gather of one rank: its own payload comes back
            C.memmove(self.recv, self.send, nbytes)
        elif op == 4:                # one slice of the sliced all-to-all
            off, stride = C.c_size_t(0), C.c_size_t(0)
            self.ctx.check(self.ctx.L.ms_shard_slice_layout(self.ctx.h, C.byref(off), C.byref(stride)))
            C.memmove(self.recv + off.value, self.send + off.value, nbytes)
        return 0                     # (2, 3: all-reduces over one rank leave the buffer as it is)

    def close(self):
        self.ctx.set_shard(0, 1, 0, 0, 0, None)
        self.ctx.pinned_free(self.send)
        self.ctx.pinned_free(self.recv)


def setup_fibonacci(field, log_n, blowup):
    N = 1 << log_n
    trace = fibonacci_trace_fast(field, N)

    def run(ctx, rng):
        p = MODULUS[field]
        assert ctx.trace_commit(trace, 3)[0] == 0 and ctx.interpolate() == 0      # (one row per leaf group: N = 2 still has two)
        for sc, idx in fibonacci_closures(field, N, orc.root_of_unity(field, N)):
            assert ctx.polys_lincomb(sc, idx) == 0
        assert ctx.lde_commit(blowup, rng.nonzero(p), 3)[0] == 0
        assert ctx.mix(rng.field(p)) == 0
    return run


def setup_cubic(field, log_n, w, blowup):
    """ms_mix_cubic: a 2N-coefficient base-field validity polynomial"""
    import parity_cases as pc
    trace, spec, sc = pc.cubic_trace(field, 1 << log_n, w, 9)

    def run(ctx, rng):
        p = MODULUS[field]
        assert ctx.trace_commit(trace, w)[0] == 0 and ctx.interpolate() == 0
        assert ctx.lde_commit(blowup, rng.nonzero(p), w)[0] == 0
        assert ctx.mix_cubic(rng.field(p), spec, sc) == 0, ctx.last_error()
    return run


def commit_phase(ctx, field, setup, blowup, seed, base_z=(), sharded=False):
    """Every foldable round of the FRI commit phase with challenges from SplitMix64(seed).  Returns [(round, ncoef, D, B, root, codeword or None)].  A codeword is None
    only in a sharded proof, for a round whose codeword the library reports as distributed over the ranks (its root stands for it); every other read must succeed."""
    import mini_stark_amd as ms
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(seed)
    setup(ctx, rng)
    rc, root = ctx.fri_begin(blowup, 64)
    assert rc == 0, ctx.last_error()

    def cw(i):
        if sharded:
            import ctypes as C
            _, D = ctx.fri_round_info(i)
            out = np.zeros((D, e), dtype=np.uint64)
            rc = ctx.L.ms_fri_round_codeword_read(ctx.h, C.c_int(i), out.ctypes.data_as(C.POINTER(C.c_uint64)))
            if rc == ms.ERR_STATE:
                return None
            assert rc == 0, ctx.last_error()
            return out.tolist()
        return ctx.fri_round_codeword(i).tolist()
    nc, D = ctx.fri_round_info(0)
    out = [(0, nc, D, None, root, cw(0))]
    i = 1
    while D >= 4:
        z = [rng.field(p) for _ in range(e)]
        if i in base_z:          # a DEEP point in the base field: y - z has zeros on the domain, the library must take the transform
            z = [z[0]] + [0] * (e - 1)
        rc, B = ctx.fri_deep(z)
        assert rc == 0, ctx.last_error()
        rc, root = ctx.fri_fold_commit([rng.field(p) for _ in range(e)])
        assert rc == 0, ctx.last_error()
        nc, D = ctx.fri_round_info(i)
        out.append((i, nc, D, B.tolist(), root, cw(i)))
        i += 1
    return out


def case_matches_transform(make, field, setup, blowup, seed=5, base_z=(), expect_D0=None, expect_odd_len=False, shard=None):
    """Pointwise rounds == transformed rounds: lengths, B values, roots and codewords of every round.  `shard(ctx)` (optional) puts a context into a one-rank world
    and returns an object with close()."""
    res = []
    for env in (UNDER_TEST, TRANSFORM):
        ctx = make(field, env)
        sh = shard(ctx) if shard else None
        try:
            res.append(commit_phase(ctx, field, setup, blowup, seed, base_z, sharded=shard is not None))
        finally:
            if sh:
                sh.close()
            ctx.close()
    got, want = res
    if expect_D0 is not None:
        assert got[0][2] == expect_D0, (got[0][2], expect_D0)
    if expect_odd_len:
        assert got[0][1] & (got[0][1] - 1), f"the case wants a trimmed length that is no power of two, got {got[0][1]}"
    assert len(got) == len(want) and len(got) == got[0][2].bit_length() - 1      # D0, D0/2, ..., 2
    for a, b in zip(got, want):
        assert a[:5] == b[:5], f"round {a[0]}: length / domain / B / root differ: {a[:5]} vs {b[:5]}"
        assert (a[5] is None) == (b[5] is None) and (shard is not None or a[5] is not None)
        if a[5] is not None and a[5] != b[5]:
            bad = [j for j, (x, y) in enumerate(zip(a[5], b[5])) if x != y]
            raise AssertionError(f"round {a[0]} (D = {a[2]}): {len(bad)} codeword elements differ, first at {bad[0]}: {a[5][bad[0]]} vs {b[5][bad[0]]}")
    return got


def case_one_round_vs_pyref(make, field=0, log_n=3, blowup=8):
    """Second anchor: tests/pyref.py's naive fold (big integers, polynomial division, evaluation point by point) - the first fold of a 2^6-point domain,
    element by element."""
    from pyref import PyProver
    p, e = MODULUS[field], EXT[field]
    N = 1 << log_n
    trace = fibonacci_trace_fast(field, N)
    rng = SplitMix64(11)
    shift, r = rng.nonzero(p), rng.field(p)
    z, alpha = [rng.field(p) for _ in range(e)], [rng.field(p) for _ in range(e)]
    ctx = make(field, UNDER_TEST)
    py = PyProver(field)
    try:
        assert ctx.trace_commit(trace, 6)[0] == 0 and ctx.interpolate() == 0
        py.trace_commit(trace, 6)
        py.interpolate()
        for sc, idx in fibonacci_closures(field, N, orc.root_of_unity(field, N)):
            assert ctx.polys_lincomb(sc, idx) == 0
            py.lincomb(sc, idx)
        assert ctx.lde_commit(blowup, shift, 6)[0] == 0 and ctx.mix(r) == 0
        py.mix(r)
        rc, root0 = ctx.fri_begin(blowup, 3)
        assert rc == 0 and root0 == py.fri_begin(blowup, 3)
        assert ctx.fri_round_info(0)[1] == 64
        rc, B = ctx.fri_deep(z)
        assert rc == 0 and [tuple(B[:e].tolist()), tuple(B[e:].tolist())] == [tuple(v) for v in py.fri_deep(z)]
        rc, root1 = ctx.fri_fold_commit(alpha)
        assert rc == 0
        want_root = py.fri_fold_commit(alpha)
        got = [tuple(v) for v in ctx.fri_round_codeword(1).tolist()]
        want = [tuple(int(x) for x in v) for v in py.rounds[1]["ev"]]
        assert len(got) == 32 and got == want
        assert root1 == want_root
    finally:
        ctx.close()


def case_shift_multiplications(make_plain):
    """ms_arith_selftest ops 8 / 9 / 10 (GL::mul_2p24 / mul_2p48 / mul_2p72) and 11 (every shift the octets use, 2^(12 k)): against Python integers AND against the
    library's general product (op 2) by the same power of two, on edge values (around p, 2^32, 2^63: every carry / borrow of the reductions) and random ones."""
    p = MODULUS[0]
    edge = [0, 1, 2, p - 1, p - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFEFFFFFFFF, 1 << 63, (1 << 63) - 1, 0xFFFFFFFE, 0x1FFFFFFFF,
            0xFFFFFFFE00000001, 0xFFFFFFFE00000002, 0x7FFFFFFF80000001, 0x80000000FFFFFFFF, 0xFFFFFFFF00000000 - 1, (1 << 40) - 1, (1 << 52), (1 << 20) + 1]
    edge += [(1 << k) % p for k in range(64)] + [(p - (1 << k)) % p for k in range(64)] + [((1 << k) - 1) % p for k in range(1, 64)]
    rng = SplitMix64(4242)
    vals = [v % p for v in edge] + [rng.field(p) for _ in range(4096)]
    ctx = make_plain(0)
    try:
        for op, s in ((8, 24), (9, 48), (10, 72)):
            got = ctx.arith_selftest(op, vals, [0] * len(vals))
            want = np.array([(x << s) % p for x in vals], dtype=np.uint64)
            assert (got == want).all(), (op, [hex(vals[i]) for i in np.nonzero(got != want)[0][:4]])
            assert (got == ctx.arith_selftest(2, vals, [(1 << s) % p] * len(vals))).all()
        for k in range(8):
            got = ctx.arith_selftest(11, vals, [k + 8 * (k & 1)] * len(vals))     # (b mod 8 selects the shift)
            want = np.array([(x << (12 * k)) % p for x in vals], dtype=np.uint64)
            assert (got == want).all(), (k, [hex(vals[i]) for i in np.nonzero(got != want)[0][:4]])
            assert (got == ctx.arith_selftest(2, vals, [(1 << (12 * k)) % p] * len(vals))).all()
    finally:
        ctx.close()
