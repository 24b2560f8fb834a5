"""ONE context through different flows and sizes: the cases of the build-defined stages' suites (linked, staged, air, air_ext, terms, parity, deep, aux, open, air_check,
grind; on the GPU also scale), called UNCHANGED as steps on a context that is never destroyed between them, shared by the emulation suite (tests/test_lifecycle_emu.py)
and the GPU suite (tests/test_lifecycle_gpu.py).  Their own suites give every case a fresh context; callers keep one for the life of the process (the bench lanes,
HostStark, examples/rust_shim), so what must survive or be dropped between proofs - have_*, the virtual LDE columns, the inverse table of ms_mix_air and its key, the
staged columns, where the validity length lives, the rounds' capacities, the plan map, buffers that only grow - is exercised here, in three orders and behind refusals.
The references are the ones the steps already answer to (the C++ oracle, tests/pyref*.py, hashlib trees); every comparison is exact, and nothing is compared with
another run of the library alone.

`Shared(new)` is the factory: one context per (field, flags, env) for the lifetime of a test, handed out under the three factory conventions of tests/ -
`make(field, flags, env=None)`, `mk(field, fresh=False)` and `make_ctx(field)`.  The contexts are SharedContext objects, whose close() does nothing until
Shared.release() at the end of the test (scale_cases.case_stage_ledger and parity_cases close what they were given).

Left out, and why:
  staged_cases.case_columns                  compares two INDEPENDENT contexts built side by side (the staged flow and the one-tree flow of the same columns)
  the *_refusals_arg_state cases, case_errors  assert the state of a context on which nothing has run (ms_interpolate == MS_ERR_STATE first of all)
  the *_alloc_failures cases                 arm the emulation build's allocation hook, whose count is the fresh context's
  the *_sharded* cases                       turn sharding on, which a context does not leave again
Steps that take a second context by the same key (linked_cases.case_definition's `other`, staged_cases.case_openings' `plain` and `B`, case_mix_cubic's ctx2 / ctx3,
the lc.prove inside staged_cases.case_end_to_end) get the SAME context again: each has finished with the first one by then."""
import numpy as np

import mini_stark_amd as ms
import air_cases as ac
import air_check_cases as cc
import air_ext_cases as xc
import aux_cases as auxc
import deep_cases as dc
import grind_cases as gc
import linked_cases as lc
import open_cases as oc
import parity_cases as pc
import staged_cases as sc
import terms_cases as tc
from common import MODULUS, EXT, SplitMix64, fibonacci_trace

SHA = lc.SHA
ZAE = oc.ZAE


class SharedContext(ms.Context):
    """a context whose close() does nothing: the steps' own close() calls must not end it.  release() destroys it."""

    def close(self):
        pass

    def release(self):
        ms.Context.close(self)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Shared:
    """`new(field, flags, env)` creates a SharedContext; one is kept per (field, flags, env).  `count` is the number created."""

    def __init__(self, new):
        self.new, self.live = new, {}

        def make(field, flags, env=None):
            key = (field, flags, tuple(sorted((env or {}).items())))
            if key not in self.live:
                ctx = new(field, flags, env)
                assert isinstance(ctx, SharedContext)
                self.live[key] = ctx
            return self.live[key]

        def mk(field, fresh=False):
            return make(field, ZAE)

        def make_ctx(field):
            return make(field, ZAE)
        self.make, self.mk, self.make_ctx = make, mk, make_ctx

    @property
    def count(self):
        return len(self.live)

    def release(self):
        for ctx in self.live.values():
            ctx.release()
        self.live = {}


# ---------------------------------------------------------------- the steps: existing cases, with the arguments their own suites give them
def steps(field, ledger=None):
    """[(name, step(S))] for one field.  `ledger` (GPU): scale_cases.case_stage_ledger at shape A, put between two small steps - buffers and plans grow and shrink"""
    e = EXT[field]
    out = [("linked.definition[cubic-64]", lambda S: lc.case_definition(S.make, SHA, field, "cubic", N=64)),
           ("linked.end_to_end", lambda S: lc.case_end_to_end(S.make, SHA, field, "cubic", N=8, R=3, gb=0))]
    out += [("staged.end_to_end[%s]" % which, lambda S, which=which: sc.case_end_to_end(S.make, SHA, field, which, N=8, R=3, gb=0)) for which in ("permutation", "logup")]
    out += [("staged.openings", lambda S: sc.case_openings(S.make, SHA, field, "logup", 3))]
    out += [("air.definition[%s-%d]" % row, lambda S, row=row: ac.case_definition(S.mk, field, *row)) for row in ac.DEFINITION_ROWS]
    if ledger is not None:
        out += [("scale.stage_ledger[A]", ledger)]
    out += [("air_ext.definition[%s-%d]" % row, lambda S, row=row: xc.case_definition(S.mk, field, *row)) for row in ac.DEFINITION_ROWS]
    out += [("terms.definition[%s-%d-%d]" % row, lambda S, row=row: tc.case_definition(S.mk, field, *row)) for row in tc.DEFINITION_ROWS]
    out += [("parity.prove[6-4]", lambda S: pc.case_prove(S.mk, field, 6, 4)),
            ("parity.prove[4-8]", lambda S: pc.case_prove(S.mk, field, 4, 8)),
            ("parity.mix_cubic", lambda S: pc.case_mix_cubic(S.mk, field)),
            ("deep.poly[8-3-2]", lambda S: dc.case_poly(S.make, field, 8, 3, 2)),
            ("deep.end_to_end", lambda S: dc.case_end_to_end(S.make, SHA, field, "fib")),
            ("aux.end_to_end[1]", lambda S: auxc.case_end_to_end(S.mk, field, 1, "permutation")),
            ("aux.end_to_end[E]", lambda S: auxc.case_end_to_end(S.mk, field, e, "logup")),
            ("open.lde_rows[65]", lambda S: oc.case_lde_rows(S.make, SHA, field, 65)),
            ("open.query_index", lambda S: oc.case_query_index(S.make, SHA, field, 8, 8, True)),
            ("air_check.clean", lambda S: cc.case_clean(S.mk, field, "mimc", 4)),
            ("grind.smallest", lambda S: gc.case_smallest(gc.ctx_of(S.make, SHA, field), SHA, bits_list=[0, 8, 9], seeds=gc.SEEDS[:1], starts=[0, 2**32 - 3])),
            ("vtree.dies_with_the_lde", lambda S: step_validity_tree_dies(S, field))]
    return out


def step_validity_tree_dies(S, field, N=16, blowup=4):
    """The one step that is not an existing case.  include/ministark.h: the validity tree (and the DEEP polynomial with it) lives until the next mix stage,
    ms_polys_*, ms_lde_commit or ms_trace_commit.  A second ms_lde_commit over the SAME polynomials on another coset leaves everything else of the linked state in
    place - the validity polynomial too - so only the commitment itself can retire the tree: ms_tree_open(MS_TREE_VALIDITY), ms_deep_evals, ms_deep_compose and
    ms_query_linked must refuse, and a new ms_validity_commit must give the root of the chunk columns on the NEW coset (hashlib tree over the oracle's coset LDE)."""
    from oracle import oracle
    p = MODULUS[field]
    ctx = oc.ctx_of(S.make, SHA, field)
    P = lc.build_state(ctx, SHA, field, "fib", N=N, blowup=blowup, R=2, seed=3)
    assert ctx.deep_len() == N and len(ctx.tree_open(ms.TREE_VALIDITY, [0])) > 0
    shift2 = SplitMix64(9090).nonzero(p)
    assert shift2 != P["shift"]
    rc, _root = ctx.lde_commit(blowup, shift2, P["c"])
    assert rc == 0, ctx.last_error()
    assert ctx.deep_len() == 0
    assert oc.raw_open(ctx, ms.TREE_VALIDITY, 0, [0], 1, None, 0)[0] == ms.ERR_STATE
    assert ctx.deep_evals(P["zs"], P["lists"])[0] == ms.ERR_STATE
    assert ctx.deep_compose(P["zs"], P["lists"], P["gamma"]) == ms.ERR_STATE
    assert lc.raw_linked(ctx, [1], 1, None, 0)[0] == ms.ERR_STATE
    m = P["m"]
    rc, root = ctx.validity_commit(m)
    assert rc == 0, ctx.last_error()
    v = ctx.validity_read().reshape(-1, ctx.e)
    chunks = [np.ascontiguousarray(v[k * N:(k + 1) * N, l]) for k in range(v.shape[0] // N) for l in range(ctx.e)]
    vmat = np.ascontiguousarray(np.stack([oracle.coset_lde(field, col, shift2, N * blowup) for col in chunks], axis=1))
    assert bytes(dc.ro.tree_nodes(SHA, vmat.reshape(-1, 1), 1, m)[-1]) == root


# ---------------------------------------------------------------- refused stages, put in front of every flow
def refuse_shape(S, field, N=16):
    """air_cases.case_refusals_shape's first refusal: the MiMC program with one boundary value wrong - the compose launch runs, the division is not exact,
    ms_mix_air returns MS_ERR_SHAPE and the context is left behind a failed mix stage (inverse table built, buffers sized for 2N coefficients)"""
    p = MODULUS[field]
    rng = SplitMix64(67)
    shift, r = rng.nonzero(p), rng.field(p)
    sp = ac.spec_mimc(field, N)
    poly, row, value = sp["boundary"][1]
    ctx = S.mk(field, fresh=True)
    ac.commit(ctx, sp["trace"], 4, shift)
    assert ac.mix(ctx, r, sp, boundary=[sp["boundary"][0], (poly, row, (value + 1) % p), sp["boundary"][2]]) == ms.ERR_SHAPE


def refuse_arg(S, field):
    """a trace with one element >= p: ms_trace_commit returns MS_ERR_ARG from the device's range check, behind the tree build, and leaves no trace"""
    ctx = S.mk(field, fresh=True)
    bad = fibonacci_trace(field, 32)
    bad[17, 2] = MODULUS[field] + 1
    assert ctx.trace_commit(bad, 6)[0] == ms.ERR_ARG
    assert ctx.interpolate() == ms.ERR_STATE


ORDERS = ("forward_reverse_forward", "behind_refusals")


def create(field, flags, env=None, **kw):
    """a SharedContext created with `flags` while the variables of `env` are set (ms_create reads the MS_* variables); kw: lib_path"""
    import os
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return SharedContext(field, flags=flags, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def case_order(new, field, order, ledger=None):
    """one order of the whole list on the contexts of one Shared.  `forward_reverse_forward`: the list forward, reversed and forward again on the same contexts (the
    third pass meets every buffer at its largest and every cache as the other order left it); `behind_refusals`: a refused stage in front of every step, the two
    kinds in turn."""
    S = Shared(new)
    try:
        todo = steps(field, ledger)
        if order == "forward_reverse_forward":
            todo = todo + todo[::-1] + todo
        for i, (name, step) in enumerate(todo):
            try:
                if order == "behind_refusals":
                    (refuse_shape if i % 2 == 0 else refuse_arg)(S, field)
                step(S)
            except AssertionError as ex:
                raise AssertionError("step %d of order %r, %s, field %d, on a shared context: %s" % (i, order, name, field, ex)) from ex
        # the steps did share: one context for each set of flags / variables a step asked for, however often it asked
        assert 1 <= S.count <= 4, sorted(S.live)
        return S.count
    finally:
        S.release()
