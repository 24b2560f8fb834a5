"""CPU suite: the kernel code of mini-stark_amd/csrc compiled for host emulation
(tests/emu, -DMS_EMU: every kernel phase executed thread by thread) against the
oracle.  Checks kernel and host-orchestration logic in this GPU-less container;
the same cases run on the real HIP build in tests/test_gpu_parity.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import parity_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def mk():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    cache = {}

    def make(field, fresh=False):
        if fresh:
            return ms.Context(field, lib_path=EMU)
        if field not in cache:
            cache[field] = ms.Context(field, lib_path=EMU)
        return cache[field]
    return make


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18])
def test_ntt(mk, field, log_n):
    pc.case_ntt(mk, field, log_n)


def test_ntt_three_pass(mk):
    pc.case_ntt(mk, 0, 19, batch=1)
    pc.case_ntt(mk, 1, 19, batch=1)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup", [(3, 2), (4, 8), (9, 4), (12, 8), (14, 8), (15, 8), (16, 4)])
def test_coset_lde(mk, field, log_n, blowup):
    pc.case_coset_lde(mk, field, log_n, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("leaf_num,ext,lpn,ic", [(16, 1, 2, 2), (16, 1, 4, 2), (16, 1, 4, 4), (16, 1, 16, 16), (2, 1, 2, 2), (3, 1, 2, 2),
                                                 (4096, 1, 2, 2), (6144, 1, 6, 2), (24, 1, 6, 2), (1 << 13, 0, 2, 2), (64, 0, 2, 2)])
def test_merkle(mk, field, leaf_num, ext, lpn, ic):
    e = ext or pc.EXT[field]
    pc.case_merkle(mk, field, leaf_num, e, lpn, ic, special=True)


@pytest.mark.parametrize("field", [0, 1])
def test_merkle_binary_tree_every_height(mk, field):
    """r05: binary trees of 2 .. 2^16 leaf groups - every height the subtree kernel can be handed (one to nine levels per launch, one or two launches), hence every
    width of the levels hashed by PAIRS of lanes (merkle.hpp Sha256Pair: 128 .. 1 parents per workgroup, whole and partial groups of eight lanes, the root's
    two halves joined in one lane) next to the one-lane-per-node first level of a nine-level launch."""
    for k in range(2, 18):
        pc.case_merkle(mk, field, 1 << k, 1, 2, 2)


@pytest.mark.parametrize("field", [0, 1])
def test_prove_base_field_deep_points(mk, field):
    pc.case_prove_base_field_deep_points(mk, field)


@pytest.mark.parametrize("field,lpn,ext", [(0, 6, 1), (0, 3, 1), (0, 2, 2), (0, 16, 1), (1, 6, 1), (1, 12, 1), (1, 2, 4), (1, 4, 4)])
def test_merkle_message_length_sweep(mk, field, lpn, ext):
    pc.case_merkle_length_sweep(mk, field, lpn, ext)


@pytest.mark.parametrize("field,log_n,blowup", [(0, 4, 2), (0, 3, 8), (0, 6, 8), (1, 3, 2), (1, 5, 4), (0, 10, 8), (1, 10, 8)])
def test_prove(mk, field, log_n, blowup):
    pc.case_prove(mk, field, log_n, blowup)


def test_prove_multilevel_scan(mk):
    # N = 2^13: round 1 has 4096 folded coefficients -> two scan blocks (multi-level suffix Horner)
    pc.case_prove(mk, 0, 13, 2, read_big=False)


@pytest.mark.parametrize("field", [0, 1])
def test_error_codes(mk, field):
    pc.case_errors(mk, field)


@pytest.mark.parametrize("kmax,fast", [("5", "0"), ("6", "0"), ("7", "0"), ("6", "1"), ("7", "1"), ("8", "1")])
def test_ntt_virtual_pass_variants(kmax, fast, monkeypatch):
    """Small tiles force the multi-pass plans (virtual radix 8x{1,2,4} first pass, 2-4 real passes)
    that full-size transforms use on the GPU."""
    monkeypatch.setenv("MS_NTT_KMAX", kmax)
    monkeypatch.setenv("MS_NTT_FAST", fast)  # 0: generic kernel incl. multi-pass virtual plans; 1: compile-time specialised tiles
    ctxs = {}

    def mk2(field, fresh=False):
        if field not in ctxs:
            ctxs[field] = ms.Context(field, lib_path=EMU)
        return ctxs[field]
    for field in (0, 1):
        for log_n, blowup in [(9, 2), (9, 4), (10, 8), (12, 8), (13, 8), (11, 16)]:
            pc.case_coset_lde(mk2, field, log_n, blowup)
        pc.case_ntt(mk2, field, 13)
        pc.case_ntt(mk2, field, 16, batch=1)
    pc.case_prove(mk2, 0, 10, 8, read_big=False)
    pc.case_prove(mk2, 1, 9, 8, read_big=False)


@pytest.mark.parametrize("field", [0, 1])
def test_wide_air_shape(mk, field):
    pc.case_prove_wide(mk, field, log_n=6, w=64)


@pytest.mark.parametrize("field", [0, 1])
def test_general_closure_path(mk, field):
    pc.case_general_closure(mk, field)


def test_trace_commit_device_pointer(mk):
    """ms_trace_commit_device: same result as the host-pointer entry (in the emulation build a device pointer is a
    host pointer; on the GPU bench.py passes a torch tensor's data_ptr)."""
    import numpy as np
    from common import fibonacci_trace
    ctx = mk(0)
    t = np.ascontiguousarray(fibonacci_trace(0, 64))
    rc1, r1 = ctx.trace_commit(t, 6)
    rc2, r2 = ctx.trace_commit_device(t.ctypes.data, 64, 3, 6)
    assert rc1 == 0 and rc2 == 0 and r1 == r2
    assert ctx.interpolate() == 0


def test_prove_randomised_shapes(mk):
    """Differential fuzz: random step counts (several padding rows), blowups, query counts, seeds, both fields."""
    import random
    rnd = random.Random(20261003)
    for _ in range(12):
        field = rnd.randrange(2)
        log_n = rnd.randrange(2, 9)
        N = 1 << log_n
        steps = rnd.randrange(N // 2, N)          # Radix2EvaluationDomain::new(steps + 1) == N
        blowup = rnd.choice([2, 4, 8, 16])
        if log_n + blowup.bit_length() - 1 > 14:
            blowup = 2
        pc.case_prove(mk, field, log_n, blowup, nq_fri=rnd.randrange(0, 4), seed=rnd.randrange(1, 1 << 30), read_big=(log_n <= 6), steps=steps)


@pytest.mark.parametrize("field,ext,lpn,n", [(0, 1, 2, 64), (0, 1, 4, 64), (0, 2, 2, 32), (1, 4, 2, 16), (1, 1, 8, 4096)])
def test_merkle_prove_by_value(mk, field, ext, lpn, n):
    pc.case_merkle_prove(mk, field, n, ext, lpn)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [7, 8, 9, 15, 16])
@pytest.mark.parametrize("linear", [0, 1])
def test_lincomb_many_terms(mk, field, k, linear):
    pc.case_lincomb_many_terms(lambda f: mk(f, fresh=True), field, k, linear)


@pytest.mark.parametrize("field", [0, 1])
def test_device_trace_range_check(mk, field):
    pc.case_device_trace_range_check(mk, field, lambda a: (a.ctypes.data, a))   # emulation: "device" memory is host memory


@pytest.mark.parametrize("field", [0, 1])
def test_device_trace_range_check_across_pool_wraps(mk, field):
    pc.case_device_trace_range_check_across_pool_wraps(mk, field)


@pytest.mark.parametrize("v2", ["1", "0"])
def test_babybear_on_the_round2_tiles(mk, monkeypatch, v2):
    """BabyBear runs the cooperative round-2 tiles by default since r03; MS_NTT_V2=0 keeps the round-1 tiles, which stay in the
    library for single-pass sizes, other blowups and transforms beyond 2^25 non-zero points.  Both must be exact."""
    monkeypatch.setenv("MS_NTT_V2", v2)
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_ntt(fresh, 1, 16)
    pc.case_coset_lde(fresh, 1, 14, 8)


@pytest.mark.parametrize("v2", ["1", "2"])
def test_ntt_register_last_pass(mk, monkeypatch, v2):
    """Plans 2^K x 2^K x 2^j with the last 2^j points of every output done in registers (msntt::RegPassKernel): MS_NTT_V2_REGPASS=2 puts
    the plan on 2^7-row tiles, so that 2^15..2^19 points walk every register radix (j = 1..5), forward, inverse and behind the virtual
    zero-padding pass.  v2 = 2 runs BabyBear on the cooperative tiles too."""
    monkeypatch.setenv("MS_NTT_V2_REGPASS", "2")
    monkeypatch.setenv("MS_NTT_V2", v2)
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    fields = (0, 1) if v2 == "2" else (0,)
    for field in fields:
        for log_n in (15, 16, 17, 18, 19):
            pc.case_ntt(fresh, field, log_n, batch=1)
        for log_n, blowup in ((12, 8), (14, 8), (16, 8)):    # m = log_n: j = ... behind the virtual radix-8 pass (12: not this plan; 15, 17: j = 1, 3 via 2^15 / 2^17 below)
            pc.case_coset_lde(fresh, field, log_n, blowup)
        pc.case_coset_lde(fresh, field, 15, 8)
        pc.case_coset_lde(fresh, field, 17, 8)


def test_ntt_register_last_pass_full_tiles(mk):
    """The shipped shape: 2^10 x 2^10 x 2 on a 2^21-point transform (default knobs)."""
    pc.case_ntt(lambda f, fresh=False: mk(f, fresh=True), 0, 21, batch=1)


def test_ntt_fused_tail_full_tiles(mk):
    """The cooperative tiles whose last sub-round is fused with the store (and, in later passes, fed by LDS-DMA): 2^10 x 2^10 plain
    (last later pass, no row twiddles), 2^16 / 2^17 coefficients behind the virtual pass (2^8-row tiles in both modes, 2^9 x 2^8), and
    the benchmark's LDE shape 2^20 -> 2^23 (2^10-row tiles: merged twiddle tables in the first pass, DMA-fed last pass)."""
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_ntt(fresh, 0, 20, batch=1)
    pc.case_coset_lde(fresh, 0, 16, 8)
    pc.case_coset_lde(fresh, 0, 17, 8)
    pc.case_coset_lde(fresh, 0, 20, 8)


def test_babybear_full_tiles(mk):
    """BabyBear on the 2^10-row tiles with three sub-rounds (r03): 64 KiB tiles of 16 columns x 512 threads (plain first pass, later pass with
    the fused tail) and 32 KiB tiles of the 8 cosets x 256 threads behind the virtual pass - the benchmark's shapes 2^20 and 2^20 -> 2^23."""
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_ntt(fresh, 1, 20, batch=1)
    pc.case_coset_lde(fresh, 1, 20, 8)
    pc.case_ntt(fresh, 1, 21, batch=1)      # + register pass


@pytest.mark.parametrize("field", [0, 1])
def test_lincomb_shared_sweep(mk, field):
    pc.case_lincomb_shared_sweep(lambda f: mk(f, fresh=True), field)


@pytest.mark.parametrize("field", [0, 1])
def test_arith_selftest(mk, field):
    """ADVICE r2 / VERDICT r2 #3: the NTT tiles' arithmetic class op by op against big integers (GPU: the exec-masked asm class GLM itself;
    emulation: the formulas it falls back to - the entry point's plumbing)."""
    pc.case_arith_selftest(mk, field, nrand=1 << 12)


@pytest.mark.parametrize("field", [0, 1])
def test_many_proofs_on_one_context_stay_identical(mk, field):
    """The same proof 80 times on ONE context: the pool of zeroed device words (counters of the deferred-block lists, degree results) wraps and is
    wiped several times on the way - a result that lived in it across a wipe would change (r03: the degree word forwarded by the tree's last launch)."""
    from common import fibonacci_trace
    ctx = mk(field, fresh=True)
    tr = fibonacci_trace(field, 32)
    first = pc.drive(ctx, field, tr, 8, 1, seed=3, read_big=False)
    for _ in range(80):
        assert pc.drive(ctx, field, tr, 8, 1, seed=3, read_big=False) == first


@pytest.mark.parametrize("field,virtual", [(0, "1"), (1, "1"), (0, "0")])
def test_virtual_linear_lde_columns(mk, monkeypatch, field, virtual):
    """r03: the linear LDE columns evaluated row by row inside the leaf-hash kernel (MS_LDE_VIRTUAL; default: AIRs of >= 16 polynomials) instead of being
    written out by the lincomb kernels - same LDE root, same LDE matrix on ms_lde_read (materialised on demand), same proof, forced on and off."""
    monkeypatch.setenv("MS_LDE_VIRTUAL", virtual)
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_prove(fresh, field, 8, 8)
    pc.case_prove(fresh, field, 6, 4, read_big=False)


@pytest.mark.parametrize("field,parents", [(0, "0"), (1, "0"), (0, "4"), (0, "4096"), (1, "1048576"), (0, "16384")])
def test_tree_levels_as_subtree_launches_or_one_by_one(mk, monkeypatch, field, parents):
    """r04: binary-tree levels of at most MS_TREE_SUBTREE_PARENTS parents (default 16384) run nine to a launch with the children in LDS (InnerSubtreeKernel);
    0: one launch per level and the fused top (the r01-r03 path, still what non-binary trees use).  Same roots, paths and proofs either way."""
    monkeypatch.setenv("MS_TREE_SUBTREE_PARENTS", parents)
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_prove(fresh, field, 9, 8, read_big=False)
    pc.case_prove(fresh, field, 3, 2, read_big=False)


@pytest.mark.parametrize("field,small_max", [(0, "0"), (1, "0"), (0, "1000000000"), (1, "1000000000")])
def test_eval_kernel_choice_by_polynomial_length(mk, monkeypatch, field, small_max):
    """r04: polynomials of at most MS_EVAL_SMALL_MAX coefficients (default 2^19) are evaluated with 4 coefficients per thread, longer ones with 16: the DEEP-ALI
    values and every FRI round's B with either kernel forced."""
    monkeypatch.setenv("MS_EVAL_SMALL_MAX", small_max)
    pc.case_prove(lambda f, fresh=False: mk(f, fresh=True), field, 8, 8, read_big=False)


@pytest.mark.parametrize("field,small_max", [(0, "0"), (1, "0"), (0, "1000000000"), (1, "1000000000")])
def test_fold_kernel_choice_by_round_size(mk, monkeypatch, field, small_max):
    """r04: rounds of at most MS_FOLD_SMALL_MAX outputs (default 131072) fold with one output per thread (latency), longer ones with eight (the inversion shared by
    eight norms): the same proof with every round forced through either kernel."""
    monkeypatch.setenv("MS_FOLD_SMALL_MAX", small_max)
    pc.case_prove(lambda f, fresh=False: mk(f, fresh=True), field, 8, 8, read_big=False)


@pytest.mark.parametrize("field,log_n,w", [(0, 4, 4), (1, 4, 4), (0, 5, 6), (1, 3, 5)])
def test_mix_cubic_true_quotient(mk, field, log_n, w):
    """BASELINE configs[4] "degree-3 constraints" (build-defined; VERDICT r2 missing #6): ms_mix_cubic against the big-integer definition, the DEEP-ALI
    identity, a full FRI over the 2N-coefficient validity polynomial, and the refusal of an invalid trace."""
    pc.case_mix_cubic(lambda f, fresh=False: mk(f, fresh=True), field, log_n=log_n, w=w)


@pytest.mark.parametrize("field", [0, 1])
def test_mix_cubic_failing_across_a_store_growth(mk, field):
    """A refused ms_mix_cubic that grew the polynomial store leaves no validity polynomial behind (ms_fri_begin refuses as before any mix stage); one that did not
    grow it leaves the earlier one in place."""
    pc.case_mix_cubic_store_growth(lambda f, fresh=False: mk(f, fresh=True), field)


def test_merkle_commit_vs_reference_script_vectors():
    """The emulation build of the Merkle kernels against the vectors produced by RUNNING the reference's scripts/merkle_tree.py (no oracle in between;
    the GPU suite runs the same case on the HIP build: VERDICT r3 missing #4)."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    pc.case_merkle_script_golden(lambda field, flags: ms.Context(field, flags=flags, lib_path=EMU))


@pytest.mark.parametrize("field,log_n,blowup", [(0, 7, 16), (1, 6, 32), (0, 4, 64), (1, 5, 1)])
def test_prove_other_blowups(mk, field, log_n, blowup):
    pc.case_prove(mk, field, log_n, blowup, read_big=False)


@pytest.mark.parametrize("field,log_n,steps", [(0, 6, 40), (1, 7, 70), (0, 8, 128)])
def test_prove_several_padding_rows(mk, field, log_n, steps):
    pc.case_prove(mk, field, log_n, 8, read_big=False, steps=steps)


@pytest.mark.parametrize("field,flags", [pytest.param(0, 1, id="0"), pytest.param(1, 1, id="1"),
                                         pytest.param(0, 1 | ms.FLAG_LATENCY, id="0-latency"), pytest.param(1, 1 | ms.FLAG_LATENCY, id="1-latency")])
def test_c_abi_never_unwinds(field, flags):
    """SURVEY 8(b) "never unwind" (VERDICT r3 #5): every entry point of libministark runs inside a guard that turns std::bad_alloc into MS_ERR_NOMEM (anything else
    into MS_ERR_HIP).  The emulation build's operator new (hidden: this library's allocations only) can be armed to fail on its N-th call: a whole proof is driven
    with the failure placed at EVERY allocation it makes, one after the other - the stage that hits it must return a negative code (never abort the process, never
    unwind into ctypes), the stages before it succeed, and after EVERY injected failure the same context proves once more with outputs identical to a clean run's (r05).
    The failures leave no resource behind either: the emulated runtime counts what it has handed out (ms_emu_live) - the same after every failure plus recovery proof
    as after a clean proof, and after ms_destroy what it was before ms_create, for the clean context, for a refused ms_create and for the context of the whole sweep."""
    import ctypes as C
    import ownership_cases as oc
    L = oc.load()
    stages = lambda h, outs=None: oc.stages(L, h, field, outs)
    base = oc.live(L)

    # ms_create itself under allocation failure: a negative code, no context
    for k in range(6):
        L.ms_emu_fail_alloc_after(k)
        h = C.c_void_p()
        rc = L.ms_create(C.byref(h), 0, field, flags)
        L.ms_emu_fail_alloc_after(-1)
        assert rc in (0, ms.ERR_NOMEM)
        if rc == 0:
            L.ms_destroy(h)
        else:
            assert not h.value
        assert oc.live(L) == base, (k, rc)
    h = C.c_void_p()
    assert L.ms_create(C.byref(h), 0, field, flags) == 0
    want = []
    assert all(rc == 0 for _, rc in stages(h, want))   # (the first proof also builds the NTT plans, which later proofs reuse)
    L.ms_destroy(h)
    assert oc.live(L) == base                          # one clean proof, then destroy: nothing is left
    assert L.ms_create(C.byref(h), 0, field, flags) == 0
    got = []
    assert all(rc == 0 for _, rc in stages(h, got)) and got == want
    n0 = L.ms_emu_alloc_count()
    assert all(rc == 0 for _, rc in stages(h))
    total = L.ms_emu_alloc_count() - n0
    steady = oc.live(L)                                # what a context that has proved holds
    assert total > 50            # the job tables, plans and error texts do allocate: the guard has something to catch
    hit = 0
    step = 1 if field == 0 else 3          # every allocation of the Goldilocks proof; every third of the BabyBear one (same code paths, twice the extension limbs)
    tried = 0
    for k in range(0, total + 3, step):
        tried += k < total
        L.ms_emu_fail_alloc_after(k)
        failed = oc.first_failure(stages(h))
        L.ms_emu_fail_alloc_after(-1)
        if failed is not None:
            hit += 1
            assert failed[1] in (ms.ERR_NOMEM, ms.ERR_HIP), (k, failed)
            assert L.ms_last_error(h)            # readable, no allocation needed
            # a failure caught by the guard must leave no state behind (pending words of the next tree launch, a swapped knob, a half-counted scope) -
            # the SAME context proves again, and every output of that proof is the clean run's
            got = []
            assert all(rc == 0 for _, rc in stages(h, got)), (k, failed)
            assert got == want, (k, failed, "a proof on the same context after the injected failure differs")
            assert oc.live(L) == steady, (k, failed, "the failed call left a buffer, stream or event behind")
    assert hit == tried, (hit, tried, total)   # every single allocation of a proof, when it fails, surfaces as a negative status of the stage that made it
    L.ms_destroy(h)
    assert oc.live(L) == base
    # after all that the library still proves: same bytes as the oracle
    pc.case_prove(lambda f, fresh=False: ms.Context(f, lib_path=EMU), field, 4, 4, read_big=False)


@pytest.mark.parametrize("field,log_n,blowup,env,root_only,base_z", [(0, 10, 8, {}, False, ()), (1, 9, 8, {"MS_SHARD_SLICES": "4", "MS_SHARD_SLICE_MIN": "1"}, False, (1, 2)),
                                                                    (0, 13, 8, {"MS_SHARD_GATHER_CHUNK": "4096"}, True, ()), (0, 8, 2, {}, False, ()),
                                                                    (0, 10, 8, {"MS_FRI_OVERLAP": "1", "MS_SYNC_POLL": "1"}, False, ()), (1, 9, 8, {"MS_SYNC_POLL": "1", "MS_FRI_TAIL_MAX": "0"}, True, (2,))])
def test_sharded_code_paths_on_one_rank(monkeypatch, field, log_n, blowup, env, root_only, base_z):
    """r04: MS_SHARD_WORLD1=1 lets a one-rank world run the SHARDED prover (coset evaluation, digest exchange, subtree + top, distributed round polynomials with their carry
    chain, query slices, paths through the exchange buffer) inside one process, every exchange a copy to itself: same bytes as the oracle.  The GPU suite runs the same case on
    the real kernels and with RCCL doing the (self-)exchanges inside the library."""
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    st, dist_rounds = pc.case_sharded_paths_on_one_rank(lambda f: ms.Context(f, lib_path=EMU), field, log_n, blowup, root_only=root_only, base_z=base_z)
    assert st[0] >= 3 and st[1] > st[0] and st[2] == 1 and st[3] == 1 and dist_rounds >= 2


def _prove_raw(ctx, field, trace, seed=9, upload=None, read="blocking", prefetch_next=None, wait=True):
    """One proof through the raw ABI on `ctx`; returns (rc of the first failing stage or 0, outputs).  upload = host pointer of a copy of the trace in "page-locked"
    memory (ms_pinned_alloc), read = "blocking" | "async" (ms_fri_proof_read_async + wait into a pinned buffer); prefetch_next = (ptr, N, w) handed to
    ms_trace_upload_async right behind the trace commitment."""
    import ctypes as C
    from common import MODULUS, EXT, SplitMix64, fibonacci_closures
    from oracle import oracle as orc
    p, e = MODULUS[field], EXT[field]
    N, w = trace.shape
    rng = SplitMix64(seed)
    outs = []
    rc, root = ctx.trace_commit_ptr(upload, N, w, 6) if upload else ctx.trace_commit(trace, 6)
    if rc:
        return rc, outs
    outs.append(root)
    if prefetch_next:
        rc = ctx.trace_upload_async(*prefetch_next)
        if rc:
            return rc, outs
    ctx.check(ctx.interpolate())
    for sc, idx in fibonacci_closures(field, N, orc.root_of_unity(field, N)):
        ctx.check(ctx.polys_lincomb(sc, idx))
    rc, root = ctx.lde_commit(8, rng.nonzero(p), 6)
    if rc:
        return rc, outs
    outs.append(root)
    ctx.check(ctx.mix(rng.field(p)))
    rounds = ctx.ceil_log2_k((N - 1) * 8 + 1)
    rc, root = ctx.fri_begin(8, rounds)
    if rc:
        return rc, outs
    outs.append(root)
    for _ in range(1, rounds):
        rc, B = ctx.fri_deep([rng.field(p) for _ in range(e)])
        if rc:
            return rc, outs
        rc, root = ctx.fri_fold_commit([rng.field(p) for _ in range(e)])
        if rc:
            return rc, outs
        outs.append((B.tolist(), root))
    if read == "blocking":
        rc, proof = ctx.fri_query([rng.next(), 5])
        outs.append(proof)
        return rc, outs
    rc, _ = ctx.fri_query([rng.next(), 5], read=False)
    if rc:
        return rc, outs
    n = ctx.fri_proof_size()
    buf = ctx.pinned_alloc(n)          # (not freed here: a copy that never completes may still "own" it - the test's context frees nothing under it either)
    rc = ctx.L.ms_fri_proof_read_async(ctx.h, C.c_void_p(buf))
    if rc == 0 and wait:
        rc = ctx.L.ms_fri_proof_wait(ctx.h)
    if rc == 0 and wait:
        outs.append(C.string_at(buf, n))
    return rc, outs, buf, n


@pytest.mark.parametrize("field", [0, 1])
def test_copy_engine_failures_fail_closed(monkeypatch, field):
    """VERDICT r4 #6 / ADVICE r4: the boundary's engine copies under failure, on the emulation build's scripted engine (MS_EMU_SDMA; rt.hpp).
      ok    - upload and read-back travel "on the engine" and the proof is the plain one; a prefetched trace (ms_trace_upload_async) is found, a prefetch of ANOTHER
              trace is ignored, back-to-back proofs alternate the two device buffers;
      fail  - the engine reports a failed copy (negative completion signal): both transfers are redone through the runtime's copy, same bytes, ms_io_engine says 0;
      hang  - the read-back never completes: MS_ERR_HIP from ms_fri_proof_wait, then MS_ERR_STATE from EVERY entry point (nothing rewrites the blob or re-arms the
              signal under the live copy), and ms_destroy returns; the same for an upload that never completes."""
    import ctypes as C
    import numpy as np
    from common import fibonacci_trace_fast
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    N = 64
    trace = fibonacci_trace_fast(field, N)
    other = fibonacci_trace_fast(field, N, secret_b=11)
    mk = lambda: ms.Context(field, lib_path=EMU)
    monkeypatch.delenv("MS_EMU_SDMA", raising=False)
    plain = mk()
    rc, want = _prove_raw(plain, field, trace)[:2]
    rc2, want_other = _prove_raw(plain, field, other)[:2]
    assert rc == 0 and rc2 == 0 and want != want_other
    assert plain.io_runtime_path() == ""
    plain.close()

    def pinned_copy(ctx, t):
        ptr = ctx.pinned_alloc(t.nbytes)
        C.memmove(ptr, t.ctypes.data, t.nbytes)
        return ptr

    # ---- ok: engine copies, prefetch hit / miss, alternating buffers
    monkeypatch.setenv("MS_EMU_SDMA", "ok")
    ctx = mk()
    pa, pb = pinned_copy(ctx, trace), pinned_copy(ctx, other)
    r = _prove_raw(ctx, field, trace, upload=pa, read="async", prefetch_next=(pb, N, 3))
    assert r[0] == 0 and r[1] == want and ctx.L.ms_io_engine(ctx.h) == 1 and "emulated" in ctx.io_runtime_path()
    r = _prove_raw(ctx, field, other, upload=pb, read="async", prefetch_next=(pb, N, 3))       # the prefetched trace; then a prefetch the next commit does not name
    assert r[0] == 0 and r[1] == want_other
    r = _prove_raw(ctx, field, trace, upload=pa, read="async")                                 # (prefetched: `other`; committed: `trace`)
    assert r[0] == 0 and r[1] == want
    for _ in range(3):                                                                        # back-to-back, each prefetching its successor
        r = _prove_raw(ctx, field, trace, upload=pa, read="async", prefetch_next=(pa, N, 3))
        assert r[0] == 0 and r[1] == want
    ctx.close()

    # ---- fail: the engine reports failure, the runtime's copy delivers
    monkeypatch.setenv("MS_EMU_SDMA", "fail")
    ctx = mk()
    pa = pinned_copy(ctx, trace)
    r = _prove_raw(ctx, field, trace, upload=pa, read="async", prefetch_next=(pa, N, 3))
    assert r[0] == 0 and r[1] == want and ctx.L.ms_io_engine(ctx.h) == 0
    r = _prove_raw(ctx, field, trace, upload=pa, read="async")                                 # (the failed prefetch is redone by the commit)
    assert r[0] == 0 and r[1] == want
    # a failed read-back nobody waited for: the NEXT proof's query phase waits for it (before it rewrites the blob) and redoes it through the runtime's copy - whole proof, right size
    r1 = _prove_raw(ctx, field, trace, upload=pa, read="async", wait=False)
    assert r1[0] == 0
    r2 = _prove_raw(ctx, field, other, read="async")
    assert r2[0] == 0 and r2[1] == want_other and C.string_at(r1[2], r1[3]) == want[-1]
    ctx.close()

    # ---- hang (read-back): poisoned context
    monkeypatch.setenv("MS_EMU_SDMA", "hang")
    monkeypatch.setenv("MS_UPLOAD", "hip")
    ctx = mk()
    r = _prove_raw(ctx, field, trace, read="async")
    assert r[0] == ms.ERR_HIP and "poisoned" in ctx.last_error()
    root = (C.c_uint8 * 32)()
    t = np.ascontiguousarray(trace)
    assert ctx.L.ms_trace_commit(ctx.h, t.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(N), C.c_size_t(3), C.c_size_t(6), root) == ms.ERR_STATE
    assert ctx.L.ms_fri_query(ctx.h, (C.c_uint64 * 2)(3, 5), 2) == ms.ERR_STATE          # would rewrite the blob the engine is still reading
    assert ctx.L.ms_fri_proof_wait(ctx.h) == ms.ERR_STATE and ctx.L.ms_fri_proof_read_async(ctx.h, C.c_void_p(r[2])) == ms.ERR_STATE
    assert ctx.L.ms_interpolate(ctx.h) == ms.ERR_STATE and ctx.L.ms_synchronize(ctx.h) == ms.ERR_STATE
    assert "poisoned" in ctx.last_error()
    ctx.close()                                                                           # waits for the transfer (the scripted engine lets an unlimited wait return), then frees
    monkeypatch.delenv("MS_UPLOAD")

    # ---- hang (upload)
    monkeypatch.setenv("MS_EMU_SDMA", "hang-upload")
    ctx = mk()
    pa = pinned_copy(ctx, trace)
    rc, _ = ctx.trace_commit_ptr(pa, N, 3, 6)
    assert rc == ms.ERR_HIP and "poisoned" in ctx.last_error()
    assert ctx.trace_commit(trace, 6)[0] == ms.ERR_STATE
    ctx.close()
    ctx = mk()                                                                            # a prefetch that never completes surfaces at the commit that needs it
    pa = pinned_copy(ctx, trace)
    assert ctx.trace_upload_async(pa, N, 3) == 0
    assert ctx.trace_commit_ptr(pa, N, 3, 6)[0] == ms.ERR_HIP and ctx.interpolate() == ms.ERR_STATE
    ctx.close()


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup,tail_max,fused", [(8, 8, "0", False), (8, 8, "8192", True), (10, 8, "1048576", True), (9, 2, "1048576", True), (6, 16, "64", True), (11, 1, "4096", True),
                                                        (12, 4, None, True), (12, 8, "1048576", True)])
def test_fri_tail_rounds_fused_and_launch_per_step(monkeypatch, field, log_n, blowup, tail_max, fused):
    """r05: a tail round of the FRI commit phase as ONE launch - fold, DEEP quotient, trimmed length, pointwise codeword, leaf digests with their
    pad-only blocks in place, every tree level, root and length to the host - against the oracle, forced off, at the default threshold and forced far up (several
    evaluation-side workgroups and a tree top for the last one to finish; blowup 1 / 2: scans of more than one block fall back)."""
    def set_env(k, v):
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    pc.case_fri_tail(lambda f: ms.Context(f, lib_path=EMU), field, log_n, blowup, tail_max, set_env, fused)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup", [(4, 8), (9, 8), (12, 4)])
def test_latency_flag_polled_results(field, log_n, blowup):
    """r05: MS_FLAG_LATENCY - the launch that ends a stage raises a sequence number behind its results and the host polls it instead of synchronising (ctx.hpp
    Results::attach / collect; emulated launches are synchronous, so this covers the bookkeeping: every polled stage carried a flag, no stale number is ever waited for),
    evaluation launches that sum their own partials, the trace's range flag riding on the tree's last launch.  The oracle's proof, twice on one context."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    ctx = ms.Context(field, lib_path=EMU, flags=ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_LATENCY)
    for _ in range(2):
        pc.case_prove(lambda f, fresh=False: ctx, field, log_n, blowup, read_big=False)
    pc.case_device_trace_range_check(lambda f, fresh=False: ctx, field, lambda a: (a.ctypes.data, a))
    pc.case_prove(lambda f, fresh=False: ctx, field, 5, 8, read_big=False)   # ... and the context proves on behind the refused trace
    ctx.close()
