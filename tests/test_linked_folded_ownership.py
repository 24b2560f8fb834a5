"""CPU suite, resource ownership of the coset-grouped row trees and the folded linked query phase (ms_lde_commit_coset, ms_lde_commit_stage_coset,
ms_validity_commit_coset, ms_tree_open of a coset tree, ms_query_linked_folded; include/ministark.h), the way tests/test_staged_ownership.py covers their plain twins: on
the emulation build, with the n-th host allocation, the n-th device / page-locked allocation or the n-th handle creation failing for EVERY n of a clean run.  The call
that is hit reports a negative status, the same context then completes the sequence with the clean run's outputs, and after ms_destroy nothing is live."""
import ctypes as C

import numpy as np
import pytest

import mini_stark_amd as ms
import ownership_cases as oc
import staged_cases as sc
from common import MODULUS, EXT, SplitMix64

NEG = (ms.ERR_NOMEM, ms.ERR_HIP)
U64P, U32P = oc.U64P, C.POINTER(C.c_uint32)
K = 2   # log_arity of the trees and of the FRI


def folded_stages(L, h, field, outs=None, N=16, blowup=4):
    """trace -> ms_lde_commit_coset -> ms_aux_running_staged -> ms_lde_commit_stage_coset -> leaf groups of the staged tree -> ms_mix_air_ext ->
    ms_validity_commit_coset -> ms_deep_compose -> the folded commit phase -> ms_query_linked_folded, as raw C calls: yields (name, rc); `outs` collects every output"""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(19)
    root = (C.c_uint8 * 32)()
    rows, main, op, fr = sc.permutation_case(field, N, 2100 + field)
    w = len(rows[0])
    t = np.array(rows, dtype=np.uint64)

    def keep(*vals):
        if outs is not None:
            outs.extend(bytes(v) for v in vals)
    yield "trace_commit", L.ms_trace_commit(h, t.ctypes.data_as(U64P), C.c_size_t(N), C.c_size_t(w), C.c_size_t(w), root)
    yield "interpolate", L.ms_interpolate(h)
    yield "lde_commit_coset", L.ms_lde_commit_coset(h, C.c_size_t(blowup), C.c_uint64(rng.nonzero(p)), C.c_int(K), root)
    keep(root)
    s, _keep = ms.aux_struct(ms.flatten_aux(op, fr, e))
    fin, col = (C.c_uint64 * e)(), (C.c_uint64 * (N * e))()
    yield "aux_running_staged", L.ms_aux_running_staged(h, C.byref(s), fin, col)
    keep(fin, col)
    yield "lde_commit_stage_coset", L.ms_lde_commit_stage_coset(h, C.c_int(K), root)
    keep(root)
    n = C.c_size_t(0)
    ix = (C.c_uint64 * 2)((N * blowup >> K) - 1, 0)
    yield "tree_open size", L.ms_tree_open(h, ms.TREE_LDE_STAGED, 0, ix, C.c_size_t(2), None, C.c_size_t(0), C.byref(n))
    blob = (C.c_uint8 * max(1, n.value))()
    yield "tree_open staged", L.ms_tree_open(h, ms.TREE_LDE_STAGED, 0, ix, C.c_size_t(2), blob, C.c_size_t(n.value), C.byref(n))
    keep(blob)
    ident = tuple(sc.k_of(field, 1))
    cons, exempt, periodic, boundary = sc.combined_air(field, N, w, main, [(op, fr)], [ident])
    air, _keep2 = ms.air_struct(ms.flatten_air(cons, exempt, periodic, boundary))
    yield "mix_air_ext", L.ms_mix_air_ext(h, (C.c_uint64 * e)(*[rng.nonzero(p) for _ in range(e)]), C.byref(air))
    L.ms_validity_len.restype = C.c_size_t
    m = e * int(L.ms_validity_len(h)) // N
    yield "validity_commit_coset", L.ms_validity_commit_coset(h, C.c_int(K), root)
    keep(root)
    c = w + e
    z = (C.c_uint64 * e)(*[rng.nonzero(p) for _ in range(e)])
    begin, poly = (C.c_uint32 * 2)(0, c + m), (C.c_uint32 * (c + m))(*range(c + m))
    deep = ms.MsDeep(1, C.cast(z, U64P), C.cast(begin, U32P), C.cast(poly, U32P))
    yield "deep_compose", L.ms_deep_compose(h, C.byref(deep), (C.c_uint64 * e)(*[rng.nonzero(p) for _ in range(e)]))
    yield "fri_begin_folded", L.ms_fri_begin_folded(h, C.c_size_t(blowup), C.c_int(K), root)
    keep(root)
    nc, D0 = C.c_uint64(0), C.c_uint64(0)
    yield "fri_round_info", L.ms_fri_round_info(h, C.c_int(0), C.byref(nc), C.byref(D0))
    R = max(1, ((D0.value // blowup).bit_length() - 1) // K)
    for _ in range(R - 1):
        yield "fri_fold_folded", L.ms_fri_fold_folded(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), root)
        keep(root)
    alpha = (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)])
    yield "fri_fold_final size", L.ms_fri_fold_final(h, alpha, None, C.c_size_t(0), C.byref(n))
    fin = (C.c_uint64 * max(1, n.value * e))()
    yield "fri_fold_final", L.ms_fri_fold_final(h, alpha, fin, C.c_size_t(n.value * e), C.byref(n))
    keep(fin)
    betas = (C.c_uint64 * 2)(5, 2**40 + 3)
    yield "query_linked_folded size", L.ms_query_linked_folded(h, betas, 2, None, C.c_size_t(0), C.byref(n))
    blob = (C.c_uint8 * max(1, n.value))()
    yield "query_linked_folded", L.ms_query_linked_folded(h, betas, 2, blob, C.c_size_t(n.value), C.byref(n))
    keep(blob)


def test_the_sequence_is_a_folded_linked_one():
    L = oc.load()
    rc, h = oc.create(L, 0)
    assert rc == 0
    got = []
    assert all(rc == 0 for _, rc in folded_stages(L, h, 0, got))
    assert got[-1][:4] == b"MSLF" and len(got) >= 9
    L.ms_destroy(h)


@pytest.mark.parametrize("field,flags", [(0, 1), (1, 1), (0, 1 | ms.FLAG_LATENCY), (1, 1 | ms.FLAG_LATENCY)])
def test_device_allocation_failures_leave_nothing(field, flags):
    L = oc.load()
    arm = L.ms_emu_fail_device_alloc_after
    count = lambda: oc.made(L)[0]   # noqa: E731
    base = oc.live(L)
    c0 = count()
    rc, h = oc.create(L, field, flags)
    assert rc == 0
    in_create = count() - c0
    want = []
    assert all(rc == 0 for _, rc in folded_stages(L, h, field, want))
    total = count() - c0
    L.ms_destroy(h)
    assert oc.live(L) == base
    assert total > in_create
    hit = set()
    for n in range(in_create, total):
        arm(n)
        rc, h = oc.create(L, field, flags)
        assert rc == 0
        failed = oc.first_failure(folded_stages(L, h, field, []))
        arm(-1)
        assert failed is not None and failed[1] in NEG, (n, failed)
        hit.add(failed[0])
        got = []
        assert all(rc == 0 for _, rc in folded_stages(L, h, field, got)), (n, failed)
        assert got == want, (n, failed)
        L.ms_destroy(h)
        assert oc.live(L) == base, (n, failed)
    assert {"lde_commit_coset", "lde_commit_stage_coset", "validity_commit_coset", "query_linked_folded"} <= hit, hit


def test_the_sequence_makes_no_handle_of_its_own():
    """streams, events and signals are all made by ms_create, also under MS_FLAG_LATENCY (the folded commit phase forks no side stream): no handle site to fail"""
    L = oc.load()
    for flags in (1, 1 | ms.FLAG_LATENCY):
        c0 = oc.made(L)[1]
        rc, h = oc.create(L, 0, flags)
        assert rc == 0
        in_create = oc.made(L)[1] - c0
        assert all(rc == 0 for _, rc in folded_stages(L, h, 0, []))
        assert oc.made(L)[1] - c0 == in_create
        L.ms_destroy(h)


@pytest.mark.parametrize("field", [0, 1])
def test_host_allocation_failures_in_the_new_entry_points(field):
    """A warm context (every buffer grown, every plan built); then the whole staged sequence again with the k-th host allocation failing, for every k: a negative
    status from the call that is hit, nothing more live than before, and the next clean run gives the first one's outputs."""
    L = oc.load()
    base = oc.live(L)
    rc, h = oc.create(L, field)
    assert rc == 0
    want = []
    assert all(rc == 0 for _, rc in folded_stages(L, h, field, want))
    n0 = L.ms_emu_alloc_count()
    assert all(rc == 0 for _, rc in folded_stages(L, h, field, []))
    total = L.ms_emu_alloc_count() - n0
    before = oc.live(L)
    hit = set()
    for k in range(total):
        L.ms_emu_fail_alloc_after(k)
        failed = oc.first_failure(folded_stages(L, h, field, []))
        L.ms_emu_fail_alloc_after(-1)
        assert failed is not None and failed[1] in NEG, (k, failed)
        hit.add(failed[0])
        assert oc.live(L) == before, (k, failed)
    assert {"lde_commit_coset", "lde_commit_stage_coset", "validity_commit_coset", "query_linked_folded"} <= hit, hit
    got = []
    assert all(rc == 0 for _, rc in folded_stages(L, h, field, got))
    assert got == want
    L.ms_destroy(h)
    assert oc.live(L) == base


# ---------------------------------------------------------------- a whole MSLP v3 proof through the driver (msh_stark_prove_linked_folded)
def _v3_setup(field, flags=1):
    import linked_folded_cases as lf
    from mini_stark_amd.host import HostStark, build_host_library
    build_host_library()
    trace, air, args, nch = lf.statement3(field, "permutation", 16, 1)
    ctx = ms.Context(field, flags=flags, lib_path=oc.EMU)
    return ctx, HostStark(ctx, 20, 8, 15, trace.shape[1], 4), (trace, air, 2, args, nch)


def _drop(ctx, hs):
    hs.__del__()      # (msh_stark_free; the handle's own destructor, a no-op the second time)
    ctx.close()


@pytest.mark.parametrize("field,flags", [(0, 1), (1, 1 | ms.FLAG_LATENCY)])
def test_v3_proof_device_allocation_failures_leave_nothing(field, flags):
    """the n-th device / page-locked allocation of a v3 proof failing, for every n: a negative status and an empty slot, the same context then proves with the clean
    run's bytes, and nothing is live behind it"""
    L = oc.load()
    base = oc.live(L)
    c0 = oc.made(L)[0]
    ctx, hs, a = _v3_setup(field, flags)
    in_create = oc.made(L)[0] - c0
    assert hs.prove_linked_folded(*a) == 0
    want = hs.linked_proof()
    total = oc.made(L)[0] - c0
    assert hs.verify_linked_folded(want, a[1], 16, a[0].shape[1], 2, a[3], a[4]) == (1, "")
    _drop(ctx, hs)
    assert oc.live(L) == base and total > in_create
    for n in range(in_create, total):
        ctx, hs, a = _v3_setup(field, flags)
        L.ms_emu_fail_device_alloc_after(n - in_create)
        rc = hs.prove_linked_folded(*a)
        L.ms_emu_fail_device_alloc_after(-1)
        assert rc in NEG and hs.linked_proof() == b"", (n, rc)
        assert hs.prove_linked_folded(*a) == 0 and hs.linked_proof() == want, n
        _drop(ctx, hs)
        assert oc.live(L) == base, n


@pytest.mark.parametrize("field", [0, 1])
def test_v3_proof_host_allocation_failures(field):
    """a warm context; then the proof again with the k-th host allocation of the library failing, for every k: a negative status, an empty slot, nothing more live,
    and the next clean proof has the first one's bytes"""
    L = oc.load()
    base = oc.live(L)
    ctx, hs, a = _v3_setup(field)
    assert hs.prove_linked_folded(*a) == 0
    want = hs.linked_proof()
    n0 = L.ms_emu_alloc_count()
    assert hs.prove_linked_folded(*a) == 0
    total = L.ms_emu_alloc_count() - n0
    before = oc.live(L)
    assert total > 0
    for k in range(total):
        L.ms_emu_fail_alloc_after(k)
        rc = hs.prove_linked_folded(*a)
        L.ms_emu_fail_alloc_after(-1)
        assert rc in NEG and hs.linked_proof() == b"" and oc.live(L) == before, (k, rc)
    assert hs.prove_linked_folded(*a) == 0 and hs.linked_proof() == want
    _drop(ctx, hs)
    assert oc.live(L) == base
