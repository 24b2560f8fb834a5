"""CPU suite, resource ownership of the staged LDE commitment (ms_aux_running_staged, ms_lde_commit_stage, ms_tree_open of the staged tree, ms_query_linked's staged
layout; include/ministark.h), the way tests/test_deep_ownership.py covers the stages around them: on the emulation build, with the n-th host allocation, the n-th
device / page-locked allocation or the n-th handle creation failing for EVERY n of a clean run.  The call that is hit reports a negative status, the same context then
completes the staged sequence with the clean run's outputs, and after ms_destroy nothing is live."""
import ctypes as C

import numpy as np
import pytest

import mini_stark_amd as ms
import ownership_cases as oc
import staged_cases as sc
from common import MODULUS, EXT, SplitMix64

NEG = (ms.ERR_NOMEM, ms.ERR_HIP)
U64P, U32P = oc.U64P, C.POINTER(C.c_uint32)
NEW = {"aux_running_staged", "lde_commit_stage", "tree_open staged", "query_linked"}


def staged_stages(L, h, field, outs=None, N=16, blowup=4, rounds=3):
    """trace -> LDE -> ms_aux_running_staged -> ms_lde_commit_stage -> rows of the staged tree -> ms_mix_air_ext -> ms_validity_commit -> ms_deep_compose -> FRI commit
    phase -> ms_query_linked (the staged layout), as raw C calls: yields (name, rc); `outs` collects every output"""
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
    yield "lde_commit", L.ms_lde_commit(h, C.c_size_t(blowup), C.c_uint64(rng.nonzero(p)), C.c_size_t(w), root)
    keep(root)
    s, _keep = ms.aux_struct(ms.flatten_aux(op, fr, e))
    fin, col = (C.c_uint64 * e)(), (C.c_uint64 * (N * e))()
    yield "aux_running_staged", L.ms_aux_running_staged(h, C.byref(s), fin, col)
    keep(fin, col)
    yield "lde_commit_stage", L.ms_lde_commit_stage(h, C.c_size_t(e), root)
    keep(root)
    n = C.c_size_t(0)
    ix = (C.c_uint64 * 2)(N * blowup - 1, 0)
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
    yield "validity_commit", L.ms_validity_commit(h, C.c_size_t(max(1, m)), root)
    keep(root)
    c = w + e
    z = (C.c_uint64 * e)(*[rng.nonzero(p) for _ in range(e)])
    begin, poly = (C.c_uint32 * 2)(0, c + m), (C.c_uint32 * (c + m))(*range(c + m))
    deep = ms.MsDeep(1, C.cast(z, U64P), C.cast(begin, U32P), C.cast(poly, U32P))
    yield "deep_compose", L.ms_deep_compose(h, C.byref(deep), (C.c_uint64 * e)(*[rng.nonzero(p) for _ in range(e)]))
    yield "fri_begin", L.ms_fri_begin(h, C.c_size_t(blowup), C.c_size_t(rounds), root)
    keep(root)
    B = (C.c_uint64 * (2 * e))()
    for _ in range(1, rounds):
        yield "fri_deep", L.ms_fri_deep(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), B)
        yield "fri_fold_commit", L.ms_fri_fold_commit(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), root)
        keep(B, root)
    betas = (C.c_uint64 * 2)(5, 2**40 + 3)
    yield "query_linked size", L.ms_query_linked(h, betas, 2, None, C.c_size_t(0), C.byref(n))
    blob = (C.c_uint8 * max(1, n.value))()
    yield "query_linked", L.ms_query_linked(h, betas, 2, blob, C.c_size_t(n.value), C.byref(n))
    keep(blob)


def test_the_sequence_is_a_staged_one():
    L = oc.load()
    rc, h = oc.create(L, 0)
    assert rc == 0
    got = []
    assert all(rc == 0 for _, rc in staged_stages(L, h, 0, got))
    assert got[-1][:4] == b"MSLS"
    L.ms_destroy(h)


@pytest.mark.parametrize("what,field,flags", [("device", 0, 1), ("device", 1, 1), ("handle", 0, 1 | ms.FLAG_LATENCY), ("device", 1, 1 | ms.FLAG_LATENCY)])
def test_device_allocation_and_handle_failures_leave_nothing(monkeypatch, field, flags, what):
    monkeypatch.setenv("MS_FRI_TAIL_MAX", "0")
    L = oc.load()
    arm = L.ms_emu_fail_device_alloc_after if what == "device" else L.ms_emu_fail_handle_after
    count = lambda: oc.made(L)[0 if what == "device" else 1]   # noqa: E731
    base = oc.live(L)
    c0 = count()
    rc, h = oc.create(L, field, flags)
    assert rc == 0
    in_create = count() - c0
    want = []
    assert all(rc == 0 for _, rc in staged_stages(L, h, field, want))
    total = count() - c0
    L.ms_destroy(h)
    assert oc.live(L) == base
    assert total > in_create
    hit = set()
    for n in range(in_create, total):
        arm(n)
        rc, h = oc.create(L, field, flags)
        assert rc == 0
        failed = oc.first_failure(staged_stages(L, h, field, []))
        arm(-1)
        assert failed is not None and failed[1] in NEG, (n, failed)
        hit.add(failed[0])
        got = []
        assert all(rc == 0 for _, rc in staged_stages(L, h, field, got)), (n, failed)
        assert got == want, (n, failed)
        L.ms_destroy(h)
        assert oc.live(L) == base, (n, failed)
    if what == "device":
        assert {"aux_running_staged", "lde_commit_stage"} <= hit, hit


@pytest.mark.parametrize("field", [0, 1])
def test_host_allocation_failures_in_the_new_entry_points(field):
    """A warm context (every buffer grown, every plan built); then the whole staged sequence again with the k-th host allocation failing, for every k: a negative
    status from the call that is hit, nothing more live than before, and the next clean run gives the first one's outputs."""
    L = oc.load()
    base = oc.live(L)
    rc, h = oc.create(L, field)
    assert rc == 0
    want = []
    assert all(rc == 0 for _, rc in staged_stages(L, h, field, want))
    n0 = L.ms_emu_alloc_count()
    assert all(rc == 0 for _, rc in staged_stages(L, h, field, []))
    total = L.ms_emu_alloc_count() - n0
    before = oc.live(L)
    hit = set()
    for k in range(total):
        L.ms_emu_fail_alloc_after(k)
        failed = oc.first_failure(staged_stages(L, h, field, []))
        L.ms_emu_fail_alloc_after(-1)
        assert failed is not None and failed[1] in NEG, (k, failed)
        hit.add(failed[0])
        assert oc.live(L) == before, (k, failed)
    assert {"aux_running_staged", "lde_commit_stage", "query_linked"} <= hit, hit
    got = []
    assert all(rc == 0 for _, rc in staged_stages(L, h, field, got))
    assert got == want
    L.ms_destroy(h)
    assert oc.live(L) == base
