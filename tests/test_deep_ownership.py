"""CPU suite, resource ownership of the composition commitment and the DEEP stage (ms_validity_commit, ms_deep_evals, ms_deep_compose, ms_tree_open of the validity
tree; include/ministark.h), the way tests/test_emu_ownership.py covers the stages before them: on the emulation build, with the n-th host allocation, the n-th device /
page-locked allocation or the n-th handle creation failing for EVERY n of a clean run.  The call that is hit reports a negative status, the same context then gives the
clean run's outputs, and after ms_destroy nothing is live."""
import ctypes as C

import numpy as np
import pytest

import mini_stark_amd as ms
import ownership_cases as oc
from common import MODULUS, EXT, SplitMix64, fibonacci_trace

NEG = (ms.ERR_NOMEM, ms.ERR_HIP)
U64P, U32P = oc.U64P, C.POINTER(C.c_uint32)
TREE_VALIDITY = ms.TREE_VALIDITY


def linked_stages(L, h, field, outs=None, N=16, blowup=4, rounds=3):
    """trace -> LDE -> ms_mix -> ms_validity_commit -> ms_deep_evals -> ms_deep_compose -> FRI commit phase over D' -> rows of the validity tree, as raw C calls:
    yields (name, rc); `outs` collects every output"""
    p, e = MODULUS[field], EXT[field]
    rng = SplitMix64(9)
    root = (C.c_uint8 * 32)()
    t = np.ascontiguousarray(fibonacci_trace(field, N))
    c = 3

    def keep(*vals):
        if outs is not None:
            outs.extend(bytes(v) for v in vals)
    yield "trace_commit", L.ms_trace_commit(h, t.ctypes.data_as(U64P), C.c_size_t(N), C.c_size_t(c), C.c_size_t(c), root)
    yield "interpolate", L.ms_interpolate(h)
    yield "polys_lincomb", L.ms_polys_lincomb(h, (C.c_uint64 * 2)(1, p - 1), (C.c_int * 2)(0, 1), 2)   # a lazily defined polynomial among the opened ones
    yield "lde_commit", L.ms_lde_commit(h, C.c_size_t(blowup), C.c_uint64(rng.nonzero(p)), C.c_size_t(c + 1), root)
    keep(root)
    yield "mix", L.ms_mix(h, C.c_uint64(rng.field(p)))
    yield "validity_commit", L.ms_validity_commit(h, C.c_size_t(1), root)
    keep(root)
    z = (C.c_uint64 * (2 * e))(*[rng.nonzero(p) for _ in range(2 * e)])
    begin, poly = (C.c_uint32 * 3)(0, c + 2, c + 4), (C.c_uint32 * (c + 4))(*(list(range(c + 2)) + [0, c + 1]))
    deep = ms.MsDeep(2, C.cast(z, U64P), C.cast(begin, U32P), C.cast(poly, U32P))
    ev = (C.c_uint64 * ((c + 4) * e))()
    yield "deep_evals", L.ms_deep_evals(h, C.byref(deep), ev)
    keep(ev)
    yield "deep_compose", L.ms_deep_compose(h, C.byref(deep), (C.c_uint64 * e)(*[rng.nonzero(p) for _ in range(e)]))
    yield "fri_begin", L.ms_fri_begin(h, C.c_size_t(blowup), C.c_size_t(rounds), root)
    keep(root)
    B = (C.c_uint64 * (2 * e))()
    for _ in range(1, rounds):
        yield "fri_deep", L.ms_fri_deep(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), B)
        yield "fri_fold_commit", L.ms_fri_fold_commit(h, (C.c_uint64 * e)(*[rng.field(p) for _ in range(e)]), root)
        keep(B, root)
    n = C.c_size_t(0)
    ix = (C.c_uint64 * 2)(N * blowup - 1, 0)
    yield "tree_open size", L.ms_tree_open(h, TREE_VALIDITY, 0, ix, C.c_size_t(2), None, C.c_size_t(0), C.byref(n))
    blob = (C.c_uint8 * max(1, n.value))()
    yield "tree_open", L.ms_tree_open(h, TREE_VALIDITY, 0, ix, C.c_size_t(2), blob, C.c_size_t(n.value), C.byref(n))
    keep(blob)


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
    assert all(rc == 0 for _, rc in linked_stages(L, h, field, want))
    total = count() - c0
    L.ms_destroy(h)
    assert oc.live(L) == base
    assert total > in_create
    hit = set()
    for n in range(in_create, total):
        arm(n)
        rc, h = oc.create(L, field, flags)
        assert rc == 0
        failed = oc.first_failure(linked_stages(L, h, field, []))
        arm(-1)
        assert failed is not None and failed[1] in NEG, (n, failed)
        hit.add(failed[0])
        got = []
        assert all(rc == 0 for _, rc in linked_stages(L, h, field, got)), (n, failed)
        assert got == want, (n, failed)
        L.ms_destroy(h)
        assert oc.live(L) == base, (n, failed)
    if what == "device":
        assert {"validity_commit", "deep_compose"} <= hit, hit


@pytest.mark.parametrize("field", [0, 1])
def test_host_allocation_failures_in_the_new_entry_points(field):
    """A warm context (every buffer grown, every plan built); then the whole linked sequence again with the k-th host allocation failing, for every k: a negative
    status from the call that is hit, nothing more live than before, and the next clean run gives the first one's outputs."""
    L = oc.load()
    base = oc.live(L)
    rc, h = oc.create(L, field)
    assert rc == 0
    want = []
    assert all(rc == 0 for _, rc in linked_stages(L, h, field, want))
    n0 = L.ms_emu_alloc_count()
    assert all(rc == 0 for _, rc in linked_stages(L, h, field, []))
    total = L.ms_emu_alloc_count() - n0
    before = oc.live(L)
    hit = set()
    for k in range(total):
        L.ms_emu_fail_alloc_after(k)
        failed = oc.first_failure(linked_stages(L, h, field, []))
        L.ms_emu_fail_alloc_after(-1)
        assert failed is not None and failed[1] in NEG, (k, failed)
        hit.add(failed[0])
        assert oc.live(L) == before, (k, failed)
    assert {"validity_commit", "deep_evals", "deep_compose"} <= hit, hit
    got = []
    assert all(rc == 0 for _, rc in linked_stages(L, h, field, got))
    assert got == want
    L.ms_destroy(h)
    assert oc.live(L) == base
