"""CPU suite, resource ownership: every device buffer, page-locked buffer, stream, event and copy-engine signal of a context has one owner that frees it (ctx.hpp).
The emulated runtime (tests/emu) counts what it has handed out (ms_emu_live) and can be told to fail its n-th host allocation, its n-th device / page-locked
allocation or its n-th handle creation: whichever call is hit reports an error, leaves the counters where they were, and ms_destroy brings them back to where
they stood before ms_create.  (The same balance around whole proofs: test_emu_parity.py::test_c_abi_never_unwinds.)"""
import ctypes as C

import pytest

import mini_stark_amd as ms
import ownership_cases as oc

NEG = (ms.ERR_NOMEM, ms.ERR_HIP)


@pytest.mark.parametrize("field", [0, 1])
def test_standalone_entry_points_free_their_buffers(field):
    """ms_ntt (64 points), ms_coset_lde (16 -> 64), ms_merkle_commit and ms_merkle_prove (64 leaves), ms_arith_selftest work on device buffers of their own.
    Warm (plans built, staging grown), then every host allocation of the call fails in turn: a negative status and nothing more live than before, each time."""
    L = oc.load()
    base = oc.live(L)
    rc, h = oc.create(L, field)
    assert rc == 0
    for name, call in oc.standalone_calls(L, h, field).items():
        rc, want = call()
        assert rc == 0, name
        n0 = L.ms_emu_alloc_count()
        assert call() == (0, want)
        total = L.ms_emu_alloc_count() - n0
        assert total >= 1, name
        before = oc.live(L)
        for k in range(total):
            L.ms_emu_fail_alloc_after(k)
            rc, _ = call()
            L.ms_emu_fail_alloc_after(-1)
            assert rc in NEG, (name, k, rc)
            assert oc.live(L) == before, (name, k)
        assert call() == (0, want), name
    L.ms_destroy(h)
    assert oc.live(L) == base


@pytest.mark.parametrize("field", [0, 1])
def test_half_built_ntt_plan_goes_with_the_failure(field):
    """A fresh context, one 2^12-point NTT (a plan of several passes and five or more twiddle tables) with every host allocation failing in turn, then ms_destroy:
    a plan is published to the context only when it is complete, the tables of one that is not go with the call that failed."""
    L = oc.load()
    base = oc.live(L)
    n = 1 << 12

    def run(k):
        rc, h = oc.create(L, field)
        assert rc == 0
        d = (C.c_uint64 * n)(*range(n))
        n0 = L.ms_emu_alloc_count()
        L.ms_emu_fail_alloc_after(k)
        rc = L.ms_ntt(h, d, C.c_size_t(n), C.c_size_t(1), 0)
        L.ms_emu_fail_alloc_after(-1)
        made = L.ms_emu_alloc_count() - n0
        if k >= 0:
            assert rc in NEG, (k, rc)
            d2 = (C.c_uint64 * n)(*range(n))
            assert L.ms_ntt(h, d2, C.c_size_t(n), C.c_size_t(1), 0) == 0 and bytes(d2) == want, k   # the same context builds the plan after all
        L.ms_destroy(h)
        assert oc.live(L) == base, k
        return made, bytes(d)
    total, want = run(-1)
    assert total >= 8
    for k in range(total):
        run(k)


LATENCY_UNFUSED = (1 | ms.FLAG_LATENCY, {"MS_FRI_TAIL_MAX": "0"})   # the coefficient side of every FRI round really forks onto the side stream


@pytest.mark.parametrize("what,field,flags,env", [("device", 0, 1, {}), ("device", 1, 1, {}), ("device", 0) + LATENCY_UNFUSED, ("device", 1) + LATENCY_UNFUSED,
                                                  ("handle", 0) + LATENCY_UNFUSED, ("handle", 1) + LATENCY_UNFUSED])
def test_device_allocation_and_handle_failures_leave_nothing(monkeypatch, field, flags, env, what):
    """A fresh context and the N = 16, blowup 4 proof with the n-th device / page-locked allocation failing, for EVERY n of a clean run (ms_create's included); and the
    same with the n-th stream / event creation (MS_FLAG_LATENCY with the fused tail off: the side stream and its event are made one after the other).  The call that
    is hit returns a negative status, the same context then proves with the clean run's outputs, and after ms_destroy nothing is live."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = oc.load()
    arm = L.ms_emu_fail_device_alloc_after if what == "device" else L.ms_emu_fail_handle_after
    count = lambda: oc.made(L)[0 if what == "device" else 1]
    base = oc.live(L)
    c0 = count()
    rc, h = oc.create(L, field, flags)
    assert rc == 0
    in_create = count() - c0
    want = []
    assert all(rc == 0 for _, rc in oc.stages(L, h, field, want))
    total = count() - c0
    L.ms_destroy(h)
    assert oc.live(L) == base
    assert in_create >= (3 if what == "device" else 1) and total > in_create, (in_create, total)
    assert what == "handle" or total >= 50
    for n in range(total):
        arm(n)
        rc, h = oc.create(L, field, flags)
        if n < in_create:
            arm(-1)
            assert rc in NEG and not h.value, (n, rc)
            assert oc.live(L) == base, n
            continue
        assert rc == 0
        failed = oc.first_failure(oc.stages(L, h, field, []))
        arm(-1)
        assert failed is not None and failed[1] in NEG, (n, failed)
        got = []
        assert all(rc == 0 for _, rc in oc.stages(L, h, field, got)), (n, failed)
        assert got == want, (n, failed)
        L.ms_destroy(h)
        assert oc.live(L) == base, (n, failed)


@pytest.mark.parametrize("field", [0, 1])
def test_handle_groups_are_whole_or_absent(monkeypatch, field):
    """Handles that only work together are made one by one and kept only as a whole.  The second (and third) creation of each group is made to fail:
      copy stream + its two events (ms_fri_proof_read_async without a copy engine) - the call reports an error, the next one builds the group and delivers the proof;
      a profile record's two events - the launch reports an error, the next one is recorded; the records of a profile never ended go with the context;
      the two copy-engine signals (scripted engine, MS_EMU_SDMA=ok) - no engine for this context, as when none can be bound: the runtime's copies deliver, no signal is kept.
    (Side stream + event: test_device_allocation_and_handle_failures_leave_nothing.  The per-slice event pairs exist on the RCCL path only, which this build lacks.)"""
    monkeypatch.delenv("MS_EMU_SDMA", raising=False)
    L = oc.load()
    base = oc.live(L)
    handles = lambda: tuple(a - b for a, b in zip(oc.live(L)[2:4], base[2:4]))   # (streams, events) of this test's context
    rc, h = oc.create(L, field)
    assert rc == 0
    want = []
    assert all(rc == 0 for _, rc in oc.stages(L, h, field, want))
    blob = want[-2]                         # (stages: ..., the proof blob, ms_merkle_commit's root)
    buf = L.ms_pinned_alloc(len(blob))
    for n in (1, 2):
        L.ms_emu_fail_handle_after(n)
        rc = L.ms_fri_proof_read_async(h, C.c_void_p(buf))
        L.ms_emu_fail_handle_after(-1)
        assert rc == ms.ERR_HIP and L.ms_fri_proof_wait(h) == 0, n
        assert handles() == (1, 0), n  # the context's own stream, no event: nothing of the group was kept
    assert L.ms_fri_proof_read_async(h, C.c_void_p(buf)) == 0 and L.ms_fri_proof_wait(h) == 0
    assert C.string_at(buf, len(blob)) == blob and handles() == (2, 2)
    # profile records
    assert L.ms_profile_begin(h) == 0
    calls = oc.standalone_calls(L, h, field)
    L.ms_emu_fail_handle_after(1)
    rc, _ = calls["ntt"]()
    L.ms_emu_fail_handle_after(-1)
    assert rc == ms.ERR_HIP and handles() == (2, 2)
    rc, _ = calls["ntt"]()
    assert rc == 0 and handles()[1] > 2 and handles()[1] % 2 == 0
    L.ms_destroy(h)                         # (no ms_profile_end)
    L.ms_pinned_free(C.c_void_p(buf))
    assert oc.live(L) == base
    # the two signals
    monkeypatch.setenv("MS_EMU_SDMA", "ok")
    for fail_second in (False, True):
        rc, h = oc.create(L, field)
        assert rc == 0
        if fail_second:
            L.ms_emu_fail_handle_after(1)   # (the proof's first two handles: the signals, when the trace commitment asks for the engine)
        got = []
        assert all(rc == 0 for _, rc in oc.stages(L, h, field, got))
        L.ms_emu_fail_handle_after(-1)
        assert got == want
        assert oc.live(L)[4] - base[4] == (0 if fail_second else 2)
        L.ms_destroy(h)
        assert oc.live(L) == base
