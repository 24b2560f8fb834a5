"""GPU suite: contexts come and go.  Every buffer, stream, event and copy-engine signal of a context is freed by its owner when the context is destroyed, behind
the waits ms_destroy performs itself (a read-back or an upload still in flight, the side stream).  Six create -> prove -> destroy cycles in one process, which
between them make every kind of handle, leave work in flight at ms_destroy, and must all give the first cycle's proof.  (Not asserted: free device memory -
it is device-wide, and the device is shared.  The balance of what is allocated and freed is counted on the emulation build: test_emu_ownership.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import mini_stark_amd as ms
from common import MODULUS, EXT, SplitMix64, fibonacci_trace_fast, fibonacci_closures
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

LOG_N, BLOWUP = 10, 8


def prove(ctx, field, trace, upload=None, prefetch=False, read="blocking"):
    """One proof; returns its roots, DEEP values and proof blob.  upload: page-locked copy of the trace (prefetch: handed to ms_trace_upload_async first);
    read: "blocking", "async" (ms_fri_proof_read_async + wait) or "leave" (ms_fri_proof_read_async and no wait: returns (outs, buffer, size))."""
    p, e = MODULUS[field], EXT[field]
    N, w = trace.shape
    rng = SplitMix64(9)
    outs = []
    if prefetch:
        ctx.check(ctx.trace_upload_async(upload, N, w))
    rc, root = ctx.trace_commit_ptr(upload, N, w, 6) if upload else ctx.trace_commit(trace, 6)
    ctx.check(rc)
    outs.append(root)
    ctx.check(ctx.interpolate())
    for sc, idx in fibonacci_closures(field, N, orc.root_of_unity(field, N)):
        ctx.check(ctx.polys_lincomb(sc, idx))
    rc, root = ctx.lde_commit(BLOWUP, rng.nonzero(p), 6)
    ctx.check(rc)
    outs.append(root)
    ctx.check(ctx.mix(rng.field(p)))
    rounds = ctx.ceil_log2_k((N - 1) * BLOWUP + 1)
    rc, root = ctx.fri_begin(BLOWUP, rounds)
    ctx.check(rc)
    outs.append(root)
    for _ in range(1, rounds):
        rc, B = ctx.fri_deep([rng.field(p) for _ in range(e)])
        ctx.check(rc)
        rc, root = ctx.fri_fold_commit([rng.field(p) for _ in range(e)])
        ctx.check(rc)
        outs.append((B.tolist(), root))
    if read == "blocking":
        rc, proof = ctx.fri_query([rng.next(), 5])
        ctx.check(rc)
        return outs + [proof]
    ctx.check(ctx.fri_query([rng.next(), 5], read=False)[0])
    n = ctx.fri_proof_size()
    buf = ctx.pinned_alloc(n)
    ctx.check(ctx.L.ms_fri_proof_read_async(ctx.h, C.c_void_p(buf)))
    if read == "leave":
        return outs, buf, n
    ctx.check(ctx.L.ms_fri_proof_wait(ctx.h))
    outs.append(C.string_at(buf, n))
    ctx.pinned_free(buf)
    return outs


@pytest.mark.parametrize("field", [0, 1])
def test_context_churn(monkeypatch, field):
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    trace = np.ascontiguousarray(fibonacci_trace_fast(field, 1 << LOG_N))
    N, w = trace.shape
    lat = ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_LATENCY

    def latency_ctx():
        monkeypatch.setenv("MS_FRI_TAIL_MAX", "0")   # read at ms_create: no fused tail, the coefficient side of every round forks onto the side stream
        ctx = ms.Context(field, flags=lat)
        monkeypatch.delenv("MS_FRI_TAIL_MAX")
        return ctx

    # 1: the plain proof, which every other cycle must reproduce
    ctx = ms.Context(field)
    want = prove(ctx, field, trace)
    ctx.close()
    # 2: side stream and its event
    ctx = latency_ctx()
    assert prove(ctx, field, trace) == want
    ctx.close()
    # a context nobody used
    ms.Context(field).close()
    # 3: a read-back nobody waited for: ms_destroy does, and the bytes are there afterwards
    ctx = ms.Context(field)
    outs, buf, n = prove(ctx, field, trace, read="leave")
    ctx.close()
    assert outs + [C.string_at(buf, n)] == want
    # 4: the trace prefetched into the second device buffer (page-locked source: a copy engine where one is usable), the read-back on the same path
    ctx = ms.Context(field)
    ctx.pinned_free(buf)
    pt = ctx.pinned_alloc(trace.nbytes)
    C.memmove(pt, trace.ctypes.data, trace.nbytes)
    assert prove(ctx, field, trace, upload=pt, prefetch=True, read="async") == want
    ctx.check(ctx.trace_upload_async(pt, N, w))       # ... and one more prefetch that no commitment picks up: in flight, or just arrived, at ms_destroy
    ctx.close()
    # 5: a profile begun and never ended: its event pairs go with the context
    ctx = ms.Context(field)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    assert prove(ctx, field, trace, upload=pt) == want
    ctx.close()
    # 6: all of it at once
    ctx = latency_ctx()
    ctx.check(ctx.trace_upload_async(pt, N, w))
    outs, buf, n = prove(ctx, field, trace, upload=pt, read="leave")
    ctx.check(ctx.trace_upload_async(pt, N, w))
    ctx.close()
    assert outs + [C.string_at(buf, n)] == want
    # ... and a context created after all that proves the same
    ctx = ms.Context(field)
    assert prove(ctx, field, trace) == want
    ctx.pinned_free(buf)
    ctx.pinned_free(pt)
    ctx.close()
