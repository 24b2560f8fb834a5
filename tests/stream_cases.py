"""Cases of ms_set_stream, ms_synchronize and ms_stream (include/ministark.h, "Streams"): a context on a caller-owned hipStream_t, work left in flight by the entry
points that return unsynchronised, and the 2 ms polling fallback of MS_FLAG_LATENCY (csrc/rt.hpp: sync_flag).  GPU only (tests/test_stream_gpu.py): the emulation
build launches synchronously and cannot see any of this.  References: the C++ oracle for the classic proof (parity_cases.drive on oracle.Session), and for linked
proofs both verifiers (msh_stark_verify_linked and tests/pyref_linked.py, through linked_cases.verdicts) plus the bytes of a proof the same verifiers accepted; every
comparison is exact.

Tools
  on_stream(make, stream)   any of the three factories of tests/ - mk(field, fresh=), make(field, flags, env=None), make_ctx(field) - with set_stream(stream) applied
                            to what it returns: existing cases run unchanged on a caller's stream
  delay(stream, ms)         a device-side wait of a calibrated length on a torch stream (torch.cuda._sleep), and an event recorded behind it
  Hooked(ctx, before, after) the context seen through hooks around every entry point that enqueues work: a delay in front of each, a switch behind each
  concurrent(a, b)          THE CONTROL: with a delay running on `a`, a tiny torch op on `b` completes while a's end event is still unsignalled.  HIP maps streams to
                            few hardware queues (GPU_MAX_HW_QUEUES); two streams on one queue serialise, and a hand-over between them proves nothing.  pick() tries up
                            to four fresh streams and FAILS the case when none runs beside its partner - it neither skips nor passes.
No case can pass vacuously: the controls, and "the delay is still pending when the unsynchronised call returns", are assertions.

Entry points that return with launches in flight, enumerated by reading csrc/ (every path whose last launch comes behind its last collect or stream
synchronisation): ms_interpolate; ms_mix; ms_polys_lincomb with MS_LAZY_LINCOMB=0 (by default it records the combination and launches nothing); ms_bench_lde.  Each
has a hand-over case in three directions (case d).  ms_mix_cubic, ms_mix_terms, ms_mix_air, ms_mix_air_ext (finish_mix: the un-shift behind the exactness check),
ms_aux_running_staged (the interpolation behind aux_columns' wait) and ms_polys_append with no coefficients (a memset) used to be of this kind too, but with a wait
INSIDE the call: no delay can be held in front of their last launch, so a hand-over case behind them could only pass vacuously.  They synchronise behind their last
launch now, and case g holds every entry point outside the list of four to that: the context's stream is idle when the call returns.  ms_fri_proof_read_async is
asynchronous by design, on a copy stream of the context's own.  ms_trace_upload_async queues a copy-engine transfer and launches nothing: no hand-over step.
ms_destroy with work in flight on a caller's stream and sharded contexts are out of scope on purpose (the first would be a use-after-free on a shared GPU if it went
wrong).

Measured on an MI355X (one run of tests/test_stream_gpu.py; calibrate() measures again in every run and asserts the rules, nothing is taken from these lines):
  torch.cuda._sleep     2.39e6 cycles per millisecond
  stage durations       host wall time of one entry point with the stream idle before and after it (an upper bound of its time on the stream), N = 2^12, blowup 8,
                        the slower field, in ms: trace_commit 0.124, interpolate 0.025, polys_lincomb 0.008, lde_commit 0.137, mix 0.029, eval_ext 0.068,
                        fri_begin 0.138, fri_deep 0.039, fri_fold_commit 0.127, fri_query 0.228, mix_air_ext 0.125, validity_commit 0.175, deep_evals 0.138,
                        deep_compose 0.117, query_linked 0.045
  delay                 5.0 ms = max(5 ms, 10 x the slowest stage = 2.28 ms), 2.5 x the polling limit; 5.07 ms measured with events; the cap is 50 ms
  controls              64 picks in the run: the first fresh stream ran beside its partner in 55, the second in 8, the third in 1; none needed the fourth
"""
import inspect
import time

import numpy as np

import mini_stark_amd as ms
import linked_cases as lc
import parity_cases as pc
from common import MODULUS, fibonacci_trace_fast
from oracle import oracle as orc

SHA = lc.SHA
ZAE, LATENCY = 1, ms.FLAG_LATENCY
BLOWUP = 8
POLL_LIMIT_MS = 2.0     # csrc/rt.hpp sync_flag: the spin gives way to the stream synchronisation after 2 ms
MIN_DELAY_MS, MAX_DELAY_MS = 5.0, 50.0
# the entry points of mini_stark_amd.Context that enqueue work on the context's stream
STAGES = frozenset("""trace_commit trace_commit_device aux_running aux_running_staged lde_commit_stage interpolate polys_lincomb polys_append poly_read lde_commit bench_lde
    lde_read mix mix_cubic mix_terms mix_air mix_air_ext air_check validity_read eval_ext fri_begin fri_deep fri_fold_commit fri_round_poly fri_round_codeword fri_query
    fri_proof_read tree_open fri_query_index validity_commit deep_evals deep_compose query_linked grind merkle_commit ntt coset_lde""".split())
UNSYNCHRONISED = frozenset(["interpolate", "mix", "polys_lincomb", "bench_lde"])
REPORT = {}             # what calibrate() and the controls measured in this run (test_stream_gpu.py prints it)


def torch():
    import torch as t   # (only the GPU suite needs it)
    return t


# ---------------------------------------------------------------- tools
def on_stream(make, stream):
    """`make` under its own calling convention, every context it returns moved to `stream` (a torch stream; kept alive by the context object)"""
    params = list(inspect.signature(make).parameters)

    def put(ctx):
        ctx.set_stream(stream.cuda_stream)
        ctx._caller_stream = stream
        assert ctx.stream() == stream.cuda_stream
        return ctx
    if "flags" in params:
        def wrapped(field, flags, env=None):
            return put(make(field, flags, env))
    elif "fresh" in params:
        def wrapped(field, fresh=False):
            return put(make(field, fresh=fresh))
    else:
        def wrapped(field):
            return put(make(field))
    return wrapped


class Hooked:
    """a Context whose entry points in STAGES run between before(name) and after(name); everything else passes through"""

    def __init__(self, ctx, before=None, after=None, replace=None):
        self._ctx, self._before, self._after, self._replace = ctx, before, after, replace or {}

    def __getattr__(self, name):
        attr = self._replace.get(name) or getattr(self._ctx, name)
        if name not in STAGES:
            return attr

        def call(*a, **k):
            if self._before:
                self._before(name)
            out = attr(*a, **k)
            if self._after:
                self._after(name)
            return out
        return call


def delay(stream, ms_=None):
    """enqueues a wait of `ms_` milliseconds (default: the calibrated delay) on `stream`; returns an event recorded behind it"""
    t = torch()
    cal = REPORT["calibration"]
    ms_ = cal["delay_ms"] if ms_ is None else ms_
    assert POLL_LIMIT_MS < ms_ <= MAX_DELAY_MS
    with t.cuda.stream(stream):
        t.cuda._sleep(int(ms_ * cal["cycles_per_ms"]))
        ev = t.cuda.Event()
        ev.record(stream)
    return ev


def own_stream(ctx):
    """the context's OWN stream as a torch stream (the context must be on it)"""
    return torch().cuda.ExternalStream(ctx.stream())


def host_timed(ctx, fn):
    """per-entry-point wall time of fn(hooked ctx) with the stream idle before and after each call: an upper bound of the stage's duration on the stream"""
    took, t0 = {}, [0.0]

    def before(name):
        ctx.synchronize()
        t0[0] = time.perf_counter()

    def after(name):
        ctx.synchronize()
        took[name] = max(took.get(name, 0.0), (time.perf_counter() - t0[0]) * 1e3)
    fn(Hooked(ctx, before, after))
    return took


def classic_trace(field, log_n):
    return fibonacci_trace_fast(field, 1 << log_n)


_ORACLE = {}


def oracle_outputs(field, log_n, read_big, trace=None, key=None):
    """parity_cases.drive on the C++ oracle, once per (field, size, detail)"""
    k = (field, log_n, read_big, key)
    if k not in _ORACLE:
        _ORACLE[k] = pc.drive(orc.Session(field), field, classic_trace(field, log_n) if trace is None else trace, BLOWUP, 2, 77, read_big=read_big)
    return _ORACLE[k]


def classic(sess, field, log_n, read_big=False, trace=None):
    return pc.drive(sess, field, classic_trace(field, log_n) if trace is None else trace, BLOWUP, 2, 77, read_big=read_big)


def assert_oracle(got, want, what):
    assert len(got) == len(want)
    for (ka, va), (kb, vb) in zip(got, want):
        assert ka == kb and va == vb, f"{what}: stage output {ka} differs from the oracle's"


def linked_statement(field, N):
    trace, cons, exempt, periodic, boundary = lc.spec_of("cubic", field, N, 101)
    return trace, (cons, exempt, periodic, boundary)


def linked_by_python(sess, ctx, field, N, R=0, verify=False):
    """a linked proof by the Python driver on `sess` (the context, or a Hooked view of it): the bytes.  verify: accepted by msh_stark_verify_linked and by
    pyref_linked's big-integer verifier (linked_cases.verdicts)"""
    from mini_stark_amd.stark import Stark, StarkConfig
    trace, air = linked_statement(field, N)
    w = trace.shape[1]
    data = Stark(StarkConfig(sess, lc.SECURITY_BITS, lc.BLOWUP, N - 1, w, 0)).prove_air(trace, air, R).to_bytes()
    if verify:
        hs, _cfg = lc.handle(ctx, N, w, 0)
        P = dict(hs=hs, field=field, d=SHA, N=N, w=w, R=R, gb=0, nq=hs.fri_queries, air=air, data=data)
        assert lc.verdicts(P) == (1, "", "")
    return data


_LINKED = {}


def linked_reference(make, field, N):
    """the linked proof of (field, N) proved on a context's own stream and accepted by both verifiers, once"""
    if (field, N) not in _LINKED:
        ctx = make(field, ZAE)
        _LINKED[field, N] = linked_by_python(ctx, ctx, field, N, verify=True)
        ctx.close()
    return _LINKED[field, N]


# ---------------------------------------------------------------- calibration, once per module
def calibrate(make):
    """cycles of torch.cuda._sleep per millisecond (events), the entry points' durations at the largest size the cases use (N = 2^12, both fields, classic and linked),
    and the delay: longer than the polling limit, at least 10 x the slowest stage, at most 50 ms - asserted here, in every run"""
    if "calibration" in REPORT:
        return REPORT["calibration"]
    t = torch()
    assert hasattr(t.cuda, "_sleep"), "this torch build has no torch.cuda._sleep"
    s = t.cuda.Stream()
    cycles, per_ms = 1_000_000, None
    for _ in range(3):       # (the first pass also loads the kernel)
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        with t.cuda.stream(s):
            a.record(s)
            t.cuda._sleep(cycles)
            b.record(s)
        s.synchronize()
        per_ms = cycles / a.elapsed_time(b)
        cycles = int(10 * per_ms)    # then measured at about 10 ms
    stage_ms = {}
    for field in (0, 1):
        ctx = make(field, ZAE)
        for rep in range(2):         # (the first pass allocates and builds the plans)
            took = host_timed(ctx, lambda h: classic(h, field, 12))
            took2 = host_timed(ctx, lambda h: linked_by_python(h, ctx, field, 1 << 12))
        for name, v in list(took.items()) + list(took2.items()):
            stage_ms[name] = max(stage_ms.get(name, 0.0), v)
        ctx.close()
    slowest = max(stage_ms.values())
    delay_ms = max(MIN_DELAY_MS, 10.0 * slowest)
    assert POLL_LIMIT_MS < delay_ms <= MAX_DELAY_MS, (delay_ms, stage_ms)
    REPORT["calibration"] = cal = dict(cycles_per_ms=per_ms, stage_ms={k: round(v, 3) for k, v in sorted(stage_ms.items())}, slowest_stage_ms=round(slowest, 3), delay_ms=delay_ms)
    # the delay is what it says: measured with events, within [0.8 x, 1.5 x] and under the cap
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record(s)
    ev = delay(s)
    b.record(s)
    ev.synchronize()
    s.synchronize()
    cal["delay_measured_ms"] = got = a.elapsed_time(b)
    assert 0.8 * delay_ms <= got <= min(1.5 * delay_ms, MAX_DELAY_MS) and got > POLL_LIMIT_MS, (got, delay_ms)
    return cal


# ---------------------------------------------------------------- the control
_TINY = {}


def tiny_op(stream):
    """one small torch kernel on `stream`, waited for by the host"""
    t = torch()
    if "x" not in _TINY:
        _TINY["x"] = t.zeros(64, device="cuda:0")
        t.cuda.synchronize()
    with t.cuda.stream(stream):
        _TINY["x"].add_(1.0)
    stream.synchronize()


def concurrent(a, b):
    """a tiny op on `b` completes while a delay on `a` is still running"""
    ev = delay(a)
    tiny_op(b)
    ok = not ev.query()
    ev.synchronize()
    return ok


def pick(what, accept, tries=4):
    """a fresh torch stream that accept(stream) finds concurrent with its partners; up to `tries` candidates; records which one passed"""
    t = torch()
    for k in range(tries):
        s = t.cuda.Stream()
        if accept(s):
            REPORT.setdefault("controls", []).append((what, k))
            return s
    raise AssertionError(f"control failed ({what}): none of {tries} fresh streams ran concurrently with its partner - the streams share a hardware queue, "
                         "a hand-over between them would prove nothing")


def streams_for(ctx, direction):
    """(A, B, handle of B) for a hand-over A -> B in direction cc (caller -> caller), co (caller -> own) or oc (own -> caller); the context must be on its own stream"""
    t = torch()
    if direction == "cc":
        a = t.cuda.Stream()
        b = pick("caller -> caller", lambda s: concurrent(a, s))
        return a, b, b.cuda_stream
    own = own_stream(ctx)
    if direction == "co":
        return pick("caller -> own", lambda s: concurrent(s, own)), own, 0
    assert direction == "oc"
    b = pick("own -> caller", lambda s: concurrent(own, s))
    return own, b, b.cuda_stream


def warm(ctx, field, log_n):
    """one classic and one linked proof of the size: every buffer is allocated and every plan built, so the calls under test neither allocate nor free (hipFree waits
    for the whole device, delay included, and would turn a missing order into an accidental one)"""
    classic(ctx, field, log_n, read_big=True)
    linked_by_python(ctx, ctx, field, 1 << log_n)
    assert ctx.bench_lde(BLOWUP, 3) == 0
    ctx.synchronize()


# ---------------------------------------------------------------- a. whole proofs on a caller's stream
def case_whole_proofs(make, field, flags):
    import scale_cases as sx
    import staged_cases as sc
    t = torch()
    s = t.cuda.Stream()
    extra = flags

    def with_flags(field, flags, env=None):
        return make(field, flags | extra, env)

    def mk(field, fresh=False):
        return make(field, ZAE | extra)
    mk3 = on_stream(with_flags, s)
    pc.case_prove(on_stream(mk, s), field, 11, BLOWUP)
    lc.case_end_to_end(mk3, SHA, field, "cubic", N=1 << 10, R=0, gb=0)
    sc.case_end_to_end(mk3, SHA, field, "permutation", N=1 << 10, R=4, gb=0)
    sx.case_stage_ledger(mk3, SHA, field, sx.SHAPES["A"])


# ---------------------------------------------------------------- b. the producer on the same stream, no host synchronisation
def closed_form_trace(field, N):
    """rows (a_i, b_i, a_i + b_i) mod q with a_i = K i^3 + 7 i + 1, b_i = 5 i^2 + 3 (K = 0x1234567): every intermediate below 2^62, so torch's int64 arithmetic on the
    device and Python's integers on the host agree; q = p for BabyBear, 2^61 - 1 for Goldilocks (whose p does not fit int64)"""
    q = MODULUS[field] if field == 1 else (1 << 61) - 1
    K = 0x1234567
    rows = [((K * i**3 + 7 * i + 1) % q, (5 * i * i + 3) % q) for i in range(N)]
    return q, K, np.array([[a, b, (a + b) % q] for a, b in rows], dtype=np.uint64)


def case_producer_same_stream(make, field, flags, log_n=10):
    t = torch()
    N = 1 << log_n
    q, K, host_trace = closed_form_trace(field, N)
    want = oracle_outputs(field, log_n, True, trace=host_trace, key="closed_form")
    ctx = make(field, ZAE | flags)
    warm(ctx, field, log_n)
    s = pick("producer stream beside the own stream", lambda c: concurrent(c, own_stream(ctx)))
    ctx.set_stream(s.cuda_stream)
    dev = t.empty((N, 3), dtype=t.int64, device="cuda:0")
    state = {}

    def produce():                   # torch ops on S; nobody waits for them on the host
        with t.cuda.stream(s):
            i = t.arange(N, dtype=t.int64, device="cuda:0")
            a = (i * i * i * K + 7 * i + 1) % q
            b = (5 * i * i + 3) % q
            dev.copy_(t.stack([a, b, (a + b) % q], dim=1))
    produce()                        # once ahead of time: torch loads its kernels on first use, which takes longer than any delay
    with t.cuda.stream(s):
        dev.zero_()
    s.synchronize()

    def commit_device(_trace, lpn):
        ev = delay(s)
        produce()                    # behind the delay
        assert not ev.query(), "vacuous: the delay in front of the producer ended before ms_trace_commit_device was called"
        out = ctx.trace_commit_device(dev.data_ptr(), N, 3, lpn)
        assert ev.query()
        with t.cuda.stream(s):       # include/ministark.h: the buffer is only read during the call - the rest of the proof must not see this
            dev.fill_(-1)
        state["overwritten"] = True
        return out
    got = classic(Hooked(ctx, replace={"trace_commit": commit_device}), field, log_n, read_big=True, trace=host_trace)   # (ctx.synchronize() is never called)
    assert state.get("overwritten")
    assert_oracle(got, want, "producer on the context's stream")
    s.synchronize()
    assert bool((dev == -1).all())
    ctx.close()


# ---------------------------------------------------------------- c. a delay in front of every stage
def delayed_view(ctx, s):
    """a delay on `s` in front of every entry point; before the next one, the delay in front of a synchronising entry point must have ended: the library waited"""
    st = {"ev": None, "name": None, "n": 0}

    def before(name):
        if st["ev"] is not None and st["name"] not in UNSYNCHRONISED:
            assert st["ev"].query(), f"{st['name']} returned before the work in front of it on its stream had ended"
        st["ev"], st["name"], st["n"] = delay(s), name, st["n"] + 1
    return Hooked(ctx, before), st


def case_delay_every_stage(make, field, flags, log_n=10):
    t = torch()
    ctx = make(field, ZAE | flags)
    warm(ctx, field, log_n)
    s = pick("delayed stream beside the own stream", lambda c: concurrent(c, own_stream(ctx)))   # (a launch that strayed to the own stream would overtake the delay)
    ctx.set_stream(s.cuda_stream)
    view, st = delayed_view(ctx, s)
    got = classic(view, field, log_n, read_big=False)
    assert st["n"] >= 10 + 2 * 12 and st["ev"].query()
    assert_oracle(got, oracle_outputs(field, log_n, False), "a delay in front of every stage")
    view, st = delayed_view(ctx, s)
    data = linked_by_python(view, ctx, field, 1 << log_n)
    assert st["n"] >= 10 and st["ev"].query()
    assert data == linked_reference(make, field, 1 << log_n)
    ctx.synchronize()
    ctx.close()


# ---------------------------------------------------------------- d. hand-over behind an entry point that returns unsynchronised
def handover_view(ctx, point, a, handle_b):
    """the delay on A in front of the FIRST call of `point`, the switch to B right behind it"""
    st = {}

    def before(name):
        if name == point and "ev" not in st:
            st["ev"] = delay(a)

    def after(name):
        if name == point and "switched" not in st:
            assert not st["ev"].query(), f"vacuous: the delay in front of {point} had ended when the call returned (did the call wait?)"
            ctx.set_stream(handle_b)
            st["switched"] = True
    return Hooked(ctx, before, after), st


def case_handover(make, field, flags, point, direction, log_n=10):
    """point: interpolate | mix | polys_lincomb (MS_LAZY_LINCOMB=0) | bench_lde.  The sequence: delay on A, the call with the context on A, set_stream(B), the next
    stage - whose outputs, and everything behind them, must be the oracle's."""
    ctx = make(field, ZAE | flags, {"MS_LAZY_LINCOMB": "0"} if point == "polys_lincomb" else None)
    warm(ctx, field, log_n)
    a, b, handle_b = streams_for(ctx, direction)
    ctx.set_stream(0 if direction == "oc" else a.cuda_stream)
    if point == "bench_lde":
        handover_bench_lde(ctx, field, log_n, a, handle_b)
    else:
        view, st = handover_view(ctx, point, a, handle_b)
        got = classic(view, field, log_n, read_big=True)
        assert st.get("switched")
        assert_oracle(got, oracle_outputs(field, log_n, True), f"hand-over behind {point}, {direction}")
        assert st["ev"].query(), f"the proof behind {point} was finished before the work in front of {point} on the stream that was left"
    ctx.synchronize()
    ctx.close()


def handover_bench_lde(ctx, field, log_n, a, handle_b):
    """ms_bench_lde writes the LDE matrix and returns; the next stage is ms_lde_commit on ANOTHER coset, which writes the same matrix: whichever runs last wins.
    Root and matrix must be the oracle's for the second coset."""
    p = MODULUS[field]
    trace = classic_trace(field, log_n)
    N, w = trace.shape
    shift1, shift2 = 3, 5
    o = orc.Session(field)
    for sess in (o, ctx):
        assert sess.trace_commit(trace, 2 * w)[0] == 0 and sess.interpolate() == 0
        for sc_, idx in pc.fibonacci_closures(field, N, orc.root_of_unity(field, N)):
            assert sess.polys_lincomb(sc_, idx) == 0
    assert 0 < shift1 < p and shift1 != shift2
    want = o.lde_commit(BLOWUP, shift2, 2 * w)
    ctx.synchronize()
    ev = delay(a)
    assert ctx.bench_lde(BLOWUP, shift1) == 0
    assert not ev.query(), "vacuous: the delay in front of ms_bench_lde had ended when the call returned"
    ctx.set_stream(handle_b)
    got = ctx.lde_commit(BLOWUP, shift2, 2 * w)
    assert got[0] == 0 and want[0] == 0 and got[1] == want[1], "LDE root behind ms_bench_lde"
    ev.synchronize()
    a.synchronize()                      # whatever was left on A has run now
    assert (ctx.lde_read() == o.lde_read()).all(), "the LDE matrix behind ms_bench_lde and a switch is not the committed coset's"


# ---------------------------------------------------------------- e. a switch at every stage boundary
def rotating_view(ctx, ring, parity):
    """ring: [(torch stream, handle)] - the context starts on ring[0] and moves to the next stream behind EVERY call.  A delay is armed on the stream about to be left
    in front of every second call (`parity`: which ones; the cases run both).  Delays of one length in front of ALL calls would order the streams by accident - the
    work behind the later delay starts later; this way the call behind a delayed one starts at once on the next stream and overtakes whatever the delayed call left
    in flight, unless the switch orders the two."""
    st = {"at": 0, "n": 0, "delays": 0}

    def before(name):
        if st["n"] % 2 == parity:
            st["ev"] = delay(ring[st["at"]][0])
            st["delays"] += 1

    def after(name):
        st["at"] = (st["at"] + 1) % len(ring)
        ctx.set_stream(ring[st["at"]][1])
        st["n"] += 1
    return Hooked(ctx, before, after), st


def case_switch_every_stage(make, field, flags, log_n=10):
    ctx = make(field, ZAE | flags, {"MS_LAZY_LINCOMB": "0"})
    warm(ctx, field, log_n)
    own = own_stream(ctx)
    a = pick("A beside own", lambda s: concurrent(own, s) and concurrent(s, own))
    b = pick("B beside A and own", lambda s: concurrent(a, s) and concurrent(s, a) and concurrent(s, own) and concurrent(own, s))
    ring = [(a, a.cuda_stream), (b, b.cuda_stream), (own, 0)]
    for parity in (0, 1):
        ctx.set_stream(a.cuda_stream)
        view, st = rotating_view(ctx, ring, parity)
        got = classic(view, field, log_n, read_big=True)
        assert st["n"] >= 3 * len(ring) and st["delays"] >= st["n"] // 2
        assert_oracle(got, oracle_outputs(field, log_n, True), "a switch at every stage boundary (classic proof, delays in front of the calls of parity %d)" % parity)
        ctx.set_stream(a.cuda_stream)
        view, st = rotating_view(ctx, ring, parity)
        data = linked_by_python(view, ctx, field, 1 << log_n)
        assert st["n"] >= 3 * len(ring) and st["delays"] >= st["n"] // 2
        assert data == linked_reference(make, field, 1 << log_n), "a switch at every stage boundary (linked proof, parity %d)" % parity
    ctx.synchronize()
    ctx.close()


# ---------------------------------------------------------------- f. ms_synchronize follows the current stream
def case_synchronize_follows(make, field, flags, log_n=10):
    t = torch()
    ctx = make(field, ZAE | flags)
    warm(ctx, field, log_n)
    own_handle = ctx.stream()
    assert own_handle != 0
    trace = classic_trace(field, log_n)
    s = t.cuda.Stream()
    for stream, handle in ((s, s.cuda_stream), (own_stream(ctx), 0)):
        ctx.set_stream(handle)
        # 0 names the context's own stream, never HIP's null stream (torch's default stream, whose handle is 0)
        assert ctx.stream() == (handle or own_handle) and ctx.stream() != t.cuda.default_stream().cuda_stream
        assert ctx.trace_commit(trace, 6)[0] == 0
        ev = delay(stream)
        assert ctx.interpolate() == 0
        assert not ev.query(), "vacuous: the delay in front of ms_interpolate had ended when the call returned"
        ctx.synchronize()
        assert ev.query(), "ms_synchronize returned with the context's current stream still busy"
        assert (ctx.poly_read(0) == orc.intt(field, trace[:, 0])).all()
    ctx.close()


# ---------------------------------------------------------------- g. every other entry point returns with the stream idle
def idle_view(ctx, stream, seen):
    """behind every entry point outside UNSYNCHRONISED the context's stream has nothing in flight (hipStreamQuery through torch).  One-sided by nature: a launch left
    in flight may have retired by the time of the query, so a pass does not prove the wait; a failure proves its absence."""
    def after(name):
        if name not in UNSYNCHRONISED:
            assert stream.query(), f"{name} returned with work in flight on the context's stream: it belongs in the list of unsynchronised returns, or must wait"
            seen.add(name)
    return Hooked(ctx, None, after)


def case_idle_at_return(make, field):
    """the classic, cubic, terms, AIR, extension-AIR, linked and staged flows (existing cases, unchanged) on a caller's stream, without MS_FLAG_LATENCY - with it a
    stage's results are home when its last kernel has stored them, a moment before the kernel retires"""
    import air_cases as ac
    import air_ext_cases as xc
    import staged_cases as sc
    import terms_cases as tc
    t = torch()
    s = t.cuda.Stream()
    seen = set()

    def make3(field, flags, env=None):
        ctx = make(field, flags, env)
        ctx.set_stream(s.cuda_stream)
        ctx._caller_stream = s
        return idle_view(ctx, s, seen)

    def mk(field, fresh=False):
        return make3(field, ZAE)
    pc.case_prove(mk, field, 10, BLOWUP, read_big=False)
    pc.case_mix_cubic(mk, field)
    tc.case_definition(mk, field, "cubic", 4, 2)
    ac.case_definition(mk, field, "mimc", 4)
    xc.case_definition(mk, field, "mimc", 4)
    lc.case_end_to_end(make3, SHA, field, "cubic", N=1 << 10, R=0, gb=4)
    sc.case_end_to_end(make3, SHA, field, "logup", N=1 << 10, R=4, gb=0)
    view = mk(field)
    trace = classic_trace(field, 10)
    assert view.trace_commit(trace, 6)[0] == 0 and view.interpolate() == 0
    assert view.polys_append([]) == 0 and view.polys_append([1, 2, 3]) == 0
    assert (view.poly_read(3) == 0).all() and view.poly_read(4)[:4].tolist() == [1, 2, 3, 0]
    want = {"mix_cubic", "mix_terms", "mix_air", "mix_air_ext", "aux_running_staged", "polys_append", "trace_commit", "lde_commit", "lde_commit_stage", "eval_ext",
            "validity_commit", "deep_evals", "deep_compose", "fri_begin", "fri_deep", "fri_fold_commit", "fri_query", "query_linked", "grind", "poly_read"}
    assert want <= seen, sorted(want - seen)
    s.synchronize()
