"""GPU suite (-m gpu): a context on a caller-owned stream - whole proofs, a producer on the same stream, a delay in front of every stage (the polling fallback of
MS_FLAG_LATENCY), hand-overs behind the entry points that return unsynchronised, a switch at every stage boundary, ms_synchronize, and the
stream found idle behind every other entry point - on libministark.so (HIP, gfx950).
Cases, tools, controls and the measured numbers: tests/stream_cases.py.  There is no emulation twin: emulated launches are synchronous."""
import os

import pytest

import mini_stark_amd as ms
import stream_cases as st
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu
FLAGS = [0, st.LATENCY]


@pytest.fixture(scope="module")
def make():
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    build_host_library()

    def mk(field, flags, env=None):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            return ms.Context(field, flags=flags)   # raises if the HIP library / GPU is unavailable: no fallback
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    cal = st.calibrate(mk)
    print("stream calibration:", cal)
    yield mk
    print("stream controls (case, index of the candidate that ran concurrently):", st.REPORT.get("controls"))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("field", [0, 1])
def test_whole_proofs_on_a_callers_stream(make, field, flags):
    st.case_whole_proofs(make, field, flags)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("field", [0, 1])
def test_producer_on_the_same_stream_without_host_synchronisation(make, field, flags):
    st.case_producer_same_stream(make, field, flags)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("field", [0, 1])
def test_delay_in_front_of_every_stage(make, field, flags):
    st.case_delay_every_stage(make, field, flags, log_n=10 if field == 0 else 12)


@pytest.mark.parametrize("direction", ["cc", "co", "oc"])
@pytest.mark.parametrize("point", ["interpolate", "mix", "polys_lincomb", "bench_lde"])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("field", [0, 1])
def test_handover_behind_an_unsynchronised_return(make, field, flags, point, direction):
    """cc: caller -> caller, co: caller -> own (set_stream(0)), oc: own -> caller"""
    st.case_handover(make, field, flags, point, direction, log_n=10 + (field + (flags != 0)) % 3)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("field", [0, 1])
def test_switch_at_every_stage_boundary(make, field, flags):
    st.case_switch_every_stage(make, field, flags)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("field", [0, 1])
def test_synchronize_follows_the_current_stream(make, field, flags):
    st.case_synchronize_follows(make, field, flags)


@pytest.mark.parametrize("field", [0, 1])
def test_every_other_entry_point_returns_with_the_stream_idle(make, field):
    st.case_idle_at_return(make, field)
