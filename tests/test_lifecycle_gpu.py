"""GPU suite (-m gpu): one context through different flows and sizes on libministark.so (HIP, gfx950) - the sequences of tests/test_lifecycle_emu.py with
scale_cases.case_stage_ledger at shape A (N = 2^11) between two small steps, once on the context's own stream and once on a caller's stream with MS_FLAG_LATENCY
(stream_cases.on_stream): asynchronous buffers reused across sizes, which the emulation build cannot show.  Steps and factory: tests/lifecycle_cases.py."""
import os

import pytest

import mini_stark_amd as ms
import lifecycle_cases as lcx
import scale_cases as sx
import stream_cases as st
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def new():
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    build_host_library()
    return lambda field, flags, env=None: lcx.create(field, flags, env)   # raises if the HIP library / GPU is unavailable: no fallback


def ledger(field):
    return lambda S: sx.case_stage_ledger(S.make, sx.SHA, field, sx.SHAPES["A"])


@pytest.mark.parametrize("order", lcx.ORDERS)
@pytest.mark.parametrize("field", [0, 1])
def test_one_context_through_every_flow(new, field, order):
    lcx.case_order(new, field, order, ledger(field))


@pytest.mark.parametrize("order", lcx.ORDERS)
@pytest.mark.parametrize("field", [0, 1])
def test_one_context_through_every_flow_on_a_callers_stream_with_latency(new, field, order):
    import torch
    s = torch.cuda.Stream()

    def latency(field, flags, env=None):
        return new(field, flags | ms.FLAG_LATENCY, env)
    lcx.case_order(st.on_stream(latency, s), field, order, ledger(field))
    s.synchronize()
