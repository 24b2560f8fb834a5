"""One context through different flows and sizes, on the emulation build of the kernel code (tests/emu, -DMS_EMU): the cases of the build-defined stages' suites as
steps on a context that lives through all of them - forward, reversed and forward again, and behind refused stages.  Steps, factory and what is left out:
tests/lifecycle_cases.py.  The same sequences run on the HIP build in tests/test_lifecycle_gpu.py (-m gpu), there also on a caller's stream."""
import os
import subprocess

import pytest

import lifecycle_cases as lcx
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def new():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    build_host_library()
    return lambda field, flags, env=None: lcx.create(field, flags, env, lib_path=EMU)


@pytest.mark.parametrize("order", lcx.ORDERS)
@pytest.mark.parametrize("field", [0, 1])
def test_one_context_through_every_flow(new, field, order):
    lcx.case_order(new, field, order)


def test_shared_factory_shares_and_survives_close(new):
    """the factory itself: the three conventions hand out ONE context per (field, flags, env), close() leaves it alive, release() ends it"""
    S = lcx.Shared(new)
    a = S.mk(0, fresh=True)
    assert a is S.make_ctx(0) is S.make(0, lcx.ZAE) is S.make(0, lcx.ZAE, {}) and S.count == 1
    assert S.make(0, lcx.ZAE, {"MS_FRI_TAIL_MAX": "0"}) is not a and S.make(1, lcx.ZAE) is not a and S.count == 3
    a.close()
    assert a.h is not None and a.root_of_unity(8) > 1 and a.polys_count() == 0
    S.release()
    assert a.h is None and S.count == 0
