"""GPU suite (-m gpu): ms_mix_air_ext on libministark.so (HIP, gfx950) - the cases of tests/test_air_ext_emu.py but the sharded refusal (an emulation-only
set-up, as for ms_mix_air)."""
import os

import pytest

import mini_stark_amd as ms
import air_cases as ac
import air_ext_cases as xc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    build_host_library()

    def mk(field, fresh=True):
        return ms.Context(field)   # raises if the HIP library / GPU is unavailable: no fallback
    return mk


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", ac.DEFINITION_ROWS)
def test_definition(make, field, name, blowup):
    xc.case_definition(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["mimc", "selector"])
@pytest.mark.parametrize("log_n,blowup", [(4, 8), (10, 4), (11, 8)])
def test_base_field_r_reproduces_mix_air(make, field, name, log_n, blowup):
    """N = 16, blowup 8: the tail of one workgroup, and the whole FRI down to the MSFP bytes; N = 2^10, blowup 4: two workgroups and the row-offset wrap;
    N = 2^11, blowup 8: several workgroups"""
    xc.case_base_r(make, field, name, log_n, blowup, full_fri=log_n == 4)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["mimc", "fib_bounded"])
@pytest.mark.parametrize("log_n,blowup", [(10, 4), (11, 8)])
def test_definition_at_extension_points(make, field, name, log_n, blowup):
    xc.case_identity(make, field, name, log_n, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", [("mimc", 4), ("fib_bounded", 2)])
def test_deep_ali_host_function_and_fri(make, field, name, blowup):
    xc.case_deep_and_fri(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_arg_and_state(make, field):
    xc.case_refusals(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_shape_refusal_leaves_the_context_usable(make, field):
    xc.case_shape_refusal_then_both(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_switching_between_the_stages(make, field):
    xc.case_switching(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_polynomial_store_grows(make, field):
    xc.case_store_growth(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_one_launch_and_shared_inverse_table(make, field):
    xc.case_one_launch(make, field)
