"""GPU suite (-m gpu): ms_mix_air on libministark.so (HIP, gfx950) - the cases of tests/test_air_emu.py, plus the bit-equality with ms_mix_terms at a size of
several workgroups."""
import os

import pytest

import mini_stark_amd as ms
import air_cases as ac
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
    ac.case_definition(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["square", "two_row", "cubic"])
@pytest.mark.parametrize("log_n,blowup", [(4, 8), (10, 4), (11, 8)])
def test_bit_equal_with_mix_terms(make, field, name, log_n, blowup):
    """N = 16: the tail of one workgroup; N = 2^10, blowup 4: two workgroups and the row-offset wrap; N = 2^11, blowup 8: several workgroups"""
    ac.case_terms_equal(make, field, name, log_n, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["mimc", "selector"])
@pytest.mark.parametrize("log_n,blowup", [(10, 4), (11, 8)])
def test_definition_at_random_points(make, field, name, log_n, blowup):
    ac.case_identity_large(make, field, name, log_n, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", [("mimc", 4), ("fib_bounded", 2)])
def test_deep_ali_host_function_and_fri(make, field, name, blowup):
    ac.case_deep_and_fri(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
def test_inverse_table_cache(make, field):
    ac.case_table_cache(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_virtual_columns(make, field):
    ac.case_virtual_columns(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_arg_and_state(make, field):
    ac.case_refusals_arg_state(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_arg_limits_of_a_longer_trace(make, field):
    ac.case_refusals_arg_large(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_shape(make, field):
    ac.case_refusals_shape(make, field)
