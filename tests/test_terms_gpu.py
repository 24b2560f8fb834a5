"""GPU suite (-m gpu): ms_mix_terms on libministark.so (HIP, gfx950) - the cases of tests/test_terms_emu.py, plus the bit-equality with ms_mix_cubic at a size
of several workgroups."""
import os

import pytest

import mini_stark_amd as ms
import terms_cases as tc
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
@pytest.mark.parametrize("name,blowup,vl_over_n", tc.DEFINITION_ROWS)
def test_definition_degree_by_degree(make, field, name, blowup, vl_over_n):
    tc.case_definition(make, field, name, blowup, vl_over_n)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,w,blowup", [(4, 4, 8), (10, 8, 4), (11, 8, 8)])
def test_bit_equal_with_mix_cubic(make, field, log_n, w, blowup):
    """N = 16: the tail of one workgroup; N = 2^10, blowup 4: two workgroups and the row-offset wrap; N = 2^11, blowup 8: several workgroups"""
    tc.case_cubic_equal(make, field, log_n, w, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,log_n,blowup", [("square", 10, 2), ("deg5", 10, 8), ("square", 11, 4), ("deg5", 11, 8)])
def test_identity_at_random_points(make, field, name, log_n, blowup):
    tc.case_identity_large(make, field, name, log_n, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", [("two_row", 4), ("deg5", 8)])
def test_deep_ali_host_function_and_fri(make, field, name, blowup):
    tc.case_deep_and_fri(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
def test_virtual_columns(make, field):
    tc.case_virtual_columns(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_arg_and_state(make, field):
    tc.case_refusals_arg_state(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_shape(make, field):
    tc.case_refusals_shape(make, field)
