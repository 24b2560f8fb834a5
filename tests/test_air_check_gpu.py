"""GPU suite (-m gpu): ms_air_check on libministark.so (HIP, gfx950) - the cases of tests/test_air_check_emu.py but the sharded refusal (an emulation-only set-up, as
for ms_mix_air_ext).  Every comparison is exact, against tests/pyref_air_check.py."""
import os

import pytest

import mini_stark_amd as ms
import air_cases as ac
import air_check_cases as cc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    build_host_library()

    def mk(field, flags=0):
        return ms.Context(field, flags=flags)   # raises if the HIP library / GPU is unavailable: no fallback
    return mk


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", ac.DEFINITION_ROWS)
def test_clean_traces(make, field, name, blowup):
    cc.case_clean(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n", [4, 10])
@pytest.mark.parametrize("which", range(5))
def test_one_planted_fault(make, field, log_n, which):
    """rho in {0, 1, N/2, N-2, N-1}: the row-offset wrap across N-1 -> 0 on either side"""
    cc.case_planted(make, field, log_n, cc.fault_rows(1 << log_n)[which])


@pytest.mark.parametrize("field", [0, 1])
def test_fault_on_an_exempt_row_and_one_row_outside(make, field):
    cc.case_exempt_rows(make, field)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("N", [2, 4, 8, 16, 1 << 8, 1 << 10, 1 << 11, 1 << 12])
def test_dense_constant_constraint(make, field, N):
    """fewer rows than lanes (phantom rows must not be counted), and the tail logic on either side of a workgroup's share"""
    cc.case_dense_constant(make, field, N)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["mimc", "selector"])
def test_dense_random_trace(make, field, name):
    cc.case_dense_random(make, field, name)


@pytest.mark.parametrize("field", [0, 1])
def test_reduction_geometry(make, field):
    cc.case_geometry(make, field)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("N", [16, 1 << 10])
def test_periodic_columns(make, field, N):
    cc.case_periodic(make, field, N)


@pytest.mark.parametrize("field", [0, 1])
def test_boundary_constraints(make, field):
    cc.case_boundary(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_after_interpolate_lincomb_and_append(make, field):
    cc.case_after_interpolate(make, field)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("ext", [1, "E"])
def test_running_columns(make, field, ext):
    cc.case_running(make, field, cc.EXT[field] if ext == "E" else 1)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("mont", [False, True])
def test_context_unchanged(make, field, mont):
    cc.case_unchanged(make, field, mont)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals(make, field):
    cc.case_refusals(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_limits_of_a_longer_trace(make, field):
    cc.case_refusals_large(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_launch_count(make, field):
    cc.case_launch_count(make, field)
