"""GPU suite (-m gpu): ms_aux_running on libministark.so (HIP, gfx950) - the cases of tests/test_aux_emu.py that do not need the emulation build's hooks."""
import os

import pytest

import mini_stark_amd as ms
import aux_cases as xc
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
@pytest.mark.parametrize("ext_is_e", [False, True])
@pytest.mark.parametrize("op", [xc.SUM, xc.PRODUCT])
@pytest.mark.parametrize("nfrac", [1, 3])
@pytest.mark.parametrize("N", [16, 64])
def test_definition(make, field, ext_is_e, op, nfrac, N):
    xc.case_definition(make, field, xc.EXT[field] if ext_is_e else 1, op, nfrac, N)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("op", [xc.SUM, xc.PRODUCT])
@pytest.mark.parametrize("N", xc.BOUNDARY_SIZES)
def test_tile_boundaries(make, field, op, N):
    xc.case_boundaries(make, field, N, op, 2)


@pytest.mark.parametrize("field", [0, 1])
def test_carry_chunk_boundary(make, field):
    xc.case_boundaries(make, field, xc.CHUNK_SIZE, xc.PRODUCT, 1)


@pytest.mark.parametrize("field", [0, 1])
def test_several_columns(make, field):
    xc.case_several(make, field)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("ext_is_e", [False, True])
@pytest.mark.parametrize("which", ["permutation", "logup"])
def test_column_proves(make, field, ext_is_e, which):
    xc.case_end_to_end(make, field, xc.EXT[field] if ext_is_e else 1, which)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("ext_is_e", [False, True])
def test_spoiled_permutation(make, field, ext_is_e):
    xc.case_spoiled_permutation(make, field, xc.EXT[field] if ext_is_e else 1)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals(make, field):
    xc.case_refusals(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_zero_denominator(make, field):
    xc.case_zero_denominator(make, field)
