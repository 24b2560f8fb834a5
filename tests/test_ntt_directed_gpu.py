"""GPU suite (-m gpu): directed inputs (tests/ntt_directed_cases.py) through the transform kernels of libministark.so (HIP, gfx950) - GLT through v_bitop3_b32 in the
two-sub-round tiles, GLM's inline asm in the three-sub-round tiles and in every radix of the register pass - at the smallest size that selects each instance, with the
instance asserted from the library's own per-kernel profile.  The register-pass tests are the GPU counterpart of test_emu_parity.py::test_ntt_register_last_pass."""
import os

import pytest

import mini_stark_amd as ms
import ntt_directed_cases as nd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk():
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    cache = {}

    def make(field, fresh=False):
        if fresh:
            return ms.Context(field)
        if field not in cache:
            cache[field] = ms.Context(field)  # raises if the HIP library / GPU is unavailable: no fallback
        return cache[field]
    return make


@pytest.mark.parametrize("field,log_n", [(f, k) for f in (0, 1) for k in nd.NTT_SIZES[f]])
def test_transform(mk, field, log_n):
    nd.case_transform_reaches(mk(field), field, log_n, nd.NTT_SIZES[field][log_n])


@pytest.mark.parametrize("field,log_n", [(f, k) for f in (0, 1) for k in nd.LDE_SIZES[f]])
def test_coset_lde(mk, field, log_n):
    nd.case_lde_reaches(mk(field), field, log_n, nd.LDE_SIZES[field][log_n])


@pytest.fixture
def mk_regpass(monkeypatch):
    """contexts created under MS_NTT_V2_REGPASS=2 (ms_create reads the knobs), closed when the test is over"""
    monkeypatch.setenv("MS_NTT_V2_REGPASS", "2")
    monkeypatch.setenv("MS_NTT_V2", "2")
    made = []

    def make(field):
        made.append(ms.Context(field))
        return made[-1]
    yield make
    for ctx in made:
        ctx.close()


@pytest.mark.parametrize("log_n", nd.REG_NTT_SIZES)
@pytest.mark.parametrize("field", [0, 1])
def test_register_pass_transform(mk_regpass, field, log_n):
    nd.case_register_pass_transform(mk_regpass, field, log_n)


@pytest.mark.parametrize("log_n", list(nd.REG_LDE_SIZES))
@pytest.mark.parametrize("field", [0, 1])
def test_register_pass_coset_lde(mk_regpass, field, log_n):
    nd.case_register_pass_lde(mk_regpass, field, log_n)
