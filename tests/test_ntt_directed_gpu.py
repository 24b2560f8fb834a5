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


def test_shared_table_instance_is_chosen_by_the_call(mk, monkeypatch):
    """The one instance a call decides, not the plan alone: the first pass behind the virtual pass as the shared-table instance (MODE 3) when several columns meet
    enough tiles.  A Goldilocks blowup-8 evaluation of 2^19 coefficients x 3 columns is the smallest such call - a first pass of 2^10 rows, whose 512 tiles fill the default
    persistent grid - against the oracle, with the launch asserted by name; a context created under MS_NTT_SHARE=0 launches the plain instance and gives the same values."""
    import parity_cases as pc
    shared, plain = (r"msntt::PassKernel2<GL, GLM, false, 10, 3, 512, 3, %d>" % mode for mode in (3, 2))
    v = nd.profiled(mk(0), lambda: pc.case_coset_lde(mk, 0, 19, 8))
    assert v.get(shared, 0) > 0 and plain not in v, v
    coeffs, shift = pc.rand_field(0, (3, 1 << 19), seed=119), 7
    rc, want = mk(0).coset_lde(coeffs, shift, 8 << 19)
    assert rc == 0, mk(0).last_error()
    monkeypatch.setenv("MS_NTT_SHARE", "0")
    ctx = mk(0, fresh=True)
    try:
        got = []
        v = nd.profiled(ctx, lambda: got.append(ctx.coset_lde(coeffs, shift, 8 << 19)))
        assert got[0][0] == 0, ctx.last_error()
        assert v.get(plain, 0) > 0 and shared not in v, v
        assert (got[0][1] == want).all()
    finally:
        ctx.close()


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
