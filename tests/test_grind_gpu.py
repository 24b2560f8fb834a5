"""GPU suite (-m gpu): ms_grind / ms_num_queries_grind and the grinding step of the prover mirrors on libministark.so (HIP, gfx950) - the cases of
tests/test_grind_emu.py, plus the 16-bit and 20-bit searches that are too long for the emulation build."""
import os

import pytest

import mini_stark_amd as ms
import grind_cases as gc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu


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
    return mk


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_smallest_nonce(make, d):
    gc.case_smallest(gc.ctx_of(make, d, ms.GOLDILOCKS), d)


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_smallest_nonce_babybear(make, d):
    gc.case_smallest(gc.ctx_of(make, d, ms.BABYBEAR), d, bits_list=[0, 8, 12], seeds=gc.SEEDS[:1])


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_smallest_nonce_16_bits(make, d):
    gc.case_smallest(gc.ctx_of(make, d), d, bits_list=[16], starts=[0])


def test_sha256_20_bits(make):
    gc.case_sha256_20_bits(gc.ctx_of(make, gc.rg.SHA256))


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_forced_splits(make, d):
    gc.case_forced_splits(make, d)


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_many_hits_in_one_launch(make, d):
    gc.case_many_hits(gc.ctx_of(make, d), d, 1 << 22)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("d", gc.DIGESTS)
def test_limits_and_refusals(make, d, field):
    gc.case_limits_and_refusals(gc.ctx_of(make, d, field), d, field, gc.ctx_of(make, d, field))


@pytest.mark.parametrize("field", [0, 1])
def test_num_queries_grind(make, field):
    gc.case_num_queries(make(field, gc.ZAE), field)


@pytest.mark.parametrize("d,field", [(gc.rg.SHA256, 0), (gc.rg.BLAKE3, 0), (gc.rg.KECCAK256, 0), (gc.rg.SHA256, 1)])
def test_whole_proof(make, d, field):
    gc.case_whole_proof(make, d, field, 12)


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_pow_check(make, d):
    gc.case_pow_check(d)
