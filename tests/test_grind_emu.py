"""ms_grind / ms_num_queries_grind (build-defined proof-of-work grinding; include/ministark.h) and the grinding step of the prover mirrors on the emulation build of
the kernel code (tests/emu, -DMS_EMU), against the linear search of tests/pyref_grind.py.  The same cases run on the HIP build in tests/test_grind_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import grind_cases as gc
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def make():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    build_host_library()

    def mk(field, flags, env=None):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            return ms.Context(field, flags=flags, lib_path=EMU)   # the MS_* variables are read by ms_create
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
def test_forced_splits(make, d):
    gc.case_forced_splits(make, d)


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_many_hits_in_one_launch(make, d):
    gc.case_many_hits(gc.ctx_of(make, d), d, 1 << 16)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("d", gc.DIGESTS)
def test_limits_and_refusals(make, d, field):
    gc.case_limits_and_refusals(gc.ctx_of(make, d, field), d, field, gc.ctx_of(make, d, field))


@pytest.mark.parametrize("field", [0, 1])
def test_num_queries_grind(make, field):
    gc.case_num_queries(make(field, gc.ZAE), field)


@pytest.mark.parametrize("d,field", [(gc.rg.SHA256, 0), (gc.rg.BLAKE3, 0), (gc.rg.KECCAK256, 0), (gc.rg.SHA256, 1)])
def test_whole_proof(make, d, field):
    gc.case_whole_proof(make, d, field, 6)


@pytest.mark.parametrize("d", gc.DIGESTS)
def test_pow_check(make, d):
    gc.case_pow_check(d)


def test_sharded_context_grinds(make, monkeypatch):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    gc.case_sharded(gc.ctx_of(make, gc.rg.SHA256))
