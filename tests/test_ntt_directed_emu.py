"""CPU suite: directed inputs (tests/ntt_directed_cases.py) through the transform kernels of the emulation build (tests/emu, -DMS_EMU), where the sign-bit class
GLT runs as written and GLM falls back to GL's formulas.  The same cases run on the HIP build in tests/test_ntt_directed_gpu.py."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import ntt_directed_cases as nd

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def mk():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    cache = {}

    def make(field, fresh=False):
        if fresh:
            return ms.Context(field, lib_path=EMU)
        if field not in cache:
            cache[field] = ms.Context(field, lib_path=EMU)
        return cache[field]
    return make


@pytest.mark.parametrize("field,log_n", [(f, k) for f in (0, 1) for k in nd.NTT_SIZES[f]])
def test_transform(mk, field, log_n):
    nd.case_transform_reaches(mk(field), field, log_n, nd.NTT_SIZES[field][log_n])


@pytest.mark.parametrize("field,log_n", [(f, k) for f in (0, 1) for k in nd.LDE_SIZES[f]])
def test_coset_lde(mk, field, log_n):
    nd.case_lde_reaches(mk(field), field, log_n, nd.LDE_SIZES[field][log_n])


@pytest.fixture
def mk_regpass(mk, monkeypatch):
    monkeypatch.setenv("MS_NTT_V2_REGPASS", "2")
    monkeypatch.setenv("MS_NTT_V2", "2")
    return lambda field: mk(field, fresh=True)


@pytest.mark.parametrize("log_n", nd.REG_NTT_SIZES)
@pytest.mark.parametrize("field", [0, 1])
def test_register_pass_transform(mk_regpass, field, log_n):
    nd.case_register_pass_transform(mk_regpass, field, log_n)


@pytest.mark.parametrize("log_n", list(nd.REG_LDE_SIZES))
@pytest.mark.parametrize("field", [0, 1])
def test_register_pass_coset_lde(mk_regpass, field, log_n):
    nd.case_register_pass_lde(mk_regpass, field, log_n)
