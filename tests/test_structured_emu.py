"""CPU suite: low-degree, sparse and zero validity polynomials and edge-of-field challenges (tests/structured_cases.py) through the emulation build of the kernel
code (tests/emu, -DMS_EMU) against the oracle, every stage's status and value bit for bit.  The same cases run on the HIP build in tests/test_structured_gpu.py."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import structured_cases as sc

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


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("name", sc.names_for(32))
@pytest.mark.parametrize("field", [0, 1])
def test_structured_2p5_rows(mk, field, name, mode):
    """every support x every challenge mode, with the polynomials, the LDE, every round's polynomial and codeword read back"""
    sc.case_structured(mk(field), field, 5, name, mode)


@pytest.mark.parametrize("name,mode", sc.REDUCED)
@pytest.mark.parametrize("field", [0, 1])
def test_structured_2p11_rows(mk, field, name, mode):
    """D0 up to 2^14: several workgroups per kernel, rounds on either side of the fused tail's limits"""
    sc.case_structured(mk(field), field, 11, name, mode, read_big=False)


@pytest.mark.parametrize("field", [0, 1])
def test_config_rounds_on_low_degree_trace_then_generic_proof(mk, field):
    sc.case_config_rounds_then_generic(mk(field), field)


@pytest.mark.parametrize("log_n", [6, 11])
@pytest.mark.parametrize("field", [0, 1])
def test_edge_challenges(mk, field, log_n):
    sc.case_edge_challenges(mk, field, log_n, read_big=(log_n == 6))
