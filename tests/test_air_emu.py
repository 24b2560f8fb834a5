"""ms_mix_air (build-defined: ms_mix_terms completed to an AIR - exemption sets per constraint, periodic columns, boundary constraints; include/ministark.h) on the
emulation build of the kernel code (tests/emu, -DMS_EMU), against the big-integer restatement of its definition (tests/pyref_air.py), bit for bit against
ms_mix_terms, and by the definition at out-of-domain points.  The same cases run on the HIP build in tests/test_air_gpu.py (-m gpu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mini_stark_amd as ms
import air_cases as ac
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def make():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    build_host_library()

    def mk(field, fresh=True):
        return ms.Context(field, lib_path=EMU)
    return mk


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", ac.DEFINITION_ROWS)
def test_definition(make, field, name, blowup):
    ac.case_definition(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["square", "two_row", "cubic"])
@pytest.mark.parametrize("log_n,blowup", [(4, 8), (10, 4)])
def test_bit_equal_with_mix_terms(make, field, name, log_n, blowup):
    """N = 16: L = 128 is less than one workgroup's share (the tail); N = 2^10, blowup 4: two workgroups and the row-offset wrap at the end of the domain"""
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


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_context_refused(make, monkeypatch, field):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    ac.case_sharded_refused(lambda f: ms.Context(f, lib_path=EMU), field)


@pytest.mark.parametrize("field", [0, 1])
def test_every_allocation_of_the_stage_failing(make, field):
    ac.case_alloc_failures(make, field, C.CDLL(EMU))


def test_python_helpers():
    P = ms.AIR_PERIODIC
    assert P == 0x80000000
    cons = [[(1, [(0, 1)]), (5, [])], [(7, [(P | 1, 0), (0, 2)])]]
    air = ms.flatten_air(cons, [[3], []], [[1, 2], [9]], [(0, 0, 4), (1, 7, 6)])
    assert (air["ncons"], air["nperiodic"], air["nbound"]) == (2, 2, 2)
    assert air["term_begin"].tolist() == [0, 2, 3] and air["coef"].tolist() == [1, 5, 7] and air["fac_begin"].tolist() == [0, 1, 1, 3]
    assert air["fac_poly"].tolist() == [0, P | 1, 0] and air["fac_row"].tolist() == [1, 0, 2]
    assert air["ex_begin"].tolist() == [0, 1, 1] and air["ex_row"].tolist() == [3]
    assert air["per_begin"].tolist() == [0, 2, 3] and air["per_val"].tolist() == [1, 2, 9]
    assert air["bnd_poly"].tolist() == [0, 1] and air["bnd_row"].tolist() == [0, 7] and air["bnd_val"].tolist() == [4, 6]
    assert all(air[k].dtype == t for k, t in ms._native.AIR_ARRAYS)
    none = ms.flatten_air(cons)
    assert none["ex_begin"].tolist() == [0, 0, 0] and none["ex_row"].size == 0 and none["per_begin"].tolist() == [0] and none["nbound"] == 0
    with pytest.raises(ValueError):
        ms.flatten_air(cons, [[3]])
    assert ms.air_rows(cons) == [0, 1, 2] and ms.air_rows([[(1, [(0, 1)])]], [(0, 5, 1)]) == [0, 1]
    s, keep = ms.air_struct(dict(air, ex_row=None))
    assert s.ncons == 2 and s.nbound == 2 and not s.ex_row and s.term_begin[2] == 3 and s.per_val[2] == 9 and keep["ex_row"] is None
    assert isinstance(keep["coef"], np.ndarray)
