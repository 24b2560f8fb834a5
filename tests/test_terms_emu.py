"""ms_mix_terms (build-defined: polynomial AIR constraints of any degree; include/ministark.h) on the emulation build of the kernel code (tests/emu, -DMS_EMU), against the
big-integer restatement of its definition (tests/pyref_terms.py), bit for bit against ms_mix_cubic, and by the DEEP-ALI identity.  The same cases run on the HIP build
in tests/test_terms_gpu.py (-m gpu)."""
import ctypes as C
import os
import subprocess

import pytest

import mini_stark_amd as ms
import terms_cases as tc
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
@pytest.mark.parametrize("name,blowup,vl_over_n", tc.DEFINITION_ROWS)
def test_definition_degree_by_degree(make, field, name, blowup, vl_over_n):
    tc.case_definition(make, field, name, blowup, vl_over_n)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,w,blowup", [(4, 4, 8), (10, 8, 4)])
def test_bit_equal_with_mix_cubic(make, field, log_n, w, blowup):
    """N = 16: L = 128 is less than one workgroup's share (the tail); N = 2^10, blowup 4: two workgroups and the row-offset wrap at the end of the domain"""
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


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_context_refused(make, monkeypatch, field):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    tc.case_sharded_refused(lambda f: ms.Context(f, lib_path=EMU), field)


@pytest.mark.parametrize("field", [0, 1])
def test_every_allocation_of_the_stage_failing(make, field):
    tc.case_alloc_failures(make, field, C.CDLL(EMU))


def test_python_helpers():
    cons = [[(1, [(0, 1)]), (5, [])], [(7, [(1, 0), (0, 2)])]]
    tb, cf, fb, fp, fr = ms.flatten_terms(cons)
    assert tb.tolist() == [0, 2, 3] and cf.tolist() == [1, 5, 7] and fb.tolist() == [0, 1, 1, 3] and fp.tolist() == [0, 1, 0] and fr.tolist() == [1, 0, 2]
    assert ms.terms_rows(cons) == [0, 1, 2]
