"""CPU suite: the field-arithmetic corners of tests/arith_cases.py through the emulation build of the kernel code (tests/emu, -DMS_EMU): every arithmetic class of
csrc/field.hpp (GLM falls back to GL's formulas and GLT's fold_small / mul_x32 / mul_x64 here) and the extension towers on directed operands, and the count of
how often those operands take each branch.  The same cases run on the HIP build in tests/test_arith_gpu.py."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import arith_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
NRAND = 1 << 12


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


def test_directed_operands_reach_every_branch():
    """reference only: no library involved"""
    ac.case_coverage()


@pytest.mark.parametrize("op", [0, 1, 2, 3])
@pytest.mark.parametrize("cls", [1, 2, 3])
def test_goldilocks_all_pairs(mk, cls, op):
    ac.case_gl_pairs(mk, cls, op, NRAND)


@pytest.mark.parametrize("cls", [1, 2, 3])
def test_goldilocks_shifts_and_folds(mk, cls):
    ac.case_gl_single(mk, cls, NRAND)


@pytest.mark.parametrize("cls", [1, 2])
def test_goldilocks_reduce128_raw(mk, cls):
    ac.case_gl_reduce128(mk, cls, NRAND)


def test_goldilocks_round1_shift_and_inverse(mk):
    ac.case_gl_own(mk, NRAND)


def test_goldilocks_class0_unchanged(mk):
    ac.case_class0_is_glm(mk, NRAND)


def test_babybear(mk):
    ac.case_bb(mk, NRAND)


@pytest.mark.parametrize("field,op", [(f, op) for f in (0, 1) for op in ac.ext_ops(f)])
def test_extension(mk, field, op):
    ac.case_ext(mk, field, op)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals(mk, field):
    ac.case_refusals(mk, field)
