"""GPU suite (-m gpu): the field-arithmetic corners of tests/arith_cases.py on libministark.so (HIP, gfx950): GL as hipcc lowers it, GLT through v_bitop3_b32,
GLM's inline asm with its hand-managed wait states, BB's Montgomery reductions and the extension towers, every operation on directed operands (all pairs of the
edge sets, the words of their full products) and on 2^16 random pairs, against Python integers.  The cases of tests/test_arith_emu.py, where test_directed_
operands_reach_every_branch counts how often those operands take each branch."""
import os

import pytest

import mini_stark_amd as ms
import arith_cases as ac

pytestmark = pytest.mark.gpu
NRAND = 1 << 16


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
