"""The linked and the staged flow at the sizes the large kernels run, on the emulation build of the kernel code (tests/emu, -DMS_EMU): shape A (N = 2^11) in full;
on shape B (N = 2^13) the stage ledger of both fields, the knob matrix of Goldilocks, one linked and one staged proof.  Cases and references: tests/scale_cases.py.
The same cases, the other fields and digests of shape B, and shape C (N = 2^16) run on the HIP build in tests/test_scale_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import linked_cases as lc
import scale_cases as sx
import staged_cases as sc
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
SHA = sx.SHA
A, B = sx.SHAPES["A"], sx.SHAPES["B"]


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


@pytest.fixture(scope="module")
def ledger(make):
    """the stage ledger of (shape, field) on a default SHA-256 context, computed once: the test of the ledger and the knob tests share it"""
    done = {}

    def get(N, field):
        if (N, field) not in done:
            done[N, field] = sx.case_stage_ledger(make, SHA, field, N)
        return done[N, field]
    return get


@pytest.mark.parametrize("field", [0, 1])
def test_stage_ledger_shape_a(ledger, field):
    ledger(A, field)


@pytest.mark.parametrize("field", [0, 1])
def test_stage_ledger_shape_b(ledger, field):
    ledger(B, field)


@pytest.mark.parametrize("knob", sorted(sx.KNOBS))
def test_knob_invariance_shape_b(make, ledger, knob):
    sx.case_knob(make, SHA, 0, B, knob, ledger(B, 0))


@pytest.mark.parametrize("field", [0, 1])
def test_staged_ledger_shape_b(make, field):
    sx.case_staged_ledger(make, SHA, field, B)


def test_linked_proof_shape_b(make):
    lc.case_end_to_end(make, SHA, 0, "cubic", N=B, R=0, gb=0)


def test_staged_proof_shape_b(make):
    sc.case_end_to_end(make, SHA, 1, "permutation", N=B, R=10)


def test_staged_proof_rounds_of_the_configuration_shape_b(make):
    sc.case_end_to_end(make, SHA, 0, "logup", N=B, R=0)
