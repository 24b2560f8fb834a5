"""GPU suite (-m gpu): the linked and the staged flow at the sizes the large kernels run, on libministark.so (HIP, gfx950) - the cases of tests/test_scale_emu.py on both
fields, the other digests on shape B, and shape C (N = 2^16, L = 2^19), which runs here only.  Cases and references: tests/scale_cases.py.  One context at a time; every
case closes its own."""
import os

import pytest

import mini_stark_amd as ms
import linked_cases as lc
import scale_cases as sx
import staged_cases as sc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu
SHA, BLAKE3, KECCAK = sx.SHA, sx.BLAKE3, sx.KECCAK
A, B, C = sx.SHAPES["A"], sx.SHAPES["B"], sx.SHAPES["C"]


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


@pytest.mark.parametrize("field", [0, 1])
def test_stage_ledger_shape_c(ledger, field):
    ledger(C, field)


@pytest.mark.parametrize("d", [BLAKE3, KECCAK])
@pytest.mark.parametrize("field", [0, 1])
def test_roots_and_openings_other_digests_shape_b(make, field, d):
    sx.case_stage_ledger(make, d, field, B, roots_only=True)


@pytest.mark.parametrize("knob", sorted(sx.KNOBS))
@pytest.mark.parametrize("field", [0, 1])
def test_knob_invariance_shape_b(make, ledger, field, knob):
    sx.case_knob(make, SHA, field, B, knob, ledger(B, field))


@pytest.mark.parametrize("field", [0, 1])
def test_staged_ledger_shape_b(make, field):
    sx.case_staged_ledger(make, SHA, field, B)


@pytest.mark.parametrize("field", [0, 1])
def test_staged_columns_eight_tiles(make, field):
    sc.case_columns(make, SHA, field, "permutation", 1 << 14)


# ---------------------------------------------------------------- whole proofs: the C++ verifier, the big-integer verifier and the Python driver's bytes
@pytest.mark.parametrize("R,gb", [(0, 0), (4, 4)])
@pytest.mark.parametrize("field", [0, 1])
def test_linked_proof_shape_b(make, field, R, gb):
    lc.case_end_to_end(make, SHA, field, "cubic", N=B, R=R, gb=gb)


@pytest.mark.parametrize("d,field", [(BLAKE3, 0), (KECCAK, 1)])
def test_linked_proof_other_digests_shape_b(make, d, field):
    lc.case_end_to_end(make, d, field, "cubic", N=B, R=0, gb=0)


@pytest.mark.parametrize("which", ["permutation", "logup"])
@pytest.mark.parametrize("field", [0, 1])
def test_staged_proof_shape_b(make, field, which):
    sc.case_end_to_end(make, SHA, field, which, N=B, R=10)


@pytest.mark.parametrize("field", [0, 1])
def test_staged_proof_rounds_of_the_configuration_shape_b(make, field):
    sc.case_end_to_end(make, SHA, field, "permutation", N=B, R=0)


@pytest.mark.parametrize("field", [0, 1])
def test_linked_proof_shape_c(make, field):
    lc.case_end_to_end(make, SHA, field, "cubic", N=C, R=0, gb=0)
