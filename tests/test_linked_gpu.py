"""GPU suite (-m gpu): ms_query_linked, the linked-proof drivers and MSLP v1 on libministark.so (HIP, gfx950) - the cases of tests/test_linked_emu.py (all but the
sharded context, which runs on the emulation build only)."""
import os

import pytest

import mini_stark_amd as ms
import linked_cases as lc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu
SHA, KECCAK = lc.SHA, lc.KECCAK


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


@pytest.mark.parametrize("name", ["fib", "cubic", "constant"])
@pytest.mark.parametrize("field", [0, 1])
def test_mslq_equals_its_definition(make, field, name):
    lc.case_definition(make, SHA, field, name)


@pytest.mark.parametrize("field", [0, 1])
def test_mslq_sponge_digest(make, field):
    lc.case_definition(make, KECCAK, field, "fib")


@pytest.mark.parametrize("R,N", [(1, 64), (4, 64), (2, 8)])
@pytest.mark.parametrize("field", [0, 1])
def test_mslq_rounds_and_sizes(make, field, R, N):
    lc.case_definition(make, SHA, field, "cubic", R=R, N=N)


@pytest.mark.parametrize("field", [0, 1])
def test_mslq_width_65(make, field):
    lc.case_definition(make, SHA, field, "wide", N=8)


@pytest.mark.parametrize("field", [0, 1])
def test_mslq_virtual_lde_column(make, field):
    lc.case_virtual_column(make, SHA, field)


@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("R", [1, 3, 4])
def test_one_launch(make, R, nq):
    lc.case_one_launch(make, SHA, R % 2, R, nq)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_and_invariance(make, field):
    lc.case_refusals(make, SHA, field)


# ---------------------------------------------------------------- linked proofs: MSLP v1 and the drivers
@pytest.mark.parametrize("name", ["fib", "cubic"])
@pytest.mark.parametrize("field", [0, 1])
def test_end_to_end(make, field, name):
    lc.case_end_to_end(make, SHA, field, name, N=8, R=3, gb=0)


@pytest.mark.parametrize("field", [0, 1])
def test_end_to_end_grinding(make, field):
    lc.case_end_to_end(make, SHA, field, "cubic", N=64, R=4, gb=4)


@pytest.mark.parametrize("field", [0, 1])
def test_end_to_end_sponge_digest(make, field):
    lc.case_end_to_end(make, KECCAK, field, "fib", N=8, R=2, gb=4)


@pytest.mark.parametrize("field", [0, 1])
def test_end_to_end_rounds_of_the_configuration(make, field):
    lc.case_end_to_end(make, SHA, field, "fib", N=64, R=0, gb=0)


def test_end_to_end_one_round(make):
    lc.case_end_to_end(make, SHA, 1, "fib", N=8, R=1, gb=0)


@pytest.mark.parametrize("field", [0, 1])
def test_redraw_rule(make, field):
    lc.case_redraw_rule(field)


def test_redraw_is_part_of_the_replay(make):
    lc.case_redraw_in_the_verdict(make, 1)


@pytest.mark.parametrize("field", [0, 1])
def test_rejections(make, field):
    lc.case_rejections(make, SHA, field)


def test_rejections_without_grinding(make):
    lc.case_rejections(make, SHA, 1, gb=0)


@pytest.mark.parametrize("field", [0, 1])
def test_false_trace(make, field):
    lc.case_false_trace(make, SHA, field)


@pytest.mark.parametrize("field", [0, 1])
def test_air_encoding_and_rows(make, field):
    lc.case_air_encoding(field)
