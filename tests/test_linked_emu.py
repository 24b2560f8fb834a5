"""ms_query_linked (the query phase of a linked proof in one launch, the MSLQ blob; include/ministark.h) on the emulation build of the kernel code (tests/emu,
-DMS_EMU), against its definition - the bytes of ms_fri_query_index and two ms_tree_open calls - and tests/pyref_linked.py.  The same cases run on the HIP build in
tests/test_linked_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import linked_cases as lc
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
SHA, KECCAK = lc.SHA, lc.KECCAK


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


def test_sharded_context_refuses(make, monkeypatch):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    lc.case_sharded(lc.ctx_of(make, SHA))


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


def test_sanitizer_fixture_is_current(make):
    """tests/golden/linked_tampered.bin, which the stand-alone sanitizer program reads (make -C tests/asan run), is what the drivers give today: the proof, the
    edits, and for every tampered copy the verdict and the step - one copy accepted, every other rejected"""
    out, cases = lc.fixture_bytes(make)
    assert sum(1 for c in cases if c[4] == 1) == 1 and all(c[4] in (0, 1) for c in cases) and len(cases) > 250
    with open(os.path.join(HERE, "golden", "linked_tampered.bin"), "rb") as fh:
        assert fh.read() == out
