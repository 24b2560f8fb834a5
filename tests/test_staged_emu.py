"""The staged LDE commitment (ms_aux_running_staged, ms_lde_commit_stage, MS_TREE_LDE_STAGED, the MSLS layout of ms_query_linked; include/ministark.h) on the
emulation build of the kernel code (tests/emu, -DMS_EMU): tests/staged_cases.py.  The same cases run on the HIP build in tests/test_staged_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import staged_cases as sc
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
SHA, KECCAK = sc.SHA, sc.KECCAK


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


@pytest.mark.parametrize("N", [8, 64])
@pytest.mark.parametrize("which", ["permutation", "logup"])
@pytest.mark.parametrize("field", [0, 1])
def test_column_is_the_early_column(make, field, which, N):
    sc.case_columns(make, SHA, field, which, N)


@pytest.mark.parametrize("field", [0, 1])
def test_four_tiles(make, field):
    """N = 1024 with 256-row tiles: the carry and apply launches run"""
    sc.case_columns(make, SHA, field, "permutation", 1024, env={"MS_AUX_TILE": "256"})


@pytest.mark.parametrize("field", [0, 1])
def test_two_staged_calls_before_one_commit(make, field):
    sc.case_columns(make, SHA, field, "logup", 64, two=True)


@pytest.mark.parametrize("field", [0, 1])
def test_form_naming_only_the_last_column(make, field):
    sc.case_columns(make, SHA, field, "permutation", 64, last_only=True)


def test_columns_sponge_digest(make):
    sc.case_columns(make, KECCAK, 1, "permutation", 8)


def test_columns_latency_flag(make):
    """MS_FLAG_LATENCY: the new entry points join the side stream of an earlier proof's rounds"""
    mk = lambda field, flags, env=None: make(field, flags | ms.FLAG_LATENCY, env)   # noqa: E731
    sc.case_columns(mk, SHA, 0, "logup", 64, R=3)
    sc.case_openings(mk, SHA, 1, "permutation", 3)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("field", [0, 1])
def test_openings_and_msls(make, field, R):
    sc.case_openings(make, SHA, field, "permutation" if R == 1 else "logup", R)


def test_openings_sponge_digest(make):
    sc.case_openings(make, KECCAK, 0, "permutation", 3)


@pytest.mark.parametrize("field", [0, 1])
def test_states_and_refusals(make, field):
    sc.case_refusals(make, SHA, field)


def test_sharded_context_refuses(make, monkeypatch):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    sc.case_sharded(sc.ctx_of(make, SHA))


@pytest.mark.parametrize("field", [0, 1])
def test_unstaged_proofs_are_unchanged(make, field):
    sc.case_v1_unchanged(make, SHA, field)


# ---------------------------------------------------------------- linked proofs with running columns: MSLP v2 and the drivers
@pytest.mark.parametrize("which", ["permutation", "logup"])
@pytest.mark.parametrize("field", [0, 1])
def test_end_to_end(make, field, which):
    sc.case_end_to_end(make, SHA, field, which, N=8, R=3, gb=0)


def test_end_to_end_grinding(make):
    sc.case_end_to_end(make, SHA, 0, "logup", N=64, R=4, gb=4)


def test_end_to_end_sponge_digest(make):
    sc.case_end_to_end(make, KECCAK, 1, "permutation", N=8, R=2, gb=4)


@pytest.mark.parametrize("field", [0, 1])
def test_end_to_end_rounds_of_the_configuration(make, field):
    sc.case_end_to_end(make, SHA, field, "permutation", N=64, R=0, gb=0)


@pytest.mark.parametrize("field", [0, 1])
def test_rejections(make, field):
    sc.case_rejections(make, SHA, field)


def test_rejections_with_grinding(make):
    sc.case_rejections(make, SHA, 1, gb=4)


@pytest.mark.parametrize("field", [0, 1])
def test_false_argument(make, field):
    sc.case_false_argument(make, SHA, field)
