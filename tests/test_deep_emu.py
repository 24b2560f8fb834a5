"""The composition commitment and the DEEP stage (ms_validity_commit, ms_deep_evals, ms_deep_compose, ms_tree_open(MS_TREE_VALIDITY); include/ministark.h) and their
verifying side (msh_deep_link_verify, msh_validity_from_chunks) on the emulation build of the kernel code (tests/emu, -DMS_EMU), against tests/pyref_deep.py.  The
same cases run on the HIP build in tests/test_deep_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import deep_cases as dc
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
SHA, KECCAK = dc.ro.SHA256, dc.ro.KECCAK256


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
@pytest.mark.parametrize("deg", [2, 3, 5])
@pytest.mark.parametrize("ext", [False, True], ids=["mix_air", "mix_air_ext"])
@pytest.mark.parametrize("field", [0, 1])
def test_chunks_and_tree(make, field, ext, deg, N):
    dc.case_chunks_tree(make, SHA, field, ext, deg, N)


@pytest.mark.parametrize("field", [0, 1])
def test_chunks_and_tree_sponge_digest(make, field):
    dc.case_chunks_tree(make, KECCAK, field, True, 3, 8)


@pytest.mark.parametrize("c", [1, 3, 65])
@pytest.mark.parametrize("field", [0, 1])
def test_evaluations(make, field, c):
    dc.case_evals(make, field, c)


@pytest.mark.parametrize("N,c,npts", [(8, 1, 1), (8, 65, 3), (2048, 1, 2), (4096, 1, 8), (4096, 65, 8)])
@pytest.mark.parametrize("field", [0, 1])
def test_polynomial(make, field, N, c, npts):
    dc.case_poly(make, field, N, c, npts)


@pytest.mark.parametrize("gamma,zkind,npts", [("zero", "full", 2), ("one", "full", 3), ("base", "full", 2), ("full", "base", 2), ("full", "full", 8), ("base", "base", 8)])
@pytest.mark.parametrize("field", [0, 1])
def test_polynomial_edge_challenges(make, field, gamma, zkind, npts):
    dc.case_poly(make, field, 8, 3, npts, gamma=gamma, zkind=zkind)


@pytest.mark.parametrize("name", ["fib", "cubic"])
@pytest.mark.parametrize("field", [0, 1])
def test_end_to_end(make, field, name):
    dc.case_end_to_end(make, SHA, field, name)


def test_end_to_end_sponge_digest(make):
    dc.case_end_to_end(make, KECCAK, 1, "fib")


@pytest.mark.parametrize("field", [0, 1])
def test_rows_of_a_round_0_domain_smaller_than_the_lde(make, field):
    dc.case_small_domain(make, SHA, field)


@pytest.mark.parametrize("field", [0, 1])
def test_splice_is_rejected(make, field):
    dc.case_splice(make, SHA, field)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals(make, field):
    dc.case_refusals(make, field)


@pytest.mark.parametrize("d,field", [(SHA, 0), (SHA, 1), (KECCAK, 0)])
def test_proof_bytes_unchanged_without_compose(make, d, field):
    dc.case_invariance(make, d, field)


def test_sharded_context_refuses(make, monkeypatch):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    dc.case_sharded(dc.ctx_of(make, SHA))


@pytest.mark.parametrize("N", [64, 4096])
@pytest.mark.parametrize("field", [0, 1])
def test_launch_count(make, field, N):
    dc.case_launches(make, field, N)
