"""GPU suite (-m gpu): the composition commitment and the DEEP stage and their verifying side on libministark.so (HIP, gfx950) - the cases of
tests/test_deep_emu.py (all but the sharded context, which runs on the emulation build only)."""
import os

import pytest

import mini_stark_amd as ms
import deep_cases as dc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu
SHA, KECCAK = dc.ro.SHA256, dc.ro.KECCAK256


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


@pytest.mark.parametrize("N", [64, 4096])
@pytest.mark.parametrize("field", [0, 1])
def test_launch_count(make, field, N):
    dc.case_launches(make, field, N)
