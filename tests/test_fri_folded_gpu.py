"""GPU suite (-m gpu): the folded FRI and its verifying side on libministark.so (HIP, gfx950) - the cases of tests/test_fri_folded_emu.py (all but the sharded
context, which runs on the emulation build only), the 2^16-point shape (several workgroups, both halves of the twiddle tables) and the launch counts."""
import os

import pytest

import mini_stark_amd as ms
import fri_folded_cases as fc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu
SHA = fc.SHA


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


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_fold_both_restatements(make, shape, k, field):
    fc.case_fold(make, SHA, field, shape[0], shape[1], k, "mix")


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_fold_and_trees_at_2_16_points(make, k, field):
    """D_0 = 2^16: 512 outputs of every fold (the first, the last, workgroup edges, random ones), the roots under SHA-256, the blob"""
    fc.case_trees_and_blob(make, SHA, field, fc.BIG[0], fc.BIG[1], k, whole=False)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("kind", fc.SOURCES[1:])
def test_fold_other_round0_sources(make, kind, k, field):
    fc.case_fold(make, SHA, field, 64, 8, k, kind)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_edge_challenges(make, k, field):
    fc.case_edge_alphas(make, SHA, field, k)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("d", fc.DIGESTS)
def test_trees_and_blob(make, d, k, field):
    fc.case_trees_and_blob(make, d, field, 64, 8, k)


@pytest.mark.parametrize("d", [fc.ro.BLAKE2S, fc.ro.SHA3_256])
def test_trees_and_blob_other_digests(make, d):
    fc.case_trees_and_blob(make, d, 0, 64, 8, 2)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("shape", [fc.SHAPES[0], fc.SHAPES[2]], ids=lambda s: "%dx%d" % s)
def test_trees_and_blob_other_shapes(make, shape, field):
    fc.case_trees_and_blob(make, SHA, field, shape[0], shape[1], 2 if shape[0] > 8 else 3)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_verifier_and_tampering(make, k, field):
    fc.case_verifier(make, SHA, field, k)


@pytest.mark.parametrize("d", fc.DIGESTS[1:])
def test_verifier_other_digests(make, d):
    fc.case_verifier(make, d, 0, 2)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_state_and_refusals(make, k, field):
    fc.case_refusals(make, SHA, field, k)


@pytest.mark.parametrize("field", [0, 1])
def test_switching_between_legacy_and_folded(make, field):
    fc.case_switching(make, SHA, field)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_latency_context(make, k, field):
    fc.case_fold(make, SHA, field, 64, 8, k, "mix", extra=fc.LATENCY)
    fc.case_fold(make, SHA, field, 64, 8, k, "deep", extra=fc.LATENCY)
    fc.case_trees_and_blob(make, SHA, field, 64, 8, k, extra=fc.LATENCY)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_launch_count(make, k, field):
    fc.case_launch_count(make, SHA, field, k=k)
