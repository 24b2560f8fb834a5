"""GPU suite (-m gpu): BLAKE2s-256 as the context's digest (MS_FLAG_DIGEST_BLAKE2S) on libministark.so (HIP, gfx950), against hashlib - the cases of
tests/test_digest_emu.py at the sizes where every launch shape runs (levels above the subtree threshold, subtree launches, the fused FRI tail)."""
import os

import pytest

import mini_stark_amd as ms
import digest_cases as dc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu


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


def test_flag_selects_blake2s(make):
    dc.case_flag_selects_blake2s(make)


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
def test_every_node(make, field, zae):
    ctx = make(field, dc.B2 | (dc.ZAE if zae else 0))
    for leaf_num, ext, lpn, ic in dc.MERKLE_SHAPES:
        dc.case_every_node(ctx, field, leaf_num, ext, lpn, ic, zae)


@pytest.mark.parametrize("field,zae", [(0, True), (1, True), (0, False)])
def test_binary_tree_every_height(make, field, zae):
    dc.case_every_height(make(field, dc.B2 | (dc.ZAE if zae else 0)), field, 17, zae)


@pytest.mark.parametrize("field", [0, 1])
def test_merkle_prove(make, field):
    dc.case_merkle_prove(make(field, dc.ZAE | dc.B2), field)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("field,lpns", [(0, (6, 16)), (1, (6, 24))])
def test_message_length_edges(make, field, lpns, lazy):
    dc.case_length_edges(make, field, lpns, lazy)


TAIL = [("fused tail", dc.ZAE | dc.B2, {"MS_FRI_TAIL_MAX": "65536"}), ("launch per step", dc.ZAE | dc.B2, {"MS_FRI_TAIL_MAX": "0"}),
        ("latency", dc.ZAE | dc.B2 | dc.LATENCY, None)]


@pytest.mark.parametrize("field", [0, 1])
def test_whole_proof_2_16_rows(make, field):
    """L = 2^19: tree levels above the 16 384-parent subtree threshold, subtree launches and the fused tail all run"""
    dc.case_whole_proof(make, field, 16, 8, variants=TAIL)


def test_whole_proof_2_18_rows(make):
    dc.case_whole_proof(make, 0, 18, 8)


@pytest.mark.parametrize("field,steps,blowup", [(0, 255, 8), (1, 31, 4)])
def test_roundtrip_and_cross_rejection(make, field, steps, blowup):
    dc.case_roundtrip_and_cross_rejection(make, field, steps, blowup)
