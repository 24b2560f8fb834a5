"""GPU suite (-m gpu): BLAKE3 as the context's digest (MS_FLAG_DIGEST_BLAKE3) on libministark.so (HIP, gfx950), against tests/pyref_blake3.py - the cases of
tests/test_blake3_emu.py at the sizes where every launch shape runs (levels above the subtree threshold, subtree launches, the fused FRI tail)."""
import os

import pytest

import mini_stark_amd as ms
import blake3_cases as bc
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


def test_flag_selects_blake3(make):
    bc.case_flag_selects_blake3(make)


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
def test_every_node(make, field, zae):
    ctx = make(field, bc.B3 | (bc.ZAE if zae else 0))
    for leaf_num, ext, lpn, ic in bc.MERKLE_SHAPES:
        bc.case_every_node(ctx, field, leaf_num, ext, lpn, ic, zae)


@pytest.mark.parametrize("field,zae", [(0, True), (1, True), (0, False)])
def test_binary_tree_every_height(make, field, zae):
    bc.case_every_height(make(field, bc.B3 | (bc.ZAE if zae else 0)), field, 17, zae)


@pytest.mark.parametrize("field", [0, 1])
def test_merkle_prove(make, field):
    bc.case_merkle_prove(make(field, bc.ZAE | bc.B3), field)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("field,lpns", [(0, (6, 16)), (1, (6, 24))])
def test_message_length_edges(make, field, lpns, lazy):
    bc.case_length_edges(make, field, lpns, lazy)


TAIL = [("fused tail", bc.ZAE | bc.B3, {"MS_FRI_TAIL_MAX": "65536"}), ("launch per step", bc.ZAE | bc.B3, {"MS_FRI_TAIL_MAX": "0"}),
        ("latency", bc.ZAE | bc.B3 | bc.LATENCY, None)]


@pytest.mark.parametrize("field", [0, 1])
def test_whole_proof_2_16_rows(make, field):
    """L = 2^19: tree levels above the 16 384-parent subtree threshold, subtree launches and the fused tail all run"""
    bc.case_whole_proof(make, field, 16, 8, variants=TAIL)


def test_whole_proof_2_18_rows(make):
    bc.case_whole_proof(make, 0, 18, 8)


@pytest.mark.parametrize("field,steps,blowup", [(0, 255, 8), (1, 31, 4)])
def test_roundtrip_and_cross_rejection(make, field, steps, blowup):
    bc.case_roundtrip_and_cross_rejection(make, field, steps, blowup)


def test_shard_fails_closed(make):
    bc.case_shard_fails_closed(make)


def test_too_long_is_refused(make):
    bc.case_too_long_is_refused(make(0, bc.ZAE | bc.B3), 0)


def test_msh_hash(make):
    bc.case_msh_hash()
