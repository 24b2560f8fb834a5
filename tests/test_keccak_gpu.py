"""GPU suite (-m gpu): Keccak-256 and SHA3-256 as the context's digest on libministark.so (HIP, gfx950), against hashlib.sha3_256 and tests/pyref_keccak.py - the
cases of tests/test_keccak_emu.py at the sizes where every launch shape runs (levels above the subtree threshold, subtree launches, the fused FRI tail)."""
import os

import pytest

import mini_stark_amd as ms
import keccak_cases as kc
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


def test_flag_selects(make):
    kc.case_flag_selects(make)


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("d", kc.DIGESTS)
def test_every_node(make, d, field, zae):
    ctx = make(field, kc.FLAG[d] | (kc.ZAE if zae else 0))
    for leaf_num, ext, lpn, ic in kc.MERKLE_SHAPES:
        kc.case_every_node(ctx, d, field, leaf_num, ext, lpn, ic, zae)


@pytest.mark.parametrize("field,zae", [(0, True), (1, True), (0, False)])
@pytest.mark.parametrize("d", kc.DIGESTS)
def test_binary_tree_every_height(make, d, field, zae):
    """2^1 ... 2^17 leaf groups: across the 16 384-parent subtree threshold and the nine-level launches"""
    kc.case_every_height(make(field, kc.FLAG[d] | (kc.ZAE if zae else 0)), d, field, 17, zae)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("d", kc.DIGESTS)
def test_merkle_prove(make, d, field):
    kc.case_merkle_prove(make(field, kc.ZAE | kc.FLAG[d]), d, field)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("field,lpns", [(0, (6, 16)), (1, (6, 28))])
@pytest.mark.parametrize("d", kc.DIGESTS)
def test_message_length_edges(make, d, field, lpns, lazy):
    kc.case_length_edges(make, d, field, lpns, lazy)


@pytest.mark.parametrize("field", [0, 1])
def test_whole_proof_2_16_rows_keccak256(make, field):
    """L = 2^19: tree levels above the 16 384-parent subtree threshold, subtree launches and the fused tail all run; BabyBear's FRI leaf group (two Fp4 elements,
    about 200 bytes) is the two-block message of the fused round"""
    kc.case_whole_proof(make, 4, field, 16, 8, variants=kc.tail_variants(4))


def test_whole_proof_2_16_rows_sha3_256(make):
    kc.case_whole_proof(make, 5, 0, 16, 8)


@pytest.mark.parametrize("field,steps,blowup", [(0, 255, 8), (1, 31, 4)])
def test_roundtrip_and_cross_rejection(make, field, steps, blowup):
    kc.case_roundtrip_and_cross_rejection(make, field, steps, blowup)


@pytest.mark.parametrize("d", kc.DIGESTS)
def test_shard_fails_closed(make, d):
    kc.case_shard_fails_closed(make, d)


def test_msh_hash(make):
    kc.case_msh_hash()
