"""Keccak-256 and SHA3-256 as the context's digest (MS_FLAG_DIGEST_KECCAK256 / MS_FLAG_DIGEST_SHA3_256) on the emulation build of the kernel code (tests/emu,
-DMS_EMU), against hashlib.sha3_256 and tests/pyref_keccak.py, which this file also pins.  The same cases run on the HIP build in tests/test_keccak_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import keccak_cases as kc
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


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


def test_pyref_keccak_pinned():
    kc.case_pyref_pinned()


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
    kc.case_every_height(make(field, kc.FLAG[d] | (kc.ZAE if zae else 0)), d, field, 10, zae)


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
@pytest.mark.parametrize("log_n", [6, 8])
def test_whole_proof_keccak256(make, field, log_n):
    kc.case_whole_proof(make, 4, field, log_n, 8, variants=kc.tail_variants(4))


def test_whole_proof_sha3_256(make):
    kc.case_whole_proof(make, 5, 0, 7, 8)


@pytest.mark.parametrize("field,steps,blowup", [(0, 255, 8), (1, 31, 4)])
def test_roundtrip_and_cross_rejection(make, field, steps, blowup):
    kc.case_roundtrip_and_cross_rejection(make, field, steps, blowup)


@pytest.mark.parametrize("d", kc.DIGESTS)
def test_shard_fails_closed(make, d):
    kc.case_shard_fails_closed(make, d)


def test_msh_hash(make):
    kc.case_msh_hash()
