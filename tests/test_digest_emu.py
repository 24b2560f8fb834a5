"""BLAKE2s-256 as the context's digest (MS_FLAG_DIGEST_BLAKE2S) on the emulation build of the kernel code (tests/emu, -DMS_EMU), against hashlib.
The same cases run on the HIP build in tests/test_digest_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import digest_cases as dc
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


def test_flag_selects_blake2s(make):
    dc.case_flag_selects_blake2s(make)


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("leaf_num,ext,lpn,ic", dc.MERKLE_SHAPES)
def test_every_node(make, field, leaf_num, ext, lpn, ic, zae):
    dc.case_every_node(make(field, dc.B2 | (dc.ZAE if zae else 0)), field, leaf_num, ext, lpn, ic, zae)


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
def test_binary_tree_every_height(make, field, zae):
    dc.case_every_height(make(field, dc.B2 | (dc.ZAE if zae else 0)), field, 16, zae)


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
def test_whole_proof_against_pyprover(make, field):
    dc.case_whole_proof(make, field, 4, 2, against_pyprover=True)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n", [10, 14])
def test_whole_proof(make, field, log_n):
    dc.case_whole_proof(make, field, log_n, 8, variants=TAIL if log_n == 10 else TAIL[:1])


@pytest.mark.parametrize("field,steps,blowup", [(0, 63, 8), (1, 31, 4)])
def test_roundtrip_and_cross_rejection(make, field, steps, blowup):
    dc.case_roundtrip_and_cross_rejection(make, field, steps, blowup)


def test_shard_fails_closed(make):
    dc.case_shard_fails_closed(make)
