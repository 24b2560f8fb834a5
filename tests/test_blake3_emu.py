"""BLAKE3 as the context's digest (MS_FLAG_DIGEST_BLAKE3) on the emulation build of the kernel code (tests/emu, -DMS_EMU), against tests/pyref_blake3.py, which
this file also pins to tests/golden/blake3_kats.json.  The same cases run on the HIP build in tests/test_blake3_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import blake3_cases as bc
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


def test_flag_selects_blake3(make):
    bc.case_flag_selects_blake3(make)


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("leaf_num,ext,lpn,ic", bc.MERKLE_SHAPES)
def test_every_node(make, field, leaf_num, ext, lpn, ic, zae):
    bc.case_every_node(make(field, bc.B3 | (bc.ZAE if zae else 0)), field, leaf_num, ext, lpn, ic, zae)


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
def test_binary_tree_every_height(make, field, zae):
    bc.case_every_height(make(field, bc.B3 | (bc.ZAE if zae else 0)), field, 16, zae)


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
def test_whole_proof_against_pyprover(make, field):
    bc.case_whole_proof(make, field, 4, 2, against_pyprover=True)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n", [10, 14])
def test_whole_proof(make, field, log_n):
    bc.case_whole_proof(make, field, log_n, 8, variants=TAIL if log_n == 10 else TAIL[:1])


@pytest.mark.parametrize("field,steps,blowup", [(0, 63, 8), (1, 31, 4)])
def test_roundtrip_and_cross_rejection(make, field, steps, blowup):
    bc.case_roundtrip_and_cross_rejection(make, field, steps, blowup)


def test_shard_fails_closed(make):
    bc.case_shard_fails_closed(make)


@pytest.mark.parametrize("field", [0, 1])
def test_too_long_is_refused(make, field):
    bc.case_too_long_is_refused(make(field, bc.ZAE | bc.B3), field)


def test_msh_hash(make):
    bc.case_msh_hash()


def test_pyref_blake3_pinned_by_kats():
    bc.case_pyref_pinned()
