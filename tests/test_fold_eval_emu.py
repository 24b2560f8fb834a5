"""The throughput form of the FRI evaluation-domain fold (csrc/poly.hpp FriFoldWgKernel) on the emulation build of the kernel code (tests/emu, -DMS_EMU: the
cooperative kernel runs on fibers, barriers included), against the library's own transform path (MS_FRI_POINTWISE=0) and tests/pyref.py.  Cases: tests/fold_eval_cases.py;
the same cases run on the HIP build in tests/test_fold_eval_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import fold_eval_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def plain():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    return lambda field: ms.Context(field, lib_path=EMU)


@pytest.fixture(scope="module")
def make(plain):
    return fc.env_ctx(plain)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup,D0", fc.SIZES)
def test_rounds_match_transform(make, field, log_n, blowup, D0):
    fc.case_matches_transform(make, field, fc.setup_fibonacci(field, log_n, blowup), blowup, expect_D0=D0)


@pytest.mark.parametrize("field", [0, 1])
def test_cubic_validity_polynomial(make, field):
    fc.case_matches_transform(make, field, fc.setup_cubic(field, 4, 4, 8), 8, expect_D0=256, expect_odd_len=True)


@pytest.mark.parametrize("field", [0, 1])
def test_base_field_deep_point_takes_the_transform(make, field):
    fc.case_matches_transform(make, field, fc.setup_fibonacci(field, 6, 8), 8, base_z=(1, 3), expect_D0=512)


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_index_map_on_one_rank(make, field, monkeypatch):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_STUB", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    got = fc.case_matches_transform(make, field, fc.setup_fibonacci(field, 7, 8), 8, expect_D0=1024, shard=lambda ctx: fc.PinnedShard(ctx, 32 * 128 * 8 + (4 << 20)))
    assert got[1][5] is None and got[2][5] is None and got[-1][5] is not None     # sharded rounds first (roots only), replicated ones behind them


def test_first_fold_against_pyref(make):
    fc.case_one_round_vs_pyref(make)


def test_shift_multiplications(plain):
    fc.case_shift_multiplications(plain)
