"""ms_mix_air_ext (build-defined: ms_mix_air with the combiner r in the extension field; include/ministark.h) on the emulation build of the kernel code (tests/emu,
-DMS_EMU): against the restatement of its definition (tests/pyref_air_ext.py), bit for bit against ms_mix_air for a base-field r, and by the defining formula at
out-of-domain points of the extension.  The same cases run on the HIP build in tests/test_air_ext_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import air_cases as ac
import air_ext_cases as xc
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def make():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    build_host_library()

    def mk(field, fresh=True):
        return ms.Context(field, lib_path=EMU)
    return mk


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", ac.DEFINITION_ROWS)
def test_definition(make, field, name, blowup):
    xc.case_definition(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["mimc", "selector"])
@pytest.mark.parametrize("log_n,blowup", [(4, 8), (10, 4), (11, 8)])
def test_base_field_r_reproduces_mix_air(make, field, name, log_n, blowup):
    """N = 16, blowup 8: L = 128, the tail of one workgroup, and the whole FRI down to the MSFP bytes; N = 2^10, blowup 4: two workgroups and the row-offset wrap;
    N = 2^11, blowup 8: several workgroups"""
    xc.case_base_r(make, field, name, log_n, blowup, full_fri=log_n == 4)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", ["mimc", "fib_bounded"])
@pytest.mark.parametrize("log_n,blowup", [(10, 4), (11, 8)])
def test_definition_at_extension_points(make, field, name, log_n, blowup):
    xc.case_identity(make, field, name, log_n, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name,blowup", [("mimc", 4), ("fib_bounded", 2)])
def test_deep_ali_host_function_and_fri(make, field, name, blowup):
    xc.case_deep_and_fri(make, field, name, blowup)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals_arg_and_state(make, field):
    xc.case_refusals(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_context_refused(make, monkeypatch, field):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    xc.case_sharded_refused(lambda f: ms.Context(f, lib_path=EMU), field)


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_context_refused_below_the_sharding_threshold(make, monkeypatch, field):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    xc.case_sharded_refused(lambda f: ms.Context(f, lib_path=EMU), field)


@pytest.mark.parametrize("field", [0, 1])
def test_shape_refusal_leaves_the_context_usable(make, field):
    xc.case_shape_refusal_then_both(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_switching_between_the_stages(make, field):
    xc.case_switching(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_polynomial_store_grows(make, field):
    xc.case_store_growth(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_one_launch_and_shared_inverse_table(make, field):
    xc.case_one_launch(make, field)
