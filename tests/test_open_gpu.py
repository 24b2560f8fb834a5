"""GPU suite (-m gpu): ms_tree_open / ms_fri_query_index and their verifying side on libministark.so (HIP, gfx950) - the cases of tests/test_open_emu.py
(all but the sharded context, which runs on the emulation build only)."""
import os

import pytest

import mini_stark_amd as ms
import open_cases as oc
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu
SHA = oc.ro.SHA256


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
@pytest.mark.parametrize("d", oc.DIGESTS)
def test_tree_heights(make, d, field):
    oc.case_tree_heights(make, d, field)


def test_tree_heights_latency_context(make):
    oc.case_tree_heights(make, SHA, 0, extra=oc.LATENCY)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("d", oc.DIGESTS)
def test_trace_tree(make, d, field):
    oc.case_trace_tree(make, d, field)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 65])
def test_lde_rows(make, c, field):
    oc.case_lde_rows(make, SHA, field, c)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("env,virtual", [({"MS_LDE_VIRTUAL": "1"}, True), ({"MS_LAZY_LINCOMB": "0"}, None), ({"MS_LDE_VIRTUAL": "0"}, False)], ids=["virtual", "not_lazy", "written"])
def test_lde_rows_lincomb_forms(make, env, virtual, field):
    oc.case_lde_rows(make, SHA, field, 3, env=env, virtual=virtual)
    oc.case_lde_rows(make, SHA, field, 65, env=env, virtual=virtual)


@pytest.mark.parametrize("d", oc.DIGESTS[1:])
def test_lde_rows_other_digests(make, d):
    oc.case_lde_rows(make, d, 0, 65)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("d", oc.DIGESTS)
def test_fri_round_trees(make, d, field):
    oc.case_fri_rounds(make, d, field)


def test_fri_round_trees_latency_context(make):
    oc.case_fri_rounds(make, SHA, 0, extra=oc.LATENCY)


@pytest.mark.parametrize("field", [0, 1])
def test_refusals(make, field):
    oc.case_refusals(make, SHA, field)


@pytest.mark.parametrize("d,field,extra", [(SHA, 0, 0), (SHA, 1, 0), (SHA, 0, oc.LATENCY), (oc.ro.BLAKE3, 0, 0), (oc.ro.KECCAK256, 1, 0)])
def test_context_unchanged(make, d, field, extra):
    oc.case_context_unchanged(make, d, field, extra)


@pytest.mark.parametrize("tail", [True, False], ids=["tail", "no_tail"])
@pytest.mark.parametrize("blowup", [2, 8])
@pytest.mark.parametrize("N", [8, 64, 1 << 10])
@pytest.mark.parametrize("field", [0, 1])
def test_query_index(make, field, N, blowup, tail):
    oc.case_query_index(make, SHA, field, N, blowup, tail)


@pytest.mark.parametrize("d", oc.DIGESTS[1:])
def test_query_index_other_digests(make, d):
    oc.case_query_index(make, d, 0, 64, 8, True, all_rounds=False)


def test_query_index_latency_context(make):
    oc.case_query_index(make, SHA, 0, 64, 8, True, extra=oc.LATENCY)


@pytest.mark.parametrize("field", [0, 1])
def test_query_index_against_pyprover(make, field):
    oc.case_pyprover(make, field)


@pytest.mark.parametrize("field", [0, 1])
def test_agreement_with_by_value_phase(make, field):
    oc.case_agreement_with_by_value(make, SHA, field)


@pytest.mark.parametrize("field", [0, 1])
def test_constant_trace_where_by_value_opens_position_0(make, field):
    oc.case_constant_trace(make, SHA, field)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("d", oc.DIGESTS)
def test_tampering(make, d, field):
    oc.case_tampering(make, d, field)


@pytest.mark.parametrize("field", [0, 1])
def test_launch_count(make, field):
    oc.case_launch_count(make, SHA, field)


@pytest.mark.parametrize("field", [0, 1])
def test_order_and_repetition(make, field):
    oc.case_order_and_repetition(make, SHA, field)
