"""GPU suite (-m gpu): the coset-grouped row trees and ms_query_linked_folded on libministark.so (HIP, gfx950) - the cases of tests/test_linked_folded_emu.py (all but
the sharded context, which runs on the emulation build only) and the 2^13-row shape (L = 2^16: 32 leaf workgroups at arity 8)."""
import os

import numpy as np
import pytest

import mini_stark_amd as ms
import linked_folded_cases as lf
from mini_stark_amd.host import build_host_library

pytestmark = pytest.mark.gpu
SHA = lf.SHA


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


# ---- 1. + 2. trees and openings
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("d", lf.DIGESTS)
def test_trees_with_staged_columns(make, d, k, field):
    """N = 64, L = 512: the three trees of a statement with one permutation argument (c0 = 6, c1 = E, m = E chunk columns - Fp4 on BabyBear)"""
    lf.case_trees(make, d, field, k, "permutation")


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k,w", [(1, 2), (2, 2), (3, 6), (3, 1), (1, 9)])
def test_lde_tree_message_lengths(make, k, w, field):
    """4 elements at k = 1, w = 2 (the short form), 48 at k = 3, w = 6 (the two-block form); 8 and 18 around the threshold of 16"""
    lf.case_trees_lde_only(make, SHA, field, k, w)


def test_lde_tree_blake3_multi_chunk(make):
    """w = 7 at k = 3 under BLAKE3 on Goldilocks: 56 elements, a message above 1024 bytes"""
    lf.case_trees_lde_only(make, lf.ro.BLAKE3, 0, 3, 7)


def test_blake3_message_above_16_kib_is_refused(make):
    """824 elements of up to 20 digits: refused before anything changes - the plain tree committed before still opens its rows"""
    ctx = lf.ctx_of(make, lf.ro.BLAKE3, 0)
    assert ctx.trace_commit(np.ones((8, 103), dtype=np.uint64), 103)[0] == 0 and ctx.interpolate() == 0
    rc, root = ctx.lde_commit(2, 3, 103)
    assert rc == 0
    rows, lde = ctx.tree_open(ms.TREE_LDE, [0, 15, 7]), ctx.lde_read().tobytes()
    assert lf.raw_commit(ctx, "lde", 3, 2, 3) == ms.ERR_ARG and "BLAKE3" in ctx.last_error()
    assert ctx.tree_open(ms.TREE_LDE, [0, 15, 7]) == rows and ctx.lde_read().tobytes() == lde
    assert ctx.lde_commit_coset(2, 3, 1)[0] == 0 and len(ctx.tree_open(ms.TREE_LDE, [7])) != len(rows) // 3   # 206 elements per leaf: committed, and opened by leaf group


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_trees_at_2_11_rows(make, k, field):
    lf.case_trees(make, SHA, field, k, "permutation", N=1 << 11)


# ---- 3. ms_query_linked_folded
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["fib", "permutation", "lowdeg"])
def test_query_equals_its_definition(make, name, k, field):
    lf.case_definition(make, SHA, field, k, name)


@pytest.mark.parametrize("d", lf.DIGESTS[1:])
def test_query_other_digests(make, d):
    lf.case_definition(make, d, 0, 2, "permutation")


@pytest.mark.parametrize("field", [0, 1])
def test_query_at_2_11_rows(make, field):
    lf.case_definition(make, SHA, field, 3, "logup", N=1 << 11)


@pytest.mark.parametrize("field", [0, 1])
def test_query_latency_context(make, field):
    lf.case_definition(make, SHA, field, 2, "permutation", extra=lf.LATENCY)


# ---- 4. the link verifier
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["fib", "permutation", "lowdeg"])
def test_link_accepts_and_names_every_tampering(make, name, k, field):
    lf.case_link(make, SHA, field, k, name)


@pytest.mark.parametrize("d", lf.DIGESTS[1:])
def test_link_other_digests(make, d):
    lf.case_link(make, d, 0, 2, "permutation")


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_link_refuses_another_proofs_msff(make, k, field):
    lf.case_splice(make, SHA, field, k)


# ---- 5. MSLP v3 and the drivers
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("which", [None, "permutation"])
@pytest.mark.parametrize("gb", [0, 4])
def test_v3_c_and_python_drivers_same_bytes(make, gb, which, k, field):
    lf.case_v3_end_to_end(make, SHA, field, which, k, gb=gb)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("which", [None, "permutation"])
@pytest.mark.parametrize("gb", [0, 4])
def test_v3_rejections_name_the_step(make, gb, which, k, field):
    lf.case_v3_rejections(make, SHA, field, which, k, gb=gb)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("which", [None, "permutation"])
def test_v3_false_trace_leaves_an_empty_slot(make, which, field):
    lf.case_v3_false_trace(make, SHA, field, which, 2)


# ---- 6. refusals and state
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_refusals_and_state(make, k, field):
    lf.case_refusals(make, SHA, field, k)


def test_virtual_columns_are_refused(make):
    lf.case_virtual_columns(make, SHA)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_trees_and_query_at_2_13_rows(make, k, field):
    """L = 2^16: 32 leaf workgroups at k = 3; the trees under SHA-256, then the whole flow and the blob"""
    lf.case_trees(make, SHA, field, k, "permutation", N=1 << 13)
    lf.case_definition(make, SHA, field, k, "permutation", N=1 << 13)
