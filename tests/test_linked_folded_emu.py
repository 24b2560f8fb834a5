"""Coset-grouped row trees (ms_lde_commit_coset, ms_lde_commit_stage_coset, ms_validity_commit_coset) and ms_query_linked_folded on the emulation build of the kernel
code (tests/emu, -DMS_EMU), against tests/pyref_linked_folded.py.  The same cases run on the HIP build in tests/test_linked_folded_gpu.py (-m gpu), which adds the
2^13-row shape."""
import json
import os
import subprocess

import numpy as np
import pytest

import mini_stark_amd as ms
import linked_folded_cases as lf
from mini_stark_amd.host import build_host_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")
SHA = lf.SHA


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


def test_sharded_context_refuses(make, monkeypatch):
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "16")
    lf.case_sharded(lf.ctx_of(make, SHA))


def test_sanitizer_fixture_is_current(make):
    """tests/golden/link_folded_tampered.bin, which the stand-alone sanitizer program reads (make -C tests/asan_link_folded run), is what the emulation build and the
    link verifier give today: the sections, the edits, and for every tampered copy the verdict and the step"""
    out, cases = lf.link_fixture_bytes(make)
    assert all(c[5] in (0, 1) for c in cases) and len(cases) > 900 and sum(1 for c in cases if c[5] == 0) > 800
    with open(os.path.join(HERE, "golden", "link_folded_tampered.bin"), "rb") as fh:
        assert fh.read() == out


def test_v3_sanitizer_fixture_is_current(make):
    """tests/golden/linked_v3_tampered.bin, which the stand-alone sanitizer program reads (make -C tests/asan_linked_v3 run), is what the drivers give today: the proof,
    the edits, and for every tampered copy the verdict and the step - one copy accepted, every other rejected"""
    out, cases = lf.v3_fixture_bytes(make)
    assert sum(1 for c in cases if c[4] == 1) == 1 and all(c[4] in (0, 1) for c in cases) and len(cases) > 400
    with open(os.path.join(HERE, "golden", "linked_v3_tampered.bin"), "rb") as fh:
        assert fh.read() == out


def test_linked_verdicts_are_the_recorded_ones(make):
    """tests/golden/linked_verdicts.json (tests/golden/gen_linked_verdicts.py) is what the drivers and verifiers of MSLP v1, v2 and v3 give today: per case the digest
    of the proof's bytes, and the whole (rc, why) for every tampered copy - v1 and v2 at N = 8, v3 at N = 16 for k = 1, 2, 3 with and without the permutation argument,
    both fields, 0 and 4 grinding bits, one v3 case per other digest.  The file was written by the three separate drivers the one driver replaced"""
    with open(os.path.join(HERE, "golden", "linked_verdicts.json")) as fh:
        text = fh.read()
    want, got = json.loads(text), lf.linked_verdicts(make)
    assert list(got["cases"]) == list(want["cases"]) and len(got["cases"]) == 36
    for name, case in got["cases"].items():
        rec = want["cases"][name]
        assert case["sha256"] == rec["sha256"], name
        assert [got["table"][i] for i in case["verdicts"]] == [want["table"][i] for i in rec["verdicts"]], name
        assert case.get("truncations") == rec.get("truncations"), name
        assert got["table"][case["verdicts"][0]] == [1, ""] and all(got["table"][i][0] in (0, 1) for i in case["verdicts"]), name   # the whole proof is accepted
    assert lf.linked_verdicts_text(got) == text                                           # ... and the file as a whole, byte for byte
