"""Directed decimal corners through every view of the leaf-hash kernel (tests/view_cases.py) on the emulation build of the kernel code (tests/emu, -DMS_EMU),
against the oracle and the hashlib / numpy references.  The same cases run on the HIP build in tests/test_views_gpu.py (-m gpu)."""
import os
import subprocess

import pytest

import mini_stark_amd as ms
import view_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libministark_emu.so")


@pytest.fixture(scope="module")
def make():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    cache = {}

    def mk(field, flags, env=None, fresh=False):
        if env is None and not fresh:
            if (field, flags) not in cache:
                cache[field, flags] = ms.Context(field, flags=flags, lib_path=EMU)
            return cache[field, flags]
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


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,w,lpns", vc.TRACE_SHAPES)
def test_trace_view(make, field, log_n, w, lpns, zae):
    vc.case_trace_view(make(field, vc.flags(vc.SHA, zae)), vc.SHA, field, log_n, w, lpns, zae)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,w,lpns,lazy_min", vc.FORCED_KERNEL)
def test_trace_view_other_leaf_kernel(make, field, log_n, w, lpns, lazy_min):
    ctx = make(field, vc.ZAE, env={"MS_LEAF_LAZY_MIN": lazy_min})
    vc.case_trace_view(ctx, vc.SHA, field, log_n, w, lpns, True)
    ctx.close()


@pytest.mark.parametrize("digest", vc.OTHER_DIGESTS)
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,w,lpns", vc.OTHER_DIGEST_TRACE_SHAPES)
def test_trace_view_other_digests(make, digest, field, log_n, w, lpns):
    vc.case_trace_view(make(field, vc.flags(digest)), digest, field, log_n, w, lpns, True)


@pytest.mark.parametrize("field", [0, 1])
def test_trace_view_device_pointer_and_montgomery_input(make, field):
    """(in the emulation build a device pointer is a host pointer; the page-locked source runs on the GPU)"""
    vc.case_trace_entries(make, field, lambda a: (a.ctypes.data, a), pinned=False)


@pytest.mark.parametrize("virtual", ["1", "0"])
@pytest.mark.parametrize("blowup", [1, 4])
@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
def test_lde_view_directed_on_the_coset(make, field, zae, blowup, virtual):
    vc.case_lde_view(make, field, zae, blowup, virtual)


@pytest.mark.parametrize("digest", vc.OTHER_DIGESTS)
@pytest.mark.parametrize("blowup", [1, 4])
@pytest.mark.parametrize("field", [0, 1])
def test_lde_view_other_digests(make, digest, field, blowup):
    vc.case_lde_view_other_digest(make, digest, field, blowup)


@pytest.mark.parametrize("tail_max", ["0", None])
@pytest.mark.parametrize("field", [0, 1])
def test_fri_round0_codeword_view(make, field, tail_max):
    vc.case_fri_view(make, field, tail_max)


@pytest.mark.parametrize("field,log_groups,defer", [(0, 16, True), (1, 16, True), (0, 17, True), (1, 17, True), (0, 16, False), (1, 16, False), (0, 19, True)])
def test_pad_only_lists_at_capacity(make, field, log_groups, defer):
    """(2^19 groups - the grid-stride loop of PadOnlyBlockKernel - on Goldilocks only here, thread by thread; both fields on the GPU)"""
    vc.case_pad_lists(make(field, vc.ZAE), field, log_groups, defer)


@pytest.mark.parametrize("world,field,env", [(2, 0, {}), (4, 1, {"MS_SHARD_SLICES": "2", "MS_SHARD_SLICE_MIN": "2"})])
def test_sharded_views_on_several_ranks(world, field, env):
    """On one rank every run starts at group 0 and the output offset of the contiguous raw-trace tree (out_g0 = rank * groups per rank) is 0: the directed matrix once
    more over gloo ranks (tests/shard_worker.py compares every rank's stage outputs with the oracle), where ranks above 0 hash from an offset into slot 0."""
    from test_shard_gloo import run_world
    res = run_world(world, field, vc.SHARD_LOG_N, vc.SHARD_BLOWUP, 16, 0, env=env, mode="directed")
    assert res["world"] == world and res["dist_rounds"] >= 2
    assert (res["slices"] > 0) == bool(env), res


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_views_on_one_rank(monkeypatch, make, field):
    def set_env(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    vc.case_sharded_views(lambda f: ms.Context(f, lib_path=EMU), set_env, field)
