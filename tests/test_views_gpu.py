"""GPU suite (-m gpu): directed decimal corners through every view of the leaf-hash kernel (tests/view_cases.py) on libministark.so (HIP, gfx950), against the
oracle and the hashlib / numpy references - the cases of tests/test_views_emu.py, plus what only the GPU has: the wave-level slot allocation of the deferred-block
lists under full load, the grid-stride loop of PadOnlyBlockKernel at 2^19 groups, a page-locked trace source and the one-rank RCCL world."""
import os

import numpy as np
import pytest

import mini_stark_amd as ms
import view_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    cache = {}

    def mk(field, flags, env=None, fresh=False):
        if env is None and not fresh:
            if (field, flags) not in cache:
                cache[field, flags] = ms.Context(field, flags=flags)   # raises if the HIP library / GPU is unavailable: no fallback
            return cache[field, flags]
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            return ms.Context(field, flags=flags)   # the MS_* variables are read by ms_create
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return mk


def _set_env(monkeypatch):
    def set_env(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    return set_env


@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
def test_trace_view(make, field, zae):
    ctx = make(field, vc.flags(vc.SHA, zae))
    for log_n, w, lpns in vc.TRACE_SHAPES:
        vc.case_trace_view(ctx, vc.SHA, field, log_n, w, lpns, zae)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,w,lpns,lazy_min", vc.FORCED_KERNEL)
def test_trace_view_other_leaf_kernel(make, field, log_n, w, lpns, lazy_min):
    ctx = make(field, vc.ZAE, env={"MS_LEAF_LAZY_MIN": lazy_min})
    vc.case_trace_view(ctx, vc.SHA, field, log_n, w, lpns, True)
    ctx.close()


@pytest.mark.parametrize("digest", vc.OTHER_DIGESTS)
@pytest.mark.parametrize("field", [0, 1])
def test_trace_view_other_digests(make, digest, field):
    ctx = make(field, vc.flags(digest))
    for log_n, w, lpns in vc.OTHER_DIGEST_TRACE_SHAPES:
        vc.case_trace_view(ctx, digest, field, log_n, w, lpns, True)


@pytest.mark.parametrize("field", [0, 1])
def test_trace_view_device_pointer_montgomery_and_page_locked_input(make, field):
    import torch

    def to_device(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        return t.data_ptr(), t
    vc.case_trace_entries(make, field, to_device, pinned=True)


@pytest.mark.parametrize("virtual", ["1", "0"])
@pytest.mark.parametrize("blowup", [1, 4])
@pytest.mark.parametrize("zae", [True, False])
@pytest.mark.parametrize("field", [0, 1])
def test_lde_view_directed_on_the_coset(make, field, zae, blowup, virtual):
    vc.case_lde_view(make, field, zae, blowup, virtual)


@pytest.mark.parametrize("digest", vc.OTHER_DIGESTS)
@pytest.mark.parametrize("field", [0, 1])
def test_lde_view_other_digests(make, digest, field):
    for blowup in (1, 4):
        vc.case_lde_view_other_digest(make, digest, field, blowup)


@pytest.mark.parametrize("tail_max", ["0", None])
@pytest.mark.parametrize("field", [0, 1])
def test_fri_round0_codeword_view(make, field, tail_max):
    vc.case_fri_view(make, field, tail_max)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_groups,defer", [(16, True), (17, True), (19, True), (16, False)])
def test_pad_only_lists_at_capacity(make, field, log_groups, defer):
    vc.case_pad_lists(make(field, vc.ZAE), field, log_groups, defer)


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_views_on_one_rank(monkeypatch, field):
    import torch
    vc.case_sharded_views(lambda f: ms.Context(f), _set_env(monkeypatch), field, device=torch.device("cuda", 0))


@pytest.mark.parametrize("field", [0, 1])
def test_sharded_views_on_one_rank_rccl(monkeypatch, field):
    """the exchanges as RCCL calls inside the library on a one-rank communicator - where the library's RCCL self-test succeeds"""
    import torch
    probe = ms.Context(field)
    rc, why = probe.L.ms_rccl_selftest(probe.h), probe.last_error()
    probe.close()
    if rc != 0:
        pytest.skip(f"ms_rccl_selftest: {why}")
    vc.case_sharded_views(lambda f: ms.Context(f), _set_env(monkeypatch), field, rccl=True, device=torch.device("cuda", 0))
