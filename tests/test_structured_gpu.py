"""GPU suite (-m gpu): low-degree, sparse and zero validity polynomials and edge-of-field challenges (tests/structured_cases.py) on libministark.so (HIP, gfx950)
against the oracle, every stage's status and value bit for bit - the cases of tests/test_structured_emu.py on the real atomics, the fused tail's completion counter
and self-clearing length word, the polled flag of MS_FLAG_LATENCY and the length word riding on the tree's last launch, at the sizes where each launch shape runs."""
import os

import pytest

import mini_stark_amd as ms
import parity_cases as pc
import structured_cases as sc

pytestmark = pytest.mark.gpu

# ms_create reads the MS_* variables: (name, flags, environment) of the contexts the reduced list runs on besides the default one
VARIANTS = [("launch per step", 0, {"MS_FRI_TAIL_MAX": "0"}),
            ("latency flag", ms.FLAG_LATENCY, {}),
            ("8-wide fold, 16-coefficient evaluation", 0, {"MS_FOLD_SMALL_MAX": "0", "MS_EVAL_SMALL_MAX": "0"}),
            ("transform instead of the pointwise codeword", 0, {"MS_FRI_POINTWISE": "0"}),
            ("one launch per tree level", 0, {"MS_TREE_SUBTREE_PARENTS": "0"})]


@pytest.fixture(scope="module")
def mk():
    assert os.path.exists(ms.library_path()), "libministark.so missing: run __graft_entry__.build()"
    cache = {}

    def make(field, fresh=False):
        if fresh:
            return ms.Context(field)
        if field not in cache:
            cache[field] = ms.Context(field)  # raises if the HIP library / GPU is unavailable: no fallback
        return cache[field]
    return make


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("name", sc.names_for(64))
@pytest.mark.parametrize("field", [0, 1])
def test_structured_2p6_rows(mk, field, name, mode):
    """every support x every challenge mode with all read-backs, then a Fibonacci proof: structured and generic proofs alternate on the module's context"""
    sc.case_structured(mk(field), field, 6, name, mode)
    sc.case_generic(mk(field), field, 6)


@pytest.mark.parametrize("name", sc.names_for(2048))
@pytest.mark.parametrize("field", [0, 1])
def test_structured_2p11_rows_fused_tail(mk, field, name):
    """D0 <= 2^14: every folded round qualifies for the fused tail (m <= 2048 coefficients, D <= 2^15) - one launch that trims, sizes, folds and hashes"""
    ctx = mk(field)
    n = sc.fri_tail_launches(ctx, lambda: [sc.case_structured(ctx, field, 11, name, mode, read_big=False) for mode in sc.MODES])
    assert n > 0


@pytest.mark.parametrize("variant", range(len(VARIANTS)), ids=[v[0].split(",")[0].replace(" ", "_") for v in VARIANTS])
@pytest.mark.parametrize("field", [0, 1])
def test_structured_2p11_rows_variants(monkeypatch, field, variant):
    _, flags, env = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = ms.Context(field, flags=ms.FLAG_ZERO_DISPLAY_EMPTY | flags)
    try:
        n = sc.fri_tail_launches(ctx, lambda: [sc.case_structured(ctx, field, 11, name, mode, read_big=False) for name, mode in sc.REDUCED])
        if env.get("MS_FRI_TAIL_MAX") == "0":
            assert n == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("name,mode", sc.LARGE)
@pytest.mark.parametrize("field", [0, 1])
def test_structured_2p14_rows(mk, field, name, mode):
    """D0 = 2^17: the smallest size with a find-first launch of its own (D > 2^16), tree levels above the 16384-parent subtree threshold, a multi-block degree
    kernel and a multi-level suffix scan (8192 folded coefficients)"""
    sc.case_structured(mk(field), field, 14, name, mode, read_big=False)


@pytest.mark.parametrize("field", [0, 1])
def test_config_rounds_on_low_degree_trace_then_generic_proof(mk, field):
    sc.case_config_rounds_then_generic(mk(field), field)


@pytest.mark.parametrize("log_n", [6, 11])
@pytest.mark.parametrize("field", [0, 1])
def test_edge_challenges(mk, field, log_n):
    sc.case_edge_challenges(mk, field, log_n, read_big=(log_n == 6))


def test_sharded_code_paths_on_one_rank_even_trace(monkeypatch):
    """The one-rank RCCL world (parity_cases.case_sharded_paths_on_one_rank) on a trace whose polynomials are even in x: every query opens two equal values, and the
    sharded lookup by value (a MIN over the ranks' first matches) must name the first of them"""
    import torch
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "64")
    trace = sc.trace_of(0, 12, "even")
    st, dist_rounds = pc.case_sharded_paths_on_one_rank(lambda f: ms.Context(f), 0, 12, 8, rccl=True, device=torch.device("cuda", 0), trace=trace)
    assert st[0] >= 3 and st[1] > st[0] and st[2] == 1 and st[3] == 1 and dist_rounds >= 2
