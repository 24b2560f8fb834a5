"""GPU suite (-m gpu): libministark.so (hand-written HIP, gfx950) through the
C ABI against the CPU oracle, bit-exact, on the same seeded inputs; plus
size-independent properties at BASELINE.json's full sizes."""
import hashlib
import os

import numpy as np
import pytest

import mini_stark_amd as ms
import parity_cases as pc
from common import MODULUS, EXT, SplitMix64, fibonacci_trace_fast, fibonacci_closures
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 7, 9, 10, 11, 13, 16, 19, 20, 21])
def test_ntt(mk, field, log_n):
    pc.case_ntt(mk, field, log_n, batch=2 if log_n < 19 else 1)


@pytest.mark.parametrize("log_n", [14, 15, 16, 18, 19, 21])
def test_coset_lde_tile_shapes(mk, log_n):
    """Blowup-8 Goldilocks LDEs whose plans walk every tile shape of the cooperative passes behind the virtual pass
    (2^7 x 2^7, 2^8 x 2^7, 2^8 x 2^8, 2^9 x 2^9, 2^10 x 2^9) and the register-only last pass (2^10 x 2^10 x 2)."""
    pc.case_coset_lde(mk, 0, log_n, 8)


@pytest.mark.parametrize("field,log_n", [(0, 23), (0, 24), (1, 23)])
def test_ntt_large_vs_oracle(mk, field, log_n):
    pc.case_ntt(mk, field, log_n, batch=1)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup", [(3, 2), (4, 8), (9, 4), (12, 8), (17, 8)])
def test_coset_lde(mk, field, log_n, blowup):
    pc.case_coset_lde(mk, field, log_n, blowup)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("leaf_num,ext,lpn,ic", [(16, 1, 2, 2), (16, 1, 4, 2), (16, 1, 4, 4), (16, 1, 16, 16), (2, 1, 2, 2), (3, 1, 2, 2),
                                                 (4096, 1, 2, 2), (6144, 1, 6, 2), (24, 1, 6, 2), (1 << 13, 0, 2, 2), (64, 0, 2, 2),
                                                 (3 << 18, 1, 6, 2), (1 << 19, 0, 2, 2), (1 << 14, 1, 128, 2)])
def test_merkle(mk, field, leaf_num, ext, lpn, ic):
    pc.case_merkle(mk, field, leaf_num, ext or EXT[field], lpn, ic, special=True)


@pytest.mark.parametrize("field", [0, 1])
def test_merkle_binary_tree_every_height(mk, field):
    """r05: binary trees of 2 .. 2^20 leaf groups against the oracle - every height the subtree kernel can be handed, hence every width of the levels hashed by
    PAIRS of lanes (merkle.hpp Sha256Pair: bank-masked DPP adds under a partial EXEC mask, whole and partial groups of eight lanes) next to the one-lane-per-node levels."""
    for k in range(2, 22):
        pc.case_merkle(mk, field, 1 << k, 1, 2, 2)


@pytest.mark.parametrize("field", [0, 1])
def test_prove_base_field_deep_points(mk, field):
    pc.case_prove_base_field_deep_points(mk, field)


@pytest.mark.parametrize("field,lpn,ext", [(0, 6, 1), (0, 3, 1), (0, 2, 2), (0, 16, 1), (1, 6, 1), (1, 12, 1), (1, 2, 4), (1, 4, 4)])
def test_merkle_message_length_sweep(mk, field, lpn, ext):
    pc.case_merkle_length_sweep(mk, field, lpn, ext)


@pytest.mark.parametrize("field,log_n,blowup", [(0, 4, 2), (0, 3, 8), (0, 6, 8), (1, 3, 2), (1, 5, 4), (0, 10, 8), (1, 10, 8), (0, 13, 2)])
def test_prove(mk, field, log_n, blowup):
    pc.case_prove(mk, field, log_n, blowup)


@pytest.mark.parametrize("field,log_n", [(0, 16), (1, 16)])
def test_prove_2p16_vs_oracle(mk, field, log_n):
    pc.case_prove(mk, field, log_n, 8, read_big=False)


@pytest.mark.parametrize("field", [0, 1])
def test_error_codes(mk, field):
    pc.case_errors(mk, field)


@pytest.mark.parametrize("field", [0, 1])
def test_full_size_properties(mk, field):
    """BASELINE.json configs[1]/[2]: 2^20 rows, blowup 8.  Too big for the scalar oracle in
    seconds, so check size-independent properties: (1) LDE restricted to the trace coset
    reproduces nothing directly, so instead INTT(NTT(x)) == x on the 2^23 domain; (2) the
    proof is deterministic (same digest twice); (3) the FRI proof is accepted by the oracle's
    verifier restatement (fri.rs:191-245), Merkle paths checked against the GPU's own roots."""
    ctx = mk(field)
    p, e = MODULUS[field], EXT[field]
    x = pc.rand_field(field, (1, 1 << 23), seed=9)
    rc, y = ctx.ntt(x)
    assert rc == 0
    rc, z = ctx.ntt(y, inverse=True)
    assert rc == 0 and (z == x).all()
    # linearity spot check of the forward transform: NTT(x)[0] = sum(x)
    assert int(y[0, 0]) == int(np.sum(x[0].astype(object))) % p

    N, blowup = 1 << 20, 8
    trace = fibonacci_trace_fast(field, N)
    digests = []
    for rep in range(2):
        rng = SplitMix64(4242)
        assert ctx.trace_commit(trace, 6)[0] == 0
        assert ctx.interpolate() == 0
        for sc, idx in fibonacci_closures(field, N, orc.root_of_unity(field, N)):
            assert ctx.polys_lincomb(sc, idx) == 0
        rc, lde_root = ctx.lde_commit(blowup, rng.nonzero(p), 6)
        assert rc == 0
        assert ctx.mix(rng.field(p)) == 0
        rc, ev = ctx.eval_ext([rng.field(p) for _ in range(e)])
        assert rc == 0
        rounds = ctx.ceil_log2_k((N - 1) * blowup + 1)
        assert rounds == 23
        rc, root0 = ctx.fri_begin(blowup, rounds)
        assert rc == 0
        roots, zs, Bs, als = [root0], [], [], []
        for _ in range(1, rounds):
            zq = [rng.field(p) for _ in range(e)]
            rc, B = ctx.fri_deep(zq)
            assert rc == 0
            al = [rng.field(p) for _ in range(e)]
            rc, root = ctx.fri_fold_commit(al)
            assert rc == 0
            zs += zq; Bs += [int(v) for v in B]; als += al; roots.append(root)
        betas = [rng.next(), rng.next()]
        rc, proof = ctx.fri_query(betas)
        assert rc == 0
        h = hashlib.sha256(lde_root + b"".join(roots) + ev.tobytes() + proof).hexdigest()
        digests.append(h)
        if rep == 0:
            assert orc.fri_verify(field, e, rounds, betas, zs, Bs, als, b"".join(roots), proof) == 1
            bad = bytearray(proof); bad[8 * e + 3] ^= 0x40
            assert orc.fri_verify(field, e, rounds, betas, zs, Bs, als, b"".join(roots), bytes(bad)) == 0
    assert digests[0] == digests[1]


@pytest.mark.parametrize("field,steps,blowup", [(0, 9, 2), (1, 7, 2), (0, 1023, 8)])
def test_host_mirror_on_gpu(mk, field, steps, blowup):
    """C++ Stark::prove mirror == Python mirror on the HIP build (transcript, stage order, proof bytes)."""
    from mini_stark_amd.host import build_host_library
    import test_host_mirror as thm
    build_host_library()
    thm.check_pair(mk(field), steps, blowup)


@pytest.mark.parametrize("field,log_n", [(0, 20), (1, 20), (0, 22)])
def test_full_size_bit_exact_vs_oracle(mk, field, log_n):
    """BASELINE.json configs[1] and configs[2] at full size (2^20 rows, blowup 8, Goldilocks / BabyBear+Fp4) and a 2^22-row proof: every
    commitment, OOD value, FRI round and the serialised FRI proof (64-256 MiB) bit-exact against the CPU oracle (OpenMP over its
    independent loops, <= 16 threads).  The 2^24-row proof of configs[3] was checked the same way once (tools/fullsize_parity.py, 164 s)."""
    orc.set_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    try:
        pc.case_prove(mk, field, log_n, 8, nq_fri=0, read_big=False)
    finally:
        orc.set_threads(1)


def test_full_size_ood_values_verify(mk):
    """DEEP-ALI half of Stark::verify (src/starks.rs:204-225, oracle restatement) on a full-size GPU proof."""
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    for field in (0, 1):
        ctx = mk(field)
        steps = (1 << 20) - 1
        tt = fibonacci_air(ctx, steps)
        hs = HostStark(ctx, 20, 8, steps, tt.constrain_number())
        proof = hs.prove(tt, read_fri_proof=False)
        ch = [int(v) for v in hs.last_challenges]
        o = orc.Session(field)
        assert o.trace_commit(tt.data, tt.constrain_number()) == (0, proof.trace_commit)   # CPU hashes the 2^20 x 3 trace too
        assert o.interpolate() == 0
        for sc, idx in tt.transitions:
            assert o.polys_lincomb(sc, idx) == 0
        ev = np.concatenate([proof.constrain_queries, proof.validity_queries[:, None, :]], axis=1)
        assert o.verify_ood(ch[1], ch[2:2 + hs.constrain_queries * ctx.e], ev) == 1


@pytest.mark.parametrize("field", [0, 1])
def test_wide_air_shape(mk, field):
    pc.case_prove_wide(mk, field, log_n=10, w=64)


def test_wide_air_2p18_vs_oracle(mk):
    """BASELINE configs[4] shape (64 trace columns, c = 128) at 2^18 rows, bit-exact vs the oracle; the full 2^22-row instance was
    checked once with tools/fullsize_parity.py (167 s)."""
    orc.set_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    try:
        pc.case_prove_wide(mk, 0, log_n=18, w=64)
    finally:
        orc.set_threads(1)


@pytest.mark.parametrize("field", [0, 1])
def test_general_closure_path(mk, field):
    pc.case_general_closure(mk, field)


@pytest.mark.parametrize("field,ext,lpn,n", [(0, 1, 2, 64), (0, 1, 4, 64), (0, 2, 2, 32), (1, 4, 2, 16), (1, 1, 8, 4096)])
def test_merkle_prove_by_value(mk, field, ext, lpn, n):
    pc.case_merkle_prove(mk, field, n, ext, lpn)


@pytest.mark.parametrize("world,field,log_n,mode", [(2, 0, 12, "gpu"), (4, 1, 11, "gpu"), (2, 0, 16, "gpu"), (4, 0, 15, "gpu,root-only"), (2, 1, 13, "gpu,base-z"),
                                                   (2, 0, 12, "gpu,low-degree")])   # trace columns of degree N/2 + 2: half-empty coefficient ranges
def test_sharded_proof_on_gpu(world, field, log_n, mode):
    """ms_set_shard on the real HIP kernels: `world` ranks share this box's GPU (gloo, payloads staged through host
    memory), each proves its share of ONE proof; every rank checks all outputs against the oracle (tests/shard_worker.py)."""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(29950 + world), os.path.join(here, "shard_worker.py"), str(field), str(log_n), "8", "64", mode]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    calls = {int(k): v for k, v in res["calls"].items()}
    assert res["world"] == world and calls[0] >= 3 and calls[2] == 1 and calls[3] == 1
    assert res["dist_rounds"] >= 2 and calls[1] > calls[0]    # r04: the coefficient-domain work is partitioned too (distributed round polynomials; multi-level scans at 2^15+ rows)


@pytest.mark.parametrize("field,log_n", [(0, 10), (1, 9), (0, 20), (1, 18)])
def test_prove_then_verify_roundtrip_on_gpu(mk, field, log_n):
    """The reference's e2e flow (tests/e2e_goldilocks.rs:98-114) on the HIP build, up to BASELINE's full size: derive_constrains on
    the verifier's copy, Stark::prove on the GPU, Stark::verify with the product's CPU verifier; a flipped proof bit is rejected."""
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    ctx = mk(field)
    steps = (1 << log_n) - 1
    tt = fibonacci_air(ctx, steps)
    hs = HostStark(ctx, 20, 8, steps, tt.constrain_number())
    constrains = hs.derive_constrains(tt)
    proof = hs.prove(tt)
    assert hs.verify(constrains, proof), hs.last_verify_error
    blob = bytearray(proof.fri_proof.blob)
    blob[8 * ctx.e] ^= 1  # y1 of the first opening
    proof.fri_proof = type(proof.fri_proof)(bytes(blob), device_resident=False)
    assert not hs.verify(constrains, proof) and "linearity" in hs.last_verify_error


def test_sharded_full_size_matches_oracle():
    """BASELINE configs[1] size (2^20 rows, blowup 8) proved by 2 ranks sharing the GPU (default MS_SHARD_MIN_LEAVES: the LDE and the
    eight largest FRI rounds are sharded): every commitment, DEEP value and the 64 MiB FRI proof equal the CPU ORACLE's (each rank runs
    the oracle itself, OpenMP x8)."""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29961", os.path.join(here, "shard_worker.py"), "0", "20", "8", "32768", "gpu"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    calls = {int(k): v for k, v in res["calls"].items()}
    # 9 digest all-to-alls (LDE + the eight largest FRI rounds); r04: besides their 9 root all-gathers, the raw-trace tree's, the DEEP-ALI partial sums, two per distributed
    # round (DEEP partial sums, scan carries), the hand-over of the first replicated round polynomial, the query jobs' aggregates and the proof slices
    assert calls[0] == 9 and calls[1] >= 9 + 2 + 2 * 8 + 2 and calls[2] == 1 and calls[3] == 1 and res["dist_rounds"] == 8


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [7, 8, 9, 15, 16])
@pytest.mark.parametrize("linear", [0, 1])
def test_lincomb_many_terms(mk, field, k, linear):
    pc.case_lincomb_many_terms(lambda f: mk(f, fresh=True), field, k, linear)


@pytest.mark.parametrize("field", [0, 1])
def test_device_trace_range_check(mk, field):
    import torch

    def to_device(a):
        t = torch.from_numpy(a.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        return t.data_ptr(), t
    pc.case_device_trace_range_check(mk, field, to_device)


@pytest.mark.parametrize("field", [0, 1])
def test_device_trace_range_check_across_pool_wraps(mk, field):
    pc.case_device_trace_range_check_across_pool_wraps(mk, field)


@pytest.mark.parametrize("field,log_n", [(0, 10), (1, 10), (0, 16)])
def test_mont64_trace_input_on_gpu(mk, field, log_n):
    """MS_FLAG_TRACE_MONT64 on the HIP build (the flag INTEGRATION.md tells the Rust shim to use: arkworks keeps Fp as x * 2^64 mod p):
    a Montgomery-form trace, host and device-resident, gives the canonical trace's proof bit for bit."""
    import torch
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    p = MODULUS[field]
    steps = (1 << log_n) - 1
    ctx = mk(field)
    tt = fibonacci_air(ctx, steps)
    proof = HostStark(ctx, 20, 8, steps, tt.constrain_number()).prove(tt)
    mctx = ms.Context(field, flags=ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_TRACE_MONT64)
    mt = fibonacci_air(mctx, steps)
    R = (1 << 64) % p
    mt.data[:] = np.array([int(v) * R % p for v in tt.data.reshape(-1)], dtype=np.uint64).reshape(tt.data.shape)
    hs = HostStark(mctx, 20, 8, steps, mt.constrain_number())
    mp = hs.prove(mt)
    assert mp.arthur == proof.arthur and mp.fri_proof.blob == proof.fri_proof.blob and mp.trace_commit == proof.trace_commit
    d = torch.from_numpy(mt.data.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    mctx.check(hs.prove_raw(mt, trace_device_ptr=d.data_ptr(), read_fri_proof=True))
    dp = hs.last_proof(read_fri_proof=True)
    assert dp.arthur == proof.arthur and dp.fri_proof.blob == proof.fri_proof.blob and dp.constrain_trace_commit == proof.constrain_trace_commit
    mctx.close()


def _oracle_threads():
    return max(1, min(64, len(os.sched_getaffinity(0))))


def test_config3_2p24_rows_bit_exact_vs_oracle(mk):
    """BASELINE.json configs[3] at FULL size on one GPU: Fibonacci AIR, Goldilocks, 2^24 trace rows, blowup 8 (L = 2^27, 27 FRI rounds,
    ~25 GiB resident): every commitment, DEEP value, FRI round and the ~1 GiB serialised FRI proof bit-exact against the CPU oracle
    (OpenMP over its independent loops).  Minutes of host time."""
    import time
    orc.set_threads(_oracle_threads())
    t0 = time.time()
    try:
        pc.case_prove(mk, 0, 24, 8, nq_fri=0, read_big=False)
    finally:
        orc.set_threads(1)
    print(f"configs[3] 2^24 rows Goldilocks: bit-exact vs oracle in {time.time() - t0:.0f} s ({_oracle_threads()} oracle threads)")


def test_config4_wide_air_2p22_rows_bit_exact_vs_oracle(mk):
    """BASELINE.json configs[4] at FULL size on one GPU: wide AIR, 64 trace columns + 64 transition polynomials (c = 128), Goldilocks,
    2^22 rows, blowup 8 (32 GiB LDE matrix, 2.5 KB leaf messages): bit-exact against the CPU oracle.  The transition polynomials are
    linear: degree-3 constraints are not expressible in the reference (quirk Q1)."""
    import time
    orc.set_threads(_oracle_threads())
    t0 = time.time()
    try:
        pc.case_prove_wide(mk, 0, log_n=22, w=64)
    finally:
        orc.set_threads(1)
    print(f"configs[4] wide AIR 2^22 rows: bit-exact vs oracle in {time.time() - t0:.0f} s ({_oracle_threads()} oracle threads)")


def test_rccl_binding_selftest(mk):
    """ms_set_shard_rccl's plumbing on one GPU: librccl.so bound at run time, a one-rank communicator, send/recv to self in a
    group, all-gather and both all-reduces on the context's stream with checked payloads."""
    ctx = mk(0, fresh=True)
    assert len(ctx.rccl_unique_id()) == 128
    rc = ctx.L.ms_rccl_selftest(ctx.h)
    assert rc == 0, ctx.last_error()
    ctx.set_shard_rccl(0, 1, bytes(128), 0)   # world 1 = sharding off
    pc.case_prove(lambda f, fresh=False: ctx, 0, 8, 8, read_big=False)


@pytest.mark.parametrize("field,log_n", [(0, 12), (1, 10), (0, 18)])
def test_mssp_roundtrip_across_processes(mk, field, log_n, tmp_path):
    """SURVEY 8(f) rank 3 on the HIP build: a GPU proof serialised by the C++ host mirror (msh_proof_serialize, MSSP), written to a
    file, deserialised and verified in a FRESH process (tests/verify_worker.py: msh_stark_verify_mssp)."""
    import subprocess
    import sys
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air, StarkProof
    build_host_library()
    ctx = mk(field)
    steps = (1 << log_n) - 1
    tt = fibonacci_air(ctx, steps)
    hs = HostStark(ctx, 20, 8, steps, tt.constrain_number())
    proof = hs.prove(tt)
    wire = hs.proof_bytes()
    assert wire == proof.to_bytes() and StarkProof.from_bytes(wire).fri_proof.blob == proof.fri_proof.blob
    f = tmp_path / "proof.mssp"
    f.write_bytes(wire)
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "verify_worker.py"), str(f), str(field), str(steps), "8"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "VERIFY accepted tampered-rejected" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.parametrize("field,log_rows", [(0, 12), (1, 10), (0, 16)])
def test_c_caller_on_gpu(field, log_rows, tmp_path):
    """SURVEY 8(f) rank 4 stand-in: examples/prove_c_caller.c, a compiled C program linked against libministark.so (HIP) and
    libministark_host.so, runs the reference's e2e flow (derive_constrains, prove, serialise, verify, tamper) on the GPU."""
    import test_c_caller as tcc
    out = tcc.build_and_run(os.path.dirname(ms.library_path()), "ministark", [field, log_rows, 8], tmp_path)
    assert out.returncode == 0 and "verify accepted, tampered rejected" in out.stdout, (out.stdout, out.stderr)


@pytest.mark.parametrize("v2", ["1", "0"])
def test_babybear_on_the_round2_tiles(mk, monkeypatch, v2):
    """BabyBear runs the cooperative round-2 tiles by default since r03; MS_NTT_V2=0 keeps the round-1 tiles, which stay in the
    library for single-pass sizes, other blowups and transforms beyond 2^25 non-zero points.  Both must be exact."""
    monkeypatch.setenv("MS_NTT_V2", v2)
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_ntt(fresh, 1, 16)
    pc.case_coset_lde(fresh, 1, 14, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1])
def test_lincomb_shared_sweep(mk, field):
    pc.case_lincomb_shared_sweep(lambda f: mk(f, fresh=True), field, log_n=12)


@pytest.mark.gpu
def test_async_proof_readback_on_gpu(mk):
    """ms_fri_proof_read_async: the 2^16-row proofs' FRI bytes arrive through the copy stream while the next proof is computed, identical
    to the blocking read-back; the next query phase orders itself behind the copy on the device."""
    from mini_stark_amd.host import HostStark
    from mini_stark_amd.stark import fibonacci_air
    ctx = mk(0, fresh=True)
    steps, blowup = (1 << 16) - 1, 8
    tts = [fibonacci_air(ctx, steps, secret_b=b) for b in (2, 7, 11)]
    hs = HostStark(ctx, 20, blowup, steps, tts[0].constrain_number())
    want = [hs.prove(tt).fri_proof.blob for tt in tts]
    assert len(set(want)) == 3
    for rep in range(2):
        got = []
        for tt in tts:
            ctx.check(hs.prove_raw(tt, read_fri_proof="async"))
            if rep == 0:
                got.append(hs.last_proof().fri_proof.blob)   # accessor waits
        if rep == 0:
            assert got == want
    assert hs.wait_proof() == 0
    assert hs.last_proof().fri_proof.blob == want[-1]
    # r04: the asynchronous read-back travels on an SDMA engine through the HSA runtime (never a blit kernel) unless MS_READBACK=hip
    assert ctx.L.ms_io_engine(ctx.h) == (0 if os.environ.get("MS_READBACK") == "hip" else 1), "the SDMA read-back did not bind: " + ctx.last_error()
    # r05: the copy engines go through the HSA runtime ALREADY mapped into the process (never one the library loads itself), and the library says which
    if os.environ.get("MS_READBACK") != "hip":
        path = ctx.io_runtime_path()
        assert "libhsa-runtime64" in path and os.path.exists(path), path
        mapped = [l.split()[-1] for l in open("/proc/self/maps") if "libhsa-runtime64" in l]
        assert os.path.realpath(path) in {os.path.realpath(m) for m in mapped}, (path, sorted(set(mapped)))   # (the loader's name of it may be a symlink)


@pytest.mark.parametrize("mode", ["hip", "sdma-async", "sdma"])
def test_readback_engines_deliver_the_same_bytes(monkeypatch, mode):
    """The three read-back paths of the boundary (MS_READBACK: the HIP runtime's copy, the SDMA engine for the asynchronous read-back, the SDMA engine for the
    blocking one too: the default) on a 2^18-row proof (16 MiB of FRI proof): same bytes in every mode, blocking and asynchronous, and ms_io_engine names the path taken."""
    from mini_stark_amd.host import HostStark
    from mini_stark_amd.stark import fibonacci_air
    monkeypatch.setenv("MS_READBACK", "hip")
    c0 = ms.Context(0)
    steps, blowup = (1 << 18) - 1, 8
    tt = fibonacci_air(c0, steps, secret_b=5)
    want = HostStark(c0, 20, blowup, steps, tt.constrain_number()).prove(tt).fri_proof.blob
    assert c0.L.ms_io_engine(c0.h) == 0
    monkeypatch.setenv("MS_READBACK", mode)
    ctx = ms.Context(0)
    hs = HostStark(ctx, 20, blowup, steps, tt.constrain_number())
    assert hs.prove(tt).fri_proof.blob == want                      # blocking read-back
    assert ctx.L.ms_io_engine(ctx.h) == (1 if mode == "sdma" else 0)
    for _ in range(3):
        ctx.check(hs.prove_raw(tt, read_fri_proof="async"))
    assert hs.wait_proof() == 0
    assert hs.last_proof().fri_proof.blob == want
    assert ctx.L.ms_io_engine(ctx.h) == (0 if mode == "hip" else 1)
    ctx.close(); c0.close()


@pytest.mark.parametrize("field", [0, 1])
def test_arith_selftest(mk, field):
    """ADVICE r2 / VERDICT r2 #3: the NTT tiles' arithmetic class op by op against big integers (GPU: the exec-masked asm class GLM itself;
    emulation: the formulas it falls back to - the entry point's plumbing)."""
    pc.case_arith_selftest(mk, field)


@pytest.mark.parametrize("field,log_n", [(0, 12), (1, 10), (0, 20)])
def test_proof_written_into_pinned_memory_on_gpu(mk, field, log_n):
    """ms_fri_query_into on the HIP build: the query-phase kernels store the MSFP blob straight into page-locked HOST memory (at 2^20 rows: 64 MiB
    over PCIe from the kernels themselves) - same bytes as the read-back; two proof slots keep proof k whole while k + 1 runs."""
    import test_host_mirror as thm
    from mini_stark_amd.host import build_host_library
    build_host_library()
    thm.check_into_and_slots(mk(field, fresh=True), (1 << log_n) - 1)


@pytest.mark.parametrize("field,virtual", [(0, "1"), (1, "1"), (0, "0")])
def test_virtual_linear_lde_columns(mk, monkeypatch, field, virtual):
    """r03: the linear LDE columns evaluated row by row inside the leaf-hash kernel (MS_LDE_VIRTUAL; default: AIRs of >= 16 polynomials) instead of being
    written out by the lincomb kernels - same LDE root, same LDE matrix on ms_lde_read (materialised on demand), same proof, forced on and off."""
    monkeypatch.setenv("MS_LDE_VIRTUAL", virtual)
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_prove(fresh, field, 8, 8)
    pc.case_prove(fresh, field, 6, 4, read_big=False)


@pytest.mark.parametrize("field,parents", [(0, "0"), (1, "0"), (0, "4"), (0, "4096"), (1, "1048576"), (0, "16384")])
def test_tree_levels_as_subtree_launches_or_one_by_one(mk, monkeypatch, field, parents):
    """r04: binary-tree levels of at most MS_TREE_SUBTREE_PARENTS parents (default 16384) run nine to a launch with the children in LDS (InnerSubtreeKernel);
    0: one launch per level and the fused top (the r01-r03 path, still what non-binary trees use).  Same roots, paths and proofs either way."""
    monkeypatch.setenv("MS_TREE_SUBTREE_PARENTS", parents)
    fresh = lambda f, fresh=False: mk(f, fresh=True)
    pc.case_prove(fresh, field, 13, 8, read_big=False)
    pc.case_prove(fresh, field, 3, 2, read_big=False)


@pytest.mark.parametrize("field,small_max", [(0, "0"), (1, "0"), (0, "1000000000"), (1, "1000000000")])
def test_eval_kernel_choice_by_polynomial_length(mk, monkeypatch, field, small_max):
    """r04: polynomials of at most MS_EVAL_SMALL_MAX coefficients (default 2^19) are evaluated with 4 coefficients per thread, longer ones with 16: the DEEP-ALI
    values and every FRI round's B with either kernel forced."""
    monkeypatch.setenv("MS_EVAL_SMALL_MAX", small_max)
    pc.case_prove(lambda f, fresh=False: mk(f, fresh=True), field, 13, 8, read_big=False)


@pytest.mark.parametrize("field,small_max", [(0, "0"), (1, "0"), (0, "1000000000"), (1, "1000000000")])
def test_fold_kernel_choice_by_round_size(mk, monkeypatch, field, small_max):
    """r04: rounds of at most MS_FOLD_SMALL_MAX outputs (default 131072) fold with one output per thread (latency), longer ones with eight (the inversion shared by
    eight norms): the same proof with every round forced through either kernel."""
    monkeypatch.setenv("MS_FOLD_SMALL_MAX", small_max)
    pc.case_prove(lambda f, fresh=False: mk(f, fresh=True), field, 12, 8, read_big=False)


@pytest.mark.parametrize("field,log_n,w", [(0, 4, 4), (1, 4, 4), (0, 6, 8), (1, 5, 7)])
def test_mix_cubic_true_quotient(mk, field, log_n, w):
    """BASELINE configs[4] "degree-3 constraints" (build-defined; VERDICT r2 missing #6): ms_mix_cubic against the big-integer definition, the DEEP-ALI
    identity, a full FRI over the 2N-coefficient validity polynomial, and the refusal of an invalid trace."""
    pc.case_mix_cubic(lambda f, fresh=False: mk(f, fresh=True), field, log_n=log_n, w=w)


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1])
def test_mix_cubic_failing_across_a_store_growth(mk, field):
    """A refused ms_mix_cubic that grew the polynomial store leaves no validity polynomial behind (ms_fri_begin refuses as before any mix stage); one that did not
    grow it leaves the earlier one in place."""
    pc.case_mix_cubic_store_growth(lambda f, fresh=False: mk(f, fresh=True), field)


def test_config4_degree3_constraints_full_width_self_verifies(mk):
    """BASELINE configs[4] as written - 64 trace columns, degree-3 constraints - at 2^18 rows (2^22 in bench.py's `extra.wide_air_cubic_2p22`): the build-defined
    composition has no reference to compare with, so it verifies itself: ms_mix_cubic accepts (exact division: nothing above 2N coefficients), and the DEEP-ALI
    identity validity(z) (z^N - 1) = (z - w^(N-1)) sum_t r^t C_t(z) holds at a random extension point with the 65 opened values at z and w z; a trace with one
    changed cell is refused."""
    from mini_stark_amd.host import build_host_library, cubic_rows_native
    from pyref import Tower
    from common import SplitMix64
    build_host_library()
    field, lr, w = 0, 18, 64
    P, N = 2**64 - 2**32 + 1, 1 << lr
    tr, sc = cubic_rows_native(P, N, w, 9)
    sc = [int(v) for v in sc]
    spec = [(j, j, (j + 1) % w, (j + 2) % w, (j + 3) % w) for j in range(w)]
    ctx = mk(field, fresh=True)
    omega = ctx.root_of_unity(N)
    rng = SplitMix64(77)
    assert ctx.trace_commit(tr, w)[0] == 0 and ctx.interpolate() == 0 and ctx.lde_commit(8, rng.nonzero(P), w)[0] == 0
    r = rng.field(P)
    assert ctx.mix_cubic(r, spec, sc) == 0, ctx.last_error()
    T = Tower(field, 2)
    z = (rng.field(P), rng.field(P))
    wz = T.mul(z, T.from_base(omega))
    rc, ev = ctx.eval_ext(np.array([z, wz], dtype=np.uint64))
    assert rc == 0
    E_ = lambda v: tuple(int(x) for x in v)
    Pz, Pwz, Vz = [E_(ev[0][j]) for j in range(w)], [E_(ev[1][j]) for j in range(w)], E_(ev[0][w])
    acc, rp = T.zero(), 1
    for (j, a, b, c_, d), s_ in zip(spec, sc):
        C_t = T.sub(T.sub(Pwz[j], T.mul(T.mul(Pz[a], Pz[b]), Pz[c_])), T.mul(Pz[d], T.from_base(s_)))
        acc = T.add(acc, T.mul(C_t, T.from_base(rp)))
        rp = rp * r % P
    assert T.mul(Vz, T.sub(T.pow(z, N), T.one())) == T.mul(acc, T.sub(z, T.from_base(pow(omega, N - 1, P))))
    rounds = lr + 1 + 3
    assert ctx.fri_begin(8, rounds)[0] == 0
    assert ctx.fri_round_info(0)[1] == 2 * N * 8
    bad = tr.copy()
    bad[N // 3, 5] = (int(bad[N // 3, 5]) + 1) % P
    ctx2 = mk(field, fresh=True)
    assert ctx2.trace_commit(bad, w)[0] == 0 and ctx2.interpolate() == 0 and ctx2.lde_commit(8, 12345, w)[0] == 0
    assert ctx2.mix_cubic(r, spec, sc) == ms.ERR_SHAPE


def test_merkle_commit_vs_reference_script_vectors():
    """VERDICT r3 missing #4: the HIP kernels meet reference-produced bytes directly - ms_merkle_commit(lpn = 1, ic = 2, zero printed as "0") against every
    vector of tests/golden/merkle_script_roots.json (leaf digests and root), generated by running the reference's scripts/merkle_tree.py."""
    pc.case_merkle_script_golden(lambda field, flags: ms.Context(field, flags=flags))


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup", [(12, 16), (12, 32), (5, 64), (9, 1)])
def test_prove_other_blowups(mk, field, log_n, blowup):
    """VERDICT r3 missing #5: StarkConfig::new takes any power-of-two blowup (starks.rs:268-310); beyond 8 the NTT plan leaves the virtual-pass fast path
    (zero padding of more than three bits), blowup 1 has no padding at all."""
    pc.case_prove(mk, field, log_n, blowup, read_big=False)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,steps", [(6, 40), (12, 3000), (12, 2048), (10, 513)])
def test_prove_several_padding_rows(mk, field, log_n, steps):
    """VERDICT r3 missing #5: traces with several padding rows (air.rs:73-96: the domain is the next power of two above steps + 1, the rows behind `steps` are random)."""
    pc.case_prove(mk, field, log_n, 8, read_big=False, steps=steps)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup", [(10, 16), (14, 16), (12, 32), (16, 16)])
def test_coset_lde_other_blowups(mk, field, log_n, blowup):
    pc.case_coset_lde(mk, field, log_n, blowup)


@pytest.mark.parametrize("upload", ["sdma", "hip"])
def test_trace_upload_from_page_locked_memory(monkeypatch, upload):
    """The other bulk transfer of the boundary: a trace handed over in page-locked host memory (ms_pinned_alloc) travels on an SDMA engine through the HSA runtime
    (MS_UPLOAD=sdma, the default) or by hipMemcpyAsync (hip) - same trace root, same LDE root, same DEEP values as from a pageable numpy array."""
    import ctypes as C
    monkeypatch.setenv("MS_UPLOAD", upload)
    ctx = ms.Context(0)
    N, w = 1 << 18, 3
    trace = fibonacci_trace_fast(0, N)
    rc, want_root = ctx.trace_commit(trace, 6)          # pageable source
    assert rc == 0
    ctx.L.ms_pinned_alloc.restype = C.c_void_p
    ctx.L.ms_pinned_free.argtypes = [C.c_void_p]
    p = ctx.L.ms_pinned_alloc(C.c_size_t(N * w * 8))
    assert p
    try:
        C.memmove(p, trace.ctypes.data, N * w * 8)
        root = (C.c_uint8 * 32)()
        for _ in range(2):                               # twice: the second upload overwrites a device buffer the first proof's kernels have read
            assert ctx.L.ms_trace_commit(ctx.h, C.c_void_p(p), C.c_size_t(N), C.c_size_t(w), C.c_size_t(6), root) == 0, ctx.last_error()
            assert bytes(root) == want_root
        ctx.N, ctx.w = N, w
        assert ctx.interpolate() == 0
        for sc, idx in fibonacci_closures(0, N, orc.root_of_unity(0, N)):
            assert ctx.polys_lincomb(sc, idx) == 0
        rc, lde_root = ctx.lde_commit(8, 12345, 6)
        c2 = ms.Context(0)
        assert c2.trace_commit(trace, 6)[0] == 0 and c2.interpolate() == 0
        for sc, idx in fibonacci_closures(0, N, orc.root_of_unity(0, N)):
            assert c2.polys_lincomb(sc, idx) == 0
        assert rc == 0 and c2.lde_commit(8, 12345, 6) == (0, lde_root)
        # a non-canonical element in page-locked memory is still refused (the range check runs in the transposing kernel)
        bad = trace.copy(); bad[7, 1] = MODULUS[0] + 5
        C.memmove(p, bad.ctypes.data, N * w * 8)
        assert ctx.L.ms_trace_commit(ctx.h, C.c_void_p(p), C.c_size_t(N), C.c_size_t(w), C.c_size_t(6), root) == ms.ERR_ARG
    finally:
        ctx.close()
        ctx.L.ms_pinned_free(C.c_void_p(p))


@pytest.mark.parametrize("field,log_n,rccl,env,root_only", [(0, 12, False, {}, False), (0, 16, True, {}, False), (1, 14, True, {"MS_SHARD_SLICES": "4", "MS_SHARD_SLICE_MIN": "64"}, True),
                                                           (0, 18, True, {"MS_SHARD_SLICES": "4", "MS_SHARD_MIN_LEAVES": "32768"}, False),
                                                           (0, 16, True, {"MS_RCCL_MAX_PIECE": "4096"}, True), (1, 14, True, {"MS_RCCL_MAX_PIECE": "1024", "MS_SHARD_SLICES": "2", "MS_SHARD_SLICE_MIN": "64"}, False),
                                                           (0, 17, True, {"MS_FRI_OVERLAP": "1", "MS_SYNC_POLL": "1", "MS_SHARD_MIN_LEAVES": "4096", "MS_FRI_TAIL_MAX": "256"}, False), (1, 14, False, {"MS_FRI_TAIL_MAX": "0", "MS_FRI_OVERLAP": "1", "MS_SYNC_POLL": "1"}, True)])
def test_sharded_code_paths_on_one_rank_on_gpu(monkeypatch, field, log_n, rccl, env, root_only):
    """The sharded prover on a one-rank world on the real kernels (MS_SHARD_WORLD1=1).  rccl=True: the exchanges are RCCL calls inside the library on a one-rank communicator -
    grouped ncclSend / ncclRecv (to itself), ncclAllGather, ncclAllReduce, the sliced digest exchange on its own stream behind events, the gather to rank 0 - so the RCCL branch,
    which no multi-GPU box has run yet, executes through whole proofs with real buffers and stream ordering, bit-exact against the oracle (2^18 rows with the default threshold).
    MS_RCCL_MAX_PIECE (r05): every transfer cut into pieces of that many bytes - the loop that keeps a single ncclSend / ncclRecv below 2 GiB (RCCL 2.26.6 delivers wrong bytes
    beyond: test_config3_sharded_form_2p24_rows_matches_unsharded), forced at small sizes.  MS_FRI_OVERLAP=1 MS_SYNC_POLL=1 (r05; what MS_FLAG_LATENCY sets): the latency mode's side stream and polled results (the sharded trees' top launch carries the flag; stages that end in a collective keep the stream synchronisation) in the replicated rounds of a
    sharded proof (distributed rounds keep one stream); MS_FRI_TAIL_MAX=0: those rounds launch per step instead of fused."""
    import torch
    monkeypatch.setenv("MS_SHARD_WORLD1", "1")
    monkeypatch.setenv("MS_SHARD_MIN_LEAVES", "64")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if log_n >= 16:
        orc.set_threads(8)
    try:
        st, dist_rounds = pc.case_sharded_paths_on_one_rank(lambda f: ms.Context(f), field, log_n, 8, rccl=rccl, device=torch.device("cuda", 0), root_only=root_only)
    finally:
        orc.set_threads(1)
    assert st[0] >= 3 and st[1] > st[0] and st[2] == 1 and st[3] == 1 and dist_rounds >= 2


def _env_setter(monkeypatch):
    def set_env(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    return set_env


def test_config3_sharded_form_2p24_rows_matches_unsharded(monkeypatch):
    """BASELINE configs[3] in its SHARDED form at full size - 2^24-row Goldilocks proof (4 GiB digest exchanges, ~1 GiB proof, 12 distributed rounds) through
    the sharded code paths on a one-rank RCCL communicator inside the library: plain and sliced digest exchange, proof on every rank and on rank 0 only.  Trace root, LDE
    root, DEEP values, every FRI round's B, root and length and the SHA-256 of the FRI blob equal the UNSHARDED proof of the same library, which
    test_config3_2p24_rows_bit_exact_vs_oracle pins to the oracle."""
    import torch
    variants = [(True, {}, False), (True, {"MS_SHARD_SLICES": "4"}, True), (True, {"MS_SHARD_SLICES": "4"}, False), (True, {}, True)]
    res = pc.case_sharded_one_rank_matches_unsharded(lambda f: ms.Context(f), 0, 24, variants, _env_setter(monkeypatch), device=torch.device("cuda", 0))
    for st, dist_rounds in res:
        assert st[0] >= 10 and st[1] > st[0] and st[2] == 1 and st[3] == 1 and dist_rounds >= 10, (st, dist_rounds)


def test_config4_sharded_form_wide_air_2p22_rows_matches_unsharded(monkeypatch):
    """BASELINE configs[4] in its SHARDED form at full size - the 64-column, c = 128 wide AIR at 2^22 rows (2.5 KB leaf messages, 1 GiB digest exchange
    for the LDE) on the one-rank RCCL world, plain and sliced, against the unsharded proof of the same library (pinned to the oracle by
    test_config4_wide_air_2p22_rows_bit_exact_vs_oracle)."""
    import torch
    variants = [(True, {}, False), (True, {"MS_SHARD_SLICES": "4"}, True)]
    res = pc.case_sharded_one_rank_matches_unsharded(lambda f: ms.Context(f), 0, 22, variants, _env_setter(monkeypatch), wide_w=64, device=torch.device("cuda", 0), seed=5)
    for st, dist_rounds in res:
        assert st[0] >= 8 and st[1] > st[0] and dist_rounds >= 8, (st, dist_rounds)


def test_sharded_2p22_rows_on_4_gloo_ranks_matches_unsharded():
    """a 2^22-row Fibonacci proof over FOUR ranks sharing this GPU (gloo; default MS_SHARD_MIN_LEAVES: LDE + ten FRI rounds sharded, round polynomials
    distributed): every rank's outputs equal an UNSHARDED proof of the same library computed by that rank (shard_worker.py gpu-self)."""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", "29967", os.path.join(here, "shard_worker.py"), "0", "22", "8", "32768", "gpu-self"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    calls = {int(k): v for k, v in res["calls"].items()}
    assert res["world"] == 4 and calls[0] >= 10 and calls[2] == 1 and calls[3] == 1 and res["dist_rounds"] >= 9, res


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,blowup,tail_max,fused", [(13, 8, "0", False), (13, 8, "8192", True), (16, 8, "1048576", True), (12, 2, "1048576", True), (10, 16, "64", True)])
def test_fri_tail_rounds_fused_and_launch_per_step(monkeypatch, field, log_n, blowup, tail_max, fused):
    """r05: a tail round of the FRI commit phase as ONE launch (csrc/fri_tail.hpp) on the real kernels - the completion counter, the device-scope
    fences and the last workgroup's tree top included - against the oracle: off, at the default threshold, and forced up to 2^20-point domains (512 evaluation-side
    workgroups, nine top levels)."""
    if log_n >= 16:
        orc.set_threads(8)
    try:
        pc.case_fri_tail(lambda f: ms.Context(f), field, log_n, blowup, tail_max, _env_setter(monkeypatch), fused)
    finally:
        orc.set_threads(1)


@pytest.mark.parametrize("field,log_n", [(0, 13), (1, 12), (0, 16), (0, 21)])
def test_latency_flag_side_stream_same_proof(field, log_n):
    """r05: MS_FLAG_LATENCY - a FRI round's coefficient side (fold, DEEP-quotient scan, trimmed length) on a side stream beside its evaluation side, joined by an event in
    front of the launch that forwards root and length word: the oracle's proof, twice on the same context (the second proof reuses streams, events and the length word).
    The flag also makes the host POLL a sequence number the stage's last kernel stores behind its results instead of synchronising with the stream (ctx.hpp Results::collect);
    2^21 rows: stages longer than the 2 ms the host spins for, which fall back to the blocking wait."""
    if log_n >= 16:
        orc.set_threads(8)
    try:
        ctx = ms.Context(field, flags=ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_LATENCY)
        for _ in range(1 if log_n >= 21 else 2):   # (2^21 rows: once - the oracle's proof is 20 s of the suite)
            pc.case_prove(lambda f, fresh=False: ctx, field, log_n, 8, read_big=False)
        ctx.close()
    finally:
        orc.set_threads(1)


@pytest.mark.parametrize("latency", [False, True])
def test_many_contexts_in_flight_prove_the_same(latency):
    """r05: twelve proving threads, one context each, from their FIRST proof on (lazy buffers, plans, streams), every stage output against a single-lane proof
    (tools/multi_lane_check.py).  The parity suite proves on one context at a time; the race this found - the length word zeroed lazily on one stream while the other
    stream's scan already wrote it, visible only from eight lanes up - is the kind it cannot see."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "multi_lane_check.py"), "--lanes", "12", "--log-rows", "17", "--proofs", "4"] + (["--latency"] if latency else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
