#!/usr/bin/env python3
"""bench.py — STARK proofs/s on the BASELINE.json workload, one process per GPU.

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one complete proof of the hot path (src/starks.rs:59-169 between
"trace filled" and "StarkProof returned"): trace commit, INTT, coset LDE,
LDE commit, mix, DEEP-ALI evaluations, FRI commit phase (all rounds) and FRI
query phase, with the Fibonacci-AIR trace already resident in HBM and the FRI
proof left resident in HBM (the PCIe-inclusive rate is the `value_with_io`
leg).  Headline workload at every N: BASELINE.json configs[1] — Fibonacci AIR,
Goldilocks, 2^20 trace rows, blowup 8, 20 security bits — independent proofs on
every rank (weak scaling: the path partitions over proofs; no data-path
collective).

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times --steps steps and prints the headline (`value`, `ms_per_step`); with
--dump-outputs DIR it first writes the proofs of the last timed step under DIR (dump_outputs).  With --full the line carries besides the headline
  roofline       per-kernel HIP-event timing of the dominant NTT pass kernel vs its algorithmic bytes
  roofline_valu  the SHA-256 kernels (59 % of the kernel time) against the VALU issue roofline
  sharded        N > 1 only: ONE 2^24-row proof (BASELINE configs[3]) computed by all ranks together (ms_set_shard_rccl:
                 coset-partitioned LDE/FRI + leaf hashing, RCCL digest all-to-all + root all-gather inside the library; r04: the
                 coefficient-domain work by coefficient range, the FRI proof assembled on rank 0; strong scaling), in a child process
                 per rank so that neither a hang nor a crash there can take the headline down; reports collective calls, bytes,
                 distributed rounds, partitioned / replicated kernel time (HIP events) and matches_unsharded
  extra          N == 1 only: 2^24-row Goldilocks and 2^20-row BabyBear+Fp4 proofs/s, NTT-only GB/s at 2^20 and 2^24 rows,
                 `value_with_io` (trace from pinned host memory, FRI proof read back, both on SDMA engines, overlapped over the
                 in-flight lanes) and `io_paired` (resident and I/O-inclusive rates alternated: the ratio to quote)
  value_with_io  N == 1 only, top level: the I/O-inclusive rate beside `value` (the contract keeps `value` = traces resident in HBM)
  cpu_baseline   N == 1 only: the CPU oracle ("port") on the same 2^20-row proof, 1 thread and OpenMP
`--mode shard` makes the sharded proof the timed step instead (the latency configuration for single large proofs).
"""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
N_SIMD, CLOCK_HZ = 1024, 2.4e9  # 256 CUs x 4 SIMD-32, 2.4 GHz max clock (same guide)


def default_inflight(log_rows):
    # 8 fills the 4 hardware queues twice over at the benchmark size; larger proofs need the HBM (25 GiB each at 2^24 rows)
    # (2^24 rows: 25 GiB resident per proof; same-box A/B r04: 2 in flight 16.4-16.5 proofs/s, 3: 17.0-17.3, 4: 17.3-17.5 - profiles/r04_ab_2p24_inflight.log)
    return 8 if log_rows <= 20 else (6 if log_rows == 21 else 4)


EMU_LIB = os.path.join(ROOT, "tests", "emu", "libministark_emu.so")


def lib_path_for(args):
    """None = the product library (HIP, gfx950).  --emu: the CPU emulation build of the same kernel source (tests/emu) - a REHEARSAL of the
    launch / collective plumbing on a box without enough GPUs; its timings mean nothing and the JSON line says so."""
    return EMU_LIB if getattr(args, "emu", False) else None


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_wave(argv, world, timeout, extra_env=None):
    """N fresh child processes of this script, one rank each (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set): what
    `python -m torch.distributed.run --nproc-per-node N` would start.  The parent never touches the GPU (no torch import, no HIP call).
    Returns (rc, rank 0's stdout lines, stderr tail of the first failing rank)."""
    import subprocess
    import tempfile
    env0 = dict(os.environ)
    env0.update({"WORLD_SIZE": str(world), "LOCAL_WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(_free_port()), "MS_BENCH_LAUNCHED": "1"})
    env0.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env0.update(extra_env or {})
    procs, outs = [], []
    for r in range(world):
        env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
        fo = tempfile.TemporaryFile(mode="w+")
        outs.append(fo)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, stdout=fo, stderr=None))
    deadline = time.time() + timeout
    rc, failed = 0, None
    pending = set(range(world))
    while pending and rc == 0:
        for r in sorted(pending):
            c = procs[r].poll()
            if c is not None:
                pending.discard(r)
                if c != 0:
                    rc, failed = c, r
        if time.time() > deadline:
            rc, failed = 124, -1
        if pending and rc == 0:
            time.sleep(0.05)
    if rc != 0:   # one rank failed (or the wave timed out): end the others - exactly the PIDs started here
        for r in pending:
            procs[r].terminate()
        for r in pending:
            try:
                procs[r].wait(timeout=20)
            except Exception:
                procs[r].kill()
    outs[0].seek(0)
    lines = outs[0].read().splitlines()
    for fo in outs:
        fo.close()
    return rc, lines, failed


def launch_ranks(args, argv):
    """`python bench.py --gpus N` without torchrun: start the N ranks here.  Wave 1 = the replicas leg (headline), wave 2 = the sharded
    2^24-row proof (fresh processes again, so that neither a hang nor a crash of it can take the headline down); the parent merges rank 0's
    two JSON lines into ONE line on stdout and exits non-zero if the headline wave failed."""
    world = args.gpus
    rc, lines, failed = _run_wave(argv, world, timeout=args.launch_timeout)
    js = [l for l in lines if l.startswith("{")]
    if rc != 0 or not js:
        print(f"[bench] rank {failed} of the {world}-rank run failed with code {rc}" if rc else "[bench] rank 0 printed no JSON line", file=sys.stderr, flush=True)
        sys.exit(rc or 1)
    out = json.loads(js[-1])
    out["launcher"] = "bench.py (self-launched ranks; no torchrun)"
    if args.mode == "replicas" and args.full and not args.no_shard_leg:
        sargv = ["--gpus", str(world), "--mode", "shard", "--log-rows", str(args.shard_log_rows), "--steps", str(args.shard_steps), "--warmup", "1", "--backend", args.backend,
                 "--field", str(args.field), "--blowup", str(args.blowup), "--no-cpu-baseline", "--no-extras", "--full"] + (["--emu"] if args.emu else [])
        # the sliced digest exchange (hashing overlapped with the all-to-all on a second stream) has never run on more than one GPU: try it first, and if that
        # wave fails or disagrees with the unsharded proof, run the plain exchange in a fresh wave and say which one the numbers come from
        rc2, lines2, failed2 = _run_wave(sargv, world, timeout=args.shard_timeout, extra_env={"MS_SHARD_SLICES": os.environ.get("MS_SHARD_SLICES", "4")})
        js2 = [l for l in lines2 if l.startswith("{")]
        ok2 = rc2 == 0 and js2 and (json.loads(js2[-1])["exchange"].get("matches_unsharded") or {}).get("all", True)
        if not ok2 and "MS_SHARD_SLICES" not in os.environ:
            first_try = {"rc": rc2, "failed_rank": failed2, "matches_unsharded": (json.loads(js2[-1])["exchange"].get("matches_unsharded") if js2 else None)}
            rc2, lines2, failed2 = _run_wave(sargv, world, timeout=args.shard_timeout, extra_env={"MS_SHARD_SLICES": "1"})
            js2 = [l for l in lines2 if l.startswith("{")]
            if rc2 == 0 and js2:
                out["sharded"] = json.loads(js2[-1])["exchange"]
                out["sharded"]["sliced_exchange_first_try"] = first_try
        if "sharded" in out:
            pass
        elif rc2 == 0 and js2:
            out["sharded"] = json.loads(js2[-1])["exchange"]
        elif rc2 == 124:
            out["sharded"] = {"error": f"the sharded leg did not finish within {args.shard_timeout:.0f} s; headline unaffected"}
        else:
            out["sharded"] = {"error": f"sharded leg: rank {failed2} exited with code {rc2}; headline unaffected"}
    print(json.dumps(out), flush=True)


class Lanes:
    """`inflight` independent provers on one GPU: one ms_ctx (own HIP stream, own HBM buffers), one host thread and one C++
    host-mirror Stark each.  io=False: traces resident in HBM, FRI proofs left in HBM.  io=True: every proof uploads its trace
    from page-locked host memory and reads the FRI proof back into page-locked host memory."""

    def __init__(self, field, log_rows, blowup, inflight, device_index, dev, seed0=2, io=False, lib=None, io_mode="async", upload=None, flags=None, prefetch=True):
        import numpy as np
        import torch
        import mini_stark_amd as ms
        from mini_stark_amd.stark import StarkConfig, fibonacci_air
        from mini_stark_amd.host import HostStark
        self.ms, self.io, self.n, self.io_mode = ms, io, inflight, io_mode
        self.samples = [set() for _ in range(inflight)]
        # lane i starts i ms after lane 0 (inside the timed region): proofs that start together stay in lock-step for tens of proofs - all lanes in the latency-bound late FRI
        # rounds at the same time, then all in the LDE hashing - and a 20-step run measured 246 proofs/s that way against 256 with the stagger (r03; profiles/HISTORY.md)
        self.stagger_ms = float(os.environ.get("MS_BENCH_STAGGER_MS", "1"))
        steps = (1 << log_rows) - 1  # "2^k trace rows" => steps = 2^k - 1 (quirk Q3)
        self.prefetch = prefetch   # io: every proof names the next proof's trace (here: the lane's own, again), whose upload then overlaps the proof (ms_trace_upload_async)
        kw = {} if flags is None else {"flags": flags}
        self.ctxs = [ms.Context(field, device=device_index, lib_path=lib, **kw) for _ in range(inflight)]
        self.tts = [fibonacci_air(c, steps, secret_b=seed0 + i) for i, c in enumerate(self.ctxs)]
        self.cfg = StarkConfig(self.ctxs[0], 20, blowup, steps, self.tts[0].constrain_number())
        self.starks = [HostStark(c, 20, blowup, steps, self.tts[0].constrain_number()) for c in self.ctxs]
        self.upload = io if upload is None else upload   # (tools/io_probe3.py splits the I/O leg into its upload and read-back halves)
        if self.upload:
            self.pinned = [torch.from_numpy(t.data.view(np.int64)).pin_memory() for t in self.tts]
            for t, pt in zip(self.tts, self.pinned):   # prove_raw takes the host pointer from trace.data
                t.data = pt.numpy().view(np.uint64)
            self.d_traces = [None] * inflight
        else:
            self.d_traces = [torch.from_numpy(t.data.view(np.int64)).to(dev) for t in self.tts]  # resident in HBM before the timed region
        if dev.type == "cuda":
            torch.cuda.synchronize()
        self.last = [None] * inflight

    def _prove_n(self, i, n):
        ptr = None if self.upload else self.d_traces[i].data_ptr()
        if self.stagger_ms and self.n > 1:
            time.sleep(i * self.stagger_ms * 1e-3)
        for k in range(n):
            # io, mode "into" (default): the query-phase kernels write the FRI proof straight into the mirror's page-locked slot (ms_fri_query_into) - it is
            # complete when prove returns, and EVERY proof is touched on the host (one word per page) before its slot is reused two proofs later.
            # io, mode "async": the read-back of proof k (copy stream) overlaps the first stages of proof k + 1; proof k is sampled from the mirror's OTHER
            # slot after prove k + 1 returned (two proof slots: ADVICE r2), the last one after the final wait.
            if self.upload and self.prefetch and k + 1 < n:
                self.starks[i].next_trace(self.tts[i].data.ctypes.data, self.tts[i].length, self.tts[i].width)
            self.ctxs[i].check(self.starks[i].prove_raw(self.tts[i], trace_device_ptr=ptr, read_fri_proof=self.io_mode if self.io else False))
            if self.io and self.io_mode == "into":
                self.samples[i].add(self.starks[i].blob_sample(0))
            elif self.io and k:
                self.samples[i].add(self.starks[i].blob_sample(1))
        if self.io and self.io_mode != "into":
            self.ctxs[i].check(self.starks[i].wait_proof())
            self.samples[i].add(self.starks[i].blob_sample(0))
        self.last[i] = self.starks[i].last_proof(read_fri_proof=False)

    def run(self, n):  # n steps = n proofs on each lane (ctypes releases the GIL inside the library)
        if self.n == 1:
            self._prove_n(0, n)
            return
        errs = [None] * self.n

        def lane(i):
            try:
                self._prove_n(i, n)
            except BaseException as e:  # noqa: BLE001 - re-raised below: a lane that died (e.g. MS_ERR_NOMEM with too many proofs in flight) must fail the run, not shorten it
                errs[i] = e
        th = [threading.Thread(target=lane, args=(i,)) for i in range(self.n)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for i, e in enumerate(errs):
            if e is not None:
                raise RuntimeError(f"lane {i} of {self.n} failed: {e}") from e

    def timed(self, grp, steps, warmup):
        if self.n > 1:
            # untimed: every kernel's first launch happens on ONE thread before the lanes start.  HIP loads a module's code object and resolves a kernel on its first
            # launch under a runtime lock; eight threads doing that at once serialise there and the one-off cost would land in the lanes' warm-up (or, with --warmup 0,
            # timed) proofs.  A timing measure, not a correctness workaround (profiles/r04_sigsegv_analysis.md)
            self._prove_n(0, 1)
        self.run(warmup)
        grp.barrier()
        t0 = time.perf_counter()
        self.run(steps)
        grp.barrier()
        return grp.max_over_ranks(time.perf_counter() - t0)

    def close(self):
        self.starks = None
        for c in self.ctxs:
            c.close()
        self.d_traces = None


def sharded_leg(args, grp, local_rank, log_rows, steps, warmup):
    """ONE proof per step computed by all ranks together; the collectives run inside the library (RCCL) unless --backend gloo."""
    import numpy as np
    import torch
    import mini_stark_amd as ms
    from mini_stark_amd.stark import StarkConfig, fibonacci_air
    from mini_stark_amd.host import HostStark
    from mini_stark_amd.dist import RcclShard, ShardExchange
    N = 1 << log_rows
    lib = lib_path_for(args)
    ctx = ms.Context(args.field, device=local_rank, lib_path=lib)
    cap = 32 * N * args.blowup // grp.world + (4 << 20)   # leaf digests of the largest commitment / world + the query phase's Merkle paths
    dev = torch.device("cpu") if args.emu else torch.device("cuda", local_rank % max(1, torch.cuda.device_count()))
    if args.backend == "nccl":
        xchg = RcclShard(grp, ctx, cap)
        how = "RCCL inside the library (ms_set_shard_rccl): ncclSend/ncclRecv all-to-all of leaf digests + ncclAllGather of subtree roots per large commitment, 2 ncclAllReduce in the query phase, all on the prover's stream"
    else:
        xchg = ShardExchange(grp, ctx, cap, staged=not args.emu, buffer_device=dev)
        how = "gloo rehearsal through the exchange callback (payloads staged through host memory)"
    ctx.shard_proof_on_root(True)    # Stark::prove returns ONE proof: the ranks' slices of the FRI proof are gathered to rank 0 (not all-gathered)
    tt = fibonacci_air(ctx, N - 1)   # every rank holds the same trace
    cfg = StarkConfig(ctx, 20, args.blowup, N - 1, tt.constrain_number())
    hs = HostStark(ctx, 20, args.blowup, N - 1, tt.constrain_number())
    d_trace = torch.from_numpy(tt.data.view("int64")).to(dev)
    if dev.type == "cuda":
        torch.cuda.synchronize()

    def prove(n):
        for _ in range(n):
            ctx.check(hs.prove_raw(tt, trace_device_ptr=d_trace.data_ptr(), read_fri_proof=False))
    prove(warmup)
    grp.barrier()
    t0 = time.perf_counter()
    prove(steps)
    grp.barrier()
    el = grp.max_over_ranks(time.perf_counter() - t0)
    mine = hs.last_proof(read_fri_proof=False)
    if args.dump_outputs and grp.rank == 0:   # ms_shard_proof_on_root: rank 0 holds the whole FRI proof
        dump_outputs(args.dump_outputs, [mine], [ctx.fri_proof_read()])
    roots = grp.all_gather_bytes(mine.fri_roots[-1])
    calls = dict(xchg.calls)     # (a snapshot: the profiled proof below goes through the same exchange)
    nbytes = xchg.bytes
    dist_rounds = sum(1 for i in range(cfg.rounds) if ctx.L.ms_shard_round_is_distributed(ctx.h, C.c_int(i)) == 1)
    shard_prof, stage_ms = {}, {}
    if args.full:
        # one more (untimed) proof with every launch bracketed by HIP events: kernel time of this rank's PART of the proof vs kernel time REPLICATED on every rank
        buf = C.create_string_buffer(1 << 15)
        ctx.check(ctx.L.ms_profile_begin(ctx.h))
        prove(1)
        ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
        shard_prof = json.loads(buf.value.decode()).get("shard", {})
        # ... and one more through the stage functions one by one (fixed challenges, every rank the same calls): host-visible milliseconds per stage of the sharded proof,
        # what a first real multi-GPU run needs to see where the time goes (collectives included)
        try:
            from mini_stark_amd.synthetic import SplitMix64
            P, e = (2**64 - 2**32 + 1, 2) if args.field == 0 else (2013265921, 4)
            rng = SplitMix64(99)

            def st(name, fn):
                t = time.perf_counter(); r = fn(); stage_ms[name] = stage_ms.get(name, 0.0) + (time.perf_counter() - t) * 1e3
                return r
            ctx.check(st("trace_commit", lambda: ctx.trace_commit_device(d_trace.data_ptr(), N, 3, tt.constrain_number()))[0])
            ctx.check(st("interpolate", ctx.interpolate))
            for sc, idx in tt.transitions:
                ctx.check(st("polys_lincomb", lambda: ctx.polys_lincomb(sc, idx)))
            ctx.check(st("lde_commit", lambda: ctx.lde_commit(args.blowup, rng.next() % P or 3, tt.constrain_number()))[0])
            ctx.check(st("mix", lambda: ctx.mix(rng.next() % P)))
            ctx.check(st("eval_ext", lambda: ctx.eval_ext(np.array([rng.next() % P for _ in range(e)], dtype=np.uint64)))[0])
            ctx.check(st("fri_begin", lambda: ctx.fri_begin(args.blowup, cfg.rounds))[0])
            for _ in range(1, cfg.rounds):
                ctx.check(st("fri_deep", lambda: ctx.fri_deep([rng.next() % P for _ in range(e)]))[0])
                ctx.check(st("fri_fold_commit", lambda: ctx.fri_fold_commit([rng.next() % P for _ in range(e)]))[0])
            ctx.check(st("fri_query", lambda: ctx.fri_query([rng.next() for _ in range(cfg.fri_queries)], read=False))[0])
            stage_ms = {k: round(v, 3) for k, v in stage_ms.items()}
        except Exception as ex:  # noqa: BLE001 - a diagnostic must not take the leg down
            stage_ms = {"error": f"{type(ex).__name__}: {ex}"}
    # the same trace proved UNSHARDED by rank 0 on a second context: pins the exchange path (a symmetric error - wrong chunk order in the
    # all-to-all, a mistake in the in-place all-reduce - gives every rank the same wrong root and would pass `all_ranks_same_final_root`)
    matches = None
    if grp.rank == 0 and args.full and not args.no_shard_check:
        c1 = ms.Context(args.field, device=local_rank, lib_path=lib)
        h1 = HostStark(c1, 20, args.blowup, N - 1, tt.constrain_number())
        c1.check(h1.prove_raw(tt, trace_device_ptr=d_trace.data_ptr(), read_fri_proof=False))
        ref = h1.last_proof(read_fri_proof=False)
        matches = {"trace_root": ref.trace_commit == mine.trace_commit, "lde_root": ref.constrain_trace_commit == mine.constrain_trace_commit,
                   "all_fri_roots": list(ref.fri_roots) == list(mine.fri_roots), "deep_values": bool((ref.constrain_queries == mine.constrain_queries).all() and (ref.validity_queries == mine.validity_queries).all()),
                   "transcript": ref.arthur == mine.arthur}
        matches["all"] = all(matches.values())
        del h1
        c1.close()
    grp.barrier()
    res = {"workload": f"Fibonacci AIR, {'Goldilocks' if args.field == 0 else 'BabyBear+Fp4'}, 2^{log_rows} trace rows, blowup {args.blowup} (rounds={cfg.rounds}): ONE proof per step over {grp.world} ranks",
           "scaling": "strong", "value": steps / el, "unit": "proofs/s", "ms_per_proof": el / steps * 1e3, "steps": steps, "warmup": warmup,
           "ranks_in_communicator": grp.world, "parallelism": how, "all_ranks_same_final_root": len(set(roots)) == 1,
           "matches_unsharded": matches,
           "collective_calls_per_rank": {n: calls[i] for i, n in enumerate(["all_to_all", "all_gather", "all_reduce_min", "all_reduce_sum"])},
           "collective_calls_per_rank_per_proof": {n: calls[i] / max(1, steps + warmup) for i, n in enumerate(["all_to_all", "all_gather", "all_reduce_min", "all_reduce_sum"])},
           "bytes_sent_per_rank": nbytes, "proofs": steps + warmup,
           "distributed_rounds": dist_rounds, "rounds": cfg.rounds, "fri_proof_assembled_on": "rank 0 only (ms_shard_proof_on_root)",
           "digest_exchange_slices": int(os.environ.get("MS_SHARD_SLICES", "1" if args.backend == "nccl" else "4")),
           "partitioned_ms_estimate": shard_prof.get("partitioned_ms"), "replicated_ms_estimate": shard_prof.get("replicated_ms"),
           "replicated_ms_by_kernel": shard_prof.get("replicated_by_kernel"), "stage_ms_rank0_one_proof": stage_ms,
           "replicated_ms_note": "rank 0, one extra proof with per-launch HIP events (they add launch overhead): kernel time of launches that work on this rank's 1/world part of the proof "
                                 "(partitioned) and of launches every rank repeats (replicated: INTT, constraint polynomials, mix, tree tops, commitments below MS_SHARD_MIN_LEAVES); "
                                 "DESIGN.md 5"}
    xchg.close()
    ctx.close()
    return res, cfg


FRI_SAMPLE_WORDS = 1 << 18   # u32 words of each FRI proof kept by --dump-outputs (2 MiB per proof as float64; 8 proofs in flight: 16 MiB)


def dump_outputs(out_dir, proofs, blobs):
    """--dump-outputs: what the timed path returned in its last step, one row per proof (the lanes in order), as float64 .npy files that hold every
    value exactly: digests, roots and the transcript as bytes (0..255), field elements as their two u32 halves (low half first).  A FRI proof (MSFP,
    ~64 MiB at 2^20 rows) is kept as its SHA-256, its length and a fixed sample of its u32 words (seeded; the same positions in every proof).
    `blobs` yields the FRI proofs in lane order; one is held in host memory at a time."""
    import hashlib
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)

    def u8(bs):
        return np.stack([np.frombuffer(b, dtype=np.uint8) for b in bs]).astype(np.float64)

    def u64_halves(a):
        a = np.asarray(a, dtype=np.uint64)
        return np.stack([a & np.uint64(0xFFFFFFFF), a >> np.uint64(32)], axis=-1).astype(np.float64)
    sha, nbytes, sample, idx = [], [], [], None
    for b in blobs:
        w = np.frombuffer(b, dtype="<u4", count=len(b) // 4)   # (a tail of < 4 bytes is covered by the digest)
        if idx is None:
            idx = np.sort(np.random.default_rng(0).choice(len(w), size=min(FRI_SAMPLE_WORDS, len(w)), replace=False))
        sha.append(hashlib.sha256(b).digest())
        nbytes.append(len(b))
        sample.append(w[idx])
    arrays = {"trace_commit": u8([p.trace_commit for p in proofs]),
              "constrain_trace_commit": u8([p.constrain_trace_commit for p in proofs]),
              "fri_roots": np.stack([u8(p.fri_roots) for p in proofs]),
              "constrain_queries": u64_halves(np.stack([p.constrain_queries for p in proofs])),
              "validity_queries": u64_halves(np.stack([p.validity_queries for p in proofs])),
              "transcript": u8([p.arthur for p in proofs]),
              "fri_proof_sha256": u8(sha),
              "fri_proof_bytes": np.array(nbytes, dtype=np.float64),
              "fri_proof_sample": np.stack(sample).astype(np.float64),
              "fri_proof_sample_index": idx.astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def profile_is_current(round_tag):
    """True if the committed counter files of `round_tag` were taken from the kernel source this run uses (profiles/<round>_profile_meta.json, written by
    tools/process_profiles.py); None if there is no record.  A kernel change without re-profiling keeps stale instruction / traffic constants: say so."""
    import hashlib
    meta = os.path.join(ROOT, "profiles", round_tag + "_profile_meta.json")
    if not os.path.exists(meta):
        return None
    try:
        m = json.load(open(meta))
        h = hashlib.sha256()
        for fn in m["files"]:
            h.update(open(os.path.join(ROOT, "mini-stark_amd", "csrc", fn), "rb").read())
        return h.hexdigest() == m["kernel_source_sha256"]
    except Exception:
        return None


def load_sq_profile():
    """VALU wave-instructions per thread per (kernel, grid) from this round's rocprofv3 SQ-counter pass (tools/process_profiles.py)."""
    for name in ("r05_sq_counters_top_kernels.csv", "r04_sq_counters_top_kernels.csv"):
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            rows = list(csv.DictReader(open(path)))
            return name, rows
    return None, []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--log-rows", type=int, default=20, help="log2 of trace rows (BASELINE configs[1]: 20)")
    ap.add_argument("--blowup", type=int, default=8)
    ap.add_argument("--field", type=int, default=0, help="0 Goldilocks, 1 BabyBear")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra legs (2^24 rows, BabyBear, NTT-only, I/O-inclusive) of the N = 1 run")
    ap.add_argument("--no-cpu-2p24", action="store_true", help="skip the CPU baseline's second sample: one 2^24-row proof (the size north_star's >= 10x target is stated on) on the "
                                                              "oracle with OpenMP, ~2-3 minutes of host time (cpu_baseline.at_2p24)")
    ap.add_argument("--cpu-log-rows", type=int, default=20, help="size of the CPU baseline's sample proof (default: the benchmark size itself, no extrapolation)")
    ap.add_argument("--inflight", type=int, default=None, help="independent proofs in flight per GPU (one ms_ctx + HIP stream each); a step = this many proofs (default: 8 up to 2^20 rows, fewer above)")
    ap.add_argument("--mode", choices=["replicas", "shard"], default="replicas",
                    help="replicas (default): every rank proves its own traces, no data-path collective (weak scaling); with N > 1 ranks a sharded 2^24-row proof is "
                         "measured as a second leg.  shard: ONE proof per step computed by all ranks together is the timed step (strong scaling)")
    ap.add_argument("--shard-log-rows", type=int, default=24, help="size of the sharded leg's proof (BASELINE configs[3]: 24)")
    ap.add_argument("--shard-steps", type=int, default=3)
    ap.add_argument("--no-shard-leg", action="store_true")
    ap.add_argument("--shard-timeout", type=float, default=240.0, help="time limit of the sharded leg's child processes (seconds)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="nccl = RCCL, one GPU per rank (the measured configuration).  gloo: rehearsal of the N>1 paths on a box with fewer GPUs than ranks "
                         "(ranks share GPUs, exchange payloads are staged through host memory)")
    ap.add_argument("--emu", action="store_true", help="REHEARSAL on the CPU: the kernel-emulation build of the same source (tests/emu) instead of the HIP library, host memory "
                                                    "instead of HBM, backend gloo; exercises the launcher, the rank plumbing and the sharded leg's exchange without a GPU.  Timings are meaningless")
    ap.add_argument("--no-shard-check", action="store_true", help="sharded leg: skip rank 0's unsharded proof of the same trace (matches_unsharded)")
    ap.add_argument("--launch-timeout", type=float, default=1500.0, help="time limit of the self-launched ranks (--gpus N > 1 without torchrun), seconds")
    ap.add_argument("--full", action="store_true", help="also run every leg beside the headline: roofline (one profiled proof), the N = 1 extras, the CPU baseline and, "
                                                     "with N > 1, the sharded proof (--mode shard: its profiled, per-stage and unsharded proofs).  Without it a run times the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the proofs of the last step (rank 0) as DIR/<name>.npy, float64: see dump_outputs")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.emu:
        args.backend = "gloo"
    # --gpus N > 1 started as a plain `python bench.py` (no torchrun, WORLD_SIZE unset): this process becomes the launcher of N ranks
    # and never touches the GPU itself.  Under torchrun (WORLD_SIZE set) the process IS one rank.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args, sys.argv[1:])
        return
    if args.gpus != int(os.environ.get("WORLD_SIZE", "1")):
        print(f"[bench] --gpus {args.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE', '1')}: the launcher's world size wins", file=sys.stderr, flush=True)

    import numpy as np
    import torch
    import mini_stark_amd as ms
    from mini_stark_amd.dist import Group
    grp = Group(args.backend)
    world, rank, local_rank, dev = grp.world, grp.rank, grp.local_rank, grp.device
    lib = lib_path_for(args)
    if args.emu:
        local_rank, dev = 0, torch.device("cpu")
    elif args.backend == "gloo":
        local_rank = local_rank % max(1, torch.cuda.device_count())
        dev = torch.device("cuda", local_rank)
    launched = os.environ.get("MS_BENCH_LAUNCHED") == "1"   # a rank of bench.py's own launcher: the parent runs the sharded leg as a second wave
    if args.inflight is None:
        args.inflight = default_inflight(args.log_rows)
    field_name = "Goldilocks" if args.field == 0 else "BabyBear+Fp4"
    out = None

    if args.mode == "shard" and world > 1:
        res, cfg = sharded_leg(args, grp, local_rank, args.log_rows, args.steps, args.warmup)
        out = {"metric": "stark_proofs_per_s", "value": res["value"], "unit": "proofs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": res["ms_per_proof"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u64" if args.field == 0 else "u32",
               "data": "synthetic", "config": {"workload": res["workload"], "proofs_per_step_per_gpu": 1.0 / world, "parallelism": res["parallelism"]}, "exchange": res}
        if rank == 0:
            print(json.dumps(out), flush=True)
        grp.close()
        return

    # ---- headline leg: independent proofs on every rank
    lanes = Lanes(args.field, args.log_rows, args.blowup, max(1, args.inflight), local_rank, dev, seed0=2 + rank * max(1, args.inflight), lib=lib)
    cfg, C_IN = lanes.cfg, lanes.n
    if os.environ.get("MS_BENCH_DUMP_MAPS"):   # diagnostics: the process's mappings once every library is loaded (names the address ranges of a native stack trace)
        with open(os.environ["MS_BENCH_DUMP_MAPS"], "w") as f:
            f.write(open("/proc/self/maps").read())
    elapsed = lanes.timed(grp, args.steps, args.warmup)
    final_roots = grp.all_gather_bytes(lanes.last[0].fri_roots[-1])  # every rank finished a proof (outside the timed region)
    assert len(final_roots) == world
    if args.dump_outputs and rank == 0:   # the FRI proofs were left in HBM by the timed proofs: read back here, outside the timed region
        dump_outputs(args.dump_outputs, lanes.last, (c.fri_proof_read() for c in lanes.ctxs))
    out = {
        "metric": "stark_proofs_per_s", "value": world * args.steps * C_IN / elapsed, "unit": "proofs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u64" if args.field == 0 else "u32", "data": "synthetic",
        "config": {"workload": f"Fibonacci AIR, {field_name}, 2^{args.log_rows} trace rows, blowup {args.blowup}, 20 security bits "
                               f"(w=3, c=6, rounds={cfg.rounds}, ood_queries={cfg.constrain_queries}, fri_queries={cfg.fri_queries}); a step = {C_IN} independent proofs in flight per GPU",
                   "proofs_per_step_per_gpu": C_IN, "parallelism": f"replicas x{world} GPUs x {C_IN} in-flight proofs (no data-path collective; the lanes of a GPU start {lanes.stagger_ms:g} ms apart, inside the timed region)"},
    }

    # ---- N > 1: the sharded proof of BASELINE configs[3] as a second leg.  It runs in a CHILD process per rank (this script in --mode shard,
    # its own rendezvous on MASTER_PORT + 1): the RCCL path inside the library has never run on more than one GPU, and neither a hang
    # (subprocess timeout) nor a crash of it may take the headline down.
    if args.emu:
        out["emulation"] = "REHEARSAL: CPU emulation build of the kernel source, host memory, gloo - exercises launcher / rank plumbing / exchange only; timings are meaningless"
    if world > 1 and args.full and not args.no_shard_leg and not launched:
        import subprocess
        lanes.close()
        lanes = None
        if not args.emu:
            torch.cuda.empty_cache()
        if rank == 0:   # stderr only (stdout carries exactly one JSON line)
            print(f"[bench] replicas leg done: {out['value']:.2f} proofs/s on {world} GPUs; starting the sharded leg in child processes", file=sys.stderr, flush=True)
        grp.barrier()
        env = dict(os.environ)
        env["MASTER_PORT"] = str(int(os.environ.get("MASTER_PORT", "29500")) + 1)
        env.pop("TORCHELASTIC_USE_AGENT_STORE", None)   # torchrun's workers use the agent's store on MASTER_PORT; the children host their own on the next port
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--mode", "shard", "--log-rows", str(args.shard_log_rows), "--steps", str(args.shard_steps),
               "--warmup", "1", "--backend", args.backend, "--field", str(args.field), "--blowup", str(args.blowup), "--no-cpu-baseline", "--no-extras", "--full"] + (["--emu"] if args.emu else [])
        try:
            cp = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.shard_timeout)
            lines = [l for l in cp.stdout.splitlines() if l.startswith("{")]
            if rank == 0:
                if cp.returncode == 0 and lines:
                    out["sharded"] = json.loads(lines[-1])["exchange"]
                else:
                    out["sharded"] = {"error": f"sharded leg exited with code {cp.returncode}; headline unaffected", "stderr_tail": cp.stderr[-600:]}
        except subprocess.TimeoutExpired:
            if rank == 0:
                out["sharded"] = {"error": f"the sharded leg did not finish within {args.shard_timeout:.0f} s; headline unaffected"}
        except Exception as e:  # noqa: BLE001 - reported in the JSON line
            if rank == 0:
                out["sharded"] = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0 and (args.emu or not args.full):
        print(json.dumps(out), flush=True)
    elif rank == 0:
        if lanes is None:
            lanes = Lanes(args.field, args.log_rows, args.blowup, 1, local_rank, dev)
        ctx = lanes.ctxs[0]
        # ---- roofline leg: per-kernel HIP events on the launching stream, one extra (untimed) proof
        buf = C.create_string_buffer(1 << 15)
        ctx.check(ctx.L.ms_profile_begin(ctx.h))
        lanes._prove_n(0, 1)
        ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
        prof = json.loads(buf.value.decode())
        prof.pop("shard", None)
        variants = prof.pop("ntt_pass_variants")
        # the NTT pass template instance with the largest total time in one proof = "the dominant HBM-class kernel"
        kname, k = max(variants.items(), key=lambda kv: kv[1]["ms"])
        avg_ms = k["ms"] / max(1, k["launches"])
        achieved = (k["alg_bytes"] / max(1, k["launches"])) / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
        traffic, traffic_src, pmc_variants = None, None, {}
        for name in ("r05_pmc_ntt_pass.json", "r04_pmc_ntt_pass.json"):
            pmc = os.path.join(ROOT, "profiles", name)
            if os.path.exists(pmc):
                try:
                    pj = json.load(open(pmc))
                    pmc_variants = pj.get("variants", {})
                    if pj.get("kernel") == kname:
                        traffic, traffic_src = pj.get("hbm_bytes_per_launch"), "profiles/" + name
                        break
                except Exception:
                    pass
        per_variant = {}
        for vn, v in variants.items():   # every NTT pass template instance of the proof: live time, algorithmic rate, PMC traffic (constant from the profile) on the live time
            a_ms = v["ms"] / max(1, v["launches"])
            tb = pmc_variants.get(vn, {}).get("hbm_bytes_per_launch")
            per_variant[vn] = {"launches_per_proof": v["launches"], "avg_launch_ms": a_ms, "alg_GBps": (v["alg_bytes"] / max(1, v["launches"])) / (a_ms * 1e-3) / 1e9 if a_ms else 0.0,
                               "traffic_bytes_per_launch": tb, "frac_of_hbm_peak_on_traffic": (tb / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if tb and a_ms else None}
        allp = prof["ntt_pass"]
        out["roofline"] = {"kernel": kname, "bound": "hbm", "limited_by": "valu_issue+access_pattern", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                           "traffic": traffic, "traffic_source": (traffic_src + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, gfx950 corrections applied; a constant, not measured in this run)") if traffic_src else None,
                           "traffic_profile_taken_from_this_kernel_source": profile_is_current(traffic_src.split("/")[1][:3]) if traffic_src else None,
                           "frac_on_traffic": (traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic and avg_ms > 0 else None,
                           "launches_per_proof": k["launches"], "avg_launch_ms": avg_ms, "alg_bytes_per_launch": k["alg_bytes"] / max(1, k["launches"]),
                           "variants": per_variant,
                           "all_ntt_pass_kernels": {"launches_per_proof": allp["launches"], "ms_per_proof": allp["ms"],
                                                    "alg_GBps": allp["alg_bytes"] / (allp["ms"] * 1e-3) / 1e9 if allp["ms"] else 0.0},
                           "note": "these passes are not bound by HBM (a column resident in the Infinity Cache or an LDS-DMA prefetch of the next tile changes nothing: profiles/HISTORY.md) but by how fast 4 waves per SIMD get "
                                   "through 64-bit modular arithmetic on 32-bit lanes: SQ counters (profiles/r04_sq_counters_ntt_passes.txt; same kernels as r03) give 79 / 113-125 VALU instructions per element (later / first pass; 96 / 139 in r02) "
                                   "and 0.65 scalar instructions per vector one, issued at one VALU instruction per SIMD per ~9 clocks; DESIGN.md 6.2"}
        tot = sum(v["ms"] for v in prof.values()) or 1.0
        out["kernel_ms_per_proof"] = {n: round(v["ms"], 4) for n, v in prof.items() if v["launches"]}
        out["kernel_ms_total_single_proof"] = tot
        sha = prof["leaf_hash"]["ms"] + prof["inner_hash"]["ms"]
        out["sha256_share_of_kernel_time"] = sha / tot

        # ---- VALU roofline of the SHA-256 kernels: wave-instructions issued per second against the issue peak
        sq_name, sq = load_sq_profile()
        if sq and args.log_rows == 20 and args.field == 0:
            def wave_instr(prefixes):   # per proof: sum over the profiled (kernel, grid) pairs of the class
                t = 0.0
                for r in sq:
                    if any(r["kernel"].startswith(p) for p in prefixes):
                        t += float(r["dispatches"]) / float(r.get("proofs_profiled", 2) or 2) * float(r["grid_threads"]) / 64.0 * float(r["valu_wave_instr_per_thread"])
                return t
            peak_guide = N_SIMD * CLOCK_HZ / 2.0      # SIMD-32: a wave64 VALU instruction occupies the SIMD for 2 cycles
            peak_meas = N_SIMD * CLOCK_HZ / 3.4       # measured: 3.3-3.6 cycles per VALU instruction in register-resident integer code (tools/ntt_lab.hip, r02)
            rv = {}
            for cls, prefixes in (("leaf_hash", ("msmerkle::LeafHashKernel", "msmerkle::PadOnlyBlockKernel")), ("inner_hash", ("msmerkle::InnerHashKernelT", "msmerkle::InnerSubtreeKernel"))):
                wi = wave_instr(prefixes)
                ms_cls = prof[cls]["ms"]
                if wi and ms_cls:
                    rate = wi / (ms_cls * 1e-3)
                    rv[cls] = {"valu_wave_instr_per_proof": wi, "ms_per_proof": ms_cls, "achieved_wave_instr_per_s": rate,
                               "frac_of_guide_peak": rate / peak_guide, "frac_of_measured_issue_peak": rate / peak_meas}
            # the whole proof against the same peaks: every profiled kernel's VALU instructions x the headline rate (8 proofs in flight keep the VALU fed)
            wi_all = wave_instr(("",))
            peak_quad = N_SIMD * 2.2e9 / 4.0          # one wave64 instruction per SIMD per 4 clocks at the 2.2 GHz the chip holds under these kernels
            big = [r for r in sq if r["kernel"].startswith("msmerkle::LeafHashKernel<GL; 1")]
            big = max(big, key=lambda r: float(r["grid_threads"])) if big else None
            rate_all = wi_all * (args.steps * C_IN / elapsed) if wi_all else 0.0
            whole = {"valu_wave_instr_per_proof": wi_all, "achieved_wave_instr_per_s": rate_all, "frac_of_guide_peak": rate_all / peak_guide,
                     "frac_of_measured_issue_peak": rate_all / peak_meas, "frac_of_quad_cycle_peak": rate_all / peak_quad,
                     "note": "the profiled kernels' SQ_INSTS_VALU per proof x the headline proofs/s of THIS run (per GPU): the prover as a whole is bound by the number of VALU "
                             "instructions it issues, 84 % of them SHA-256"}
            if big:
                r1 = float(big["grid_threads"]) / 64.0 * float(big["valu_wave_instr_per_thread"]) / (float(big["avg_us"]) * 1e-6)
                whole["largest_leaf_launch"] = {"wave_instr_per_s": r1, "frac_of_quad_cycle_peak": r1 / peak_quad, "source": "profiles/" + sq_name + " (LDE leaf hashing: grid, instructions per thread and duration of the profiled run)"}
            peak_lab = N_SIMD * 2.2e9 / 3.65          # tools/sha_lab.hip (profiles/r04_sha_lab.log): the same compression code on registers only, 4-8 waves/SIMD: 3.5-3.8 clocks per instruction
            for v in rv.values():
                v["frac_of_sha_lab_rate"] = v["achieved_wave_instr_per_s"] / peak_lab
            whole["frac_of_sha_lab_rate"] = rate_all / peak_lab
            if big:
                whole["largest_leaf_launch"]["frac_of_sha_lab_rate"] = whole["largest_leaf_launch"]["wave_instr_per_s"] / peak_lab
            out["roofline_valu"] = {"bound": "valu_issue", "unit": "wave-instr/s", "peak_guide": peak_guide, "whole_proof": whole, "peak_sha_lab": peak_lab,
                                    "peak_sha_lab_basis": "tools/sha_lab.hip: the compression function of csrc/merkle.hpp on register-resident data (no memory) issues one instruction per 3.5-3.8 clocks per SIMD at 4-8 waves "
                                    "(28.5 G compressions/s chip-wide at 8 waves/SIMD, 26.4 at the leaf kernel's 4): the practical VALU ceiling of SHA-256 on this chip",
                                    "peak_quad_cycle": peak_quad, "peak_quad_cycle_basis": "one wave64 VALU instruction per SIMD per 4 clocks, 1024 SIMDs, 2.2 GHz (the clock rocprofv3 GRBM_GUI_ACTIVE shows under the hash kernels): "
                                    "the issue rate of the carry / 64-bit / rotate / multiply / v_add3 class (tools/valu_rate.hip; simple 32-bit operations issue at ~2.5 cycles) and the average the large SHA-256 launches reach (96 %)", "peak_guide_basis": "MI355X_MICROARCH.md: 4 SIMD-32 per CU, a wave64 VALU op = 2 cycles, 2.4 GHz",
                                    "peak_measured": peak_meas, "peak_measured_basis": "3.4 cycles per VALU instruction: what register-resident integer butterfly code sustains at >= 4 waves/SIMD whatever the opcode mix "
                                    "(tools/ntt_lab.hip, profiles/r04_ntt_lab.log); the per-opcode costs of tools/valu_rate.hip did not carry over to mixed code",
                                    "instr_source": "profiles/" + sq_name + " (rocprofv3 --pmc SQ_INSTS_VALU per dispatch; constants, not measured in this run)",
                                    "instr_profile_taken_from_this_kernel_source": profile_is_current(sq_name[:3]),
                                    "times": "live: HIP events of this run, one proof alone (small tree levels are latency-bound, which lowers the class average)", "kernels": rv}

        # ---- what actually bounds the proof: the kernel class with the largest share of a proof's kernel time, priced on the roofline of ITS class.
        # `roofline` above stays the NTT object the metric names (NTT GB/s against HBM); this is the one a reader should take for "how close to the hardware is the prover"
        classes = {n: v["ms"] for n, v in prof.items() if isinstance(v, dict) and v.get("launches")}
        dom = max(classes, key=classes.get) if classes else None
        if dom:
            rd = {"kernel_class": dom, "share_of_kernel_time": classes[dom] / tot, "ms_per_proof": classes[dom], "launches_per_proof": prof[dom]["launches"],
                  "sha256_classes_share_of_kernel_time": sha / tot,
                  "kernels": {"leaf_hash": "msmerkle::LeafHashKernel<F, E> + PadOnlyBlockKernel (csrc/merkle.hpp)", "inner_hash": "msmerkle::InnerHashKernelT<2> + InnerSubtreeKernel (csrc/merkle.hpp)"}.get(dom, dom)}
            rvd = out.get("roofline_valu", {}).get("kernels", {}).get(dom)
            if rvd:   # a SHA-256 class: 32-bit VALU issue is the roofline
                rv_all = out["roofline_valu"]
                rd.update({"bound": "valu_issue", "unit": "wave-instr/s", "achieved": rvd["achieved_wave_instr_per_s"], "peak": rv_all["peak_guide"], "frac": rvd["frac_of_guide_peak"],
                           "peak_source": "MI355X_MICROARCH.md: a wave64 VALU instruction occupies a SIMD-32 for 2 cycles; 1024 SIMDs x 2.4 GHz / 2",
                           "valu_wave_instr_per_proof": rvd["valu_wave_instr_per_proof"], "instr_source": rv_all["instr_source"],
                           "instr_profile_taken_from_this_kernel_source": rv_all["instr_profile_taken_from_this_kernel_source"],
                           "measured_ceiling": rv_all["peak_sha_lab"], "frac_of_measured_ceiling": rvd["frac_of_sha_lab_rate"], "measured_ceiling_source": rv_all["peak_sha_lab_basis"],
                           "largest_launch": rv_all["whole_proof"].get("largest_leaf_launch") if dom == "leaf_hash" else None,
                           "whole_proof_at_headline_rate": {k: rv_all["whole_proof"][k] for k in ("achieved_wave_instr_per_s", "frac_of_guide_peak", "frac_of_sha_lab_rate") if k in rv_all["whole_proof"]},
                           "times": "live (HIP events of this run, one proof alone); instruction counts: constants from the committed rocprofv3 SQ_INSTS_VALU pass"})
            else:
                rd.update({"bound": "hbm", "unit": "GB/s", "achieved": prof[dom]["alg_bytes"] / (classes[dom] * 1e-3) / 1e9 if prof[dom].get("alg_bytes") else None, "peak": HBM_PEAK_GBS})
                rd["frac"] = rd["achieved"] / HBM_PEAK_GBS if rd["achieved"] else None
            out["roofline_dominant"] = rd

        if world == 1 and not args.no_extras and args.log_rows == 20 and args.field == 0:
            lanes.close()
            lanes = None
            extra = {}

            def leg(name, fn):
                try:
                    extra[name] = fn()
                except Exception as e:  # noqa: BLE001 - an extra leg must not take the headline down
                    extra[name] = {"error": f"{type(e).__name__}: {e}"}

            def proofs_leg(field, log_rows, steps, warmup, inflight=None, io=False, io_mode="async", copies=None, flags=None):
                infl = inflight or default_inflight(log_rows)
                if copies:   # "hip": the boundary's bulk copies by the HIP runtime (hipMemcpyAsync) instead of the SDMA engines - read at ms_create
                    os.environ["MS_READBACK"], os.environ["MS_UPLOAD"] = copies, copies
                try:
                    ln = Lanes(field, log_rows, args.blowup, infl, local_rank, dev, io=io, io_mode=io_mode, flags=flags)
                finally:
                    if copies:
                        del os.environ["MS_READBACK"], os.environ["MS_UPLOAD"]
                el = ln.timed(grp, steps, warmup)
                lat = None
                if not io:
                    t0 = time.perf_counter(); ln._prove_n(0, 2); lat = (time.perf_counter() - t0) / 2 * 1e3
                r = {"value": steps * infl / el, "unit": "proofs/s", "ms_per_proof_in_flight": el / (steps * infl) * 1e3, "in_flight": infl, "steps": steps, "rounds": ln.cfg.rounds}
                if lat is not None:
                    r["ms_single_proof_latency"] = lat
                if io:   # every lane proves the same trace over and over: one distinct non-zero sample per lane = every proof arrived whole
                    r["every_proof_sampled_on_host"] = all(len(sm) == 1 and 0 not in sm for sm in ln.samples)
                    r["readback_engine"] = {0: "hipMemcpyAsync (HIP runtime)", 1: "SDMA engine (hsa_amd_memory_async_copy_on_engine)"}.get(ln.ctxs[0].L.ms_io_engine(ln.ctxs[0].h), "?")
                ln.close()
                return r
            leg("goldilocks_2p24_rows", lambda: dict(proofs_leg(0, 24, 4, 1), workload="BASELINE configs[3] per GPU: Fibonacci AIR, Goldilocks, 2^24 rows, blowup 8 (L = 2^27, ~25 GiB resident per proof)"))
            leg("babybear_fp4_2p20_rows", lambda: dict(proofs_leg(1, 20, 10, 2), workload="BASELINE configs[2]: Fibonacci AIR, BabyBear + quartic extension, 2^20 rows, blowup 8 (u32 storage)"))
            leg("value_with_io", lambda: dict(proofs_leg(0, 20, 20, 2, io=True, io_mode="async"), workload="configs[1] with the boundary's I/O inside the timed region: every proof uploads its 24 MiB trace "
                                              "from page-locked host memory and its ~64 MiB FRI proof is copied into page-locked host memory by ms_fri_proof_read_async while proof k + 1 starts - both on SDMA "
                                              "engines through the HSA runtime (r04; no blit kernels); the host mirror keeps two proof slots, proof k is touched on the host (one word per page) after prove k + 1 "
                                              "returned, every read-back finished inside the timed region"))
            def io_paired():
                # the two rates whose RATIO is the claim, measured against each other: both sets of lanes alive, timed runs alternating (3 x [resident, with I/O], 10 steps each) -
                # legs that run minutes apart differ by +-1-2 % on their own (the modes flipped sign between runs)
                a = Lanes(0, 20, args.blowup, 8, local_rank, dev)
                b = Lanes(0, 20, args.blowup, 8, local_rank, dev, io=True, io_mode="async")
                ra, rb = [], []
                for _ in range(3):
                    ra.append(10 * 8 / a.timed(grp, 10, 1))
                    rb.append(10 * 8 / b.timed(grp, 10, 1))
                ok = all(len(sm) == 1 and 0 not in sm for sm in b.samples)
                eng = b.ctxs[0].L.ms_io_engine(b.ctxs[0].h)
                a.close(); b.close()
                med = lambda v: sorted(v)[len(v) // 2]
                return {"resident": med(ra), "with_io": med(rb), "ratio": med(rb) / med(ra), "passes_resident": ra, "passes_with_io": rb, "every_proof_sampled_on_host": ok,
                        "readback_on_sdma_engine": eng == 1, "unit": "proofs/s", "workload": "configs[1], 8 lanes: resident vs trace upload + FRI proof read-back (asynchronous) in the timed region, alternated"}
            leg("io_paired", io_paired)
            leg("value_with_io_blocking_readback", lambda: dict(proofs_leg(0, 20, 20, 2, io=True, io_mode=True), workload="the same with a blocking ms_fri_proof_read at the end of every proof (SDMA engine too)"))
            leg("value_with_io_hip_copies", lambda: dict(proofs_leg(0, 20, 20, 2, io=True, io_mode="async", copies="hip"), workload="the same as value_with_io with MS_UPLOAD=hip MS_READBACK=hip: both copies by the "
                                              "HIP runtime's hipMemcpyAsync (r03's path: part of them runs as blit kernels that take issue slots from the provers)"))
            leg("value_with_io_kernels_write_host", lambda: dict(proofs_leg(0, 20, 10, 2, io=True, io_mode="into"), workload="the same with ms_fri_query_into: the query-phase kernels store the FRI proof straight into "
                                              "page-locked host memory (no copy).  Measured r03: SLOWER (the 64 MiB cross PCIe as stores of kernels whose waves hold their CUs meanwhile; coherent or non-coherent "
                                              "pinned memory alike) - kept as an API for device-memory destinations, not used as the read-back path"))
            import mini_stark_amd as _ms
            leg("single_proof", lambda: dict(proofs_leg(0, 20, 30, 4, inflight=1, flags=_ms.FLAG_ZERO_DISPLAY_EMPTY | _ms.FLAG_LATENCY),
                                             workload="configs[1] with ONE proof in flight, context created with MS_FLAG_LATENCY (the latency configuration: a FRI round's coefficient side on a side "
                                                      "stream beside its evaluation side): 1 / value = the time of one Stark::prove"))
            leg("single_proof_default_flags", lambda: dict(proofs_leg(0, 20, 30, 4, inflight=1), workload="the same without MS_FLAG_LATENCY (the throughput configuration, one lane)"))

            def wide_air():
                # BASELINE configs[4] on one GPU: 64 trace columns + 64 transition polynomials (c = 128), Goldilocks, 2^22 rows, blowup 8; linear transitions
                # (degree-3 constraints are not expressible in the reference: quirk Q1); challenges from SplitMix64; one proof in flight, trace resident in HBM
                from mini_stark_amd.synthetic import SplitMix64
                P, lr, w = 2**64 - 2**32 + 1, 22, 64
                N = 1 << lr
                rs = np.random.RandomState(7)
                d_tr = torch.from_numpy((rs.randint(0, 2**62, size=(N, w), dtype=np.int64))).to(dev)   # < 2^62 < p: canonical
                c2 = ms.Context(0, device=local_rank)
                rng = SplitMix64(5)
                combos = [([rng.next() % P or 1, rng.next() % P, P - 1], [j, (j + 1) % w, (j + 7) % w]) for j in range(w)]
                rounds = lr + 3

                def one():
                    r2 = SplitMix64(6)
                    c2.check(c2.trace_commit_device(d_tr.data_ptr(), N, w, 2 * w)[0]); c2.check(c2.interpolate())
                    for sc, idx in combos:
                        c2.check(c2.polys_lincomb(sc, idx))
                    c2.check(c2.lde_commit(args.blowup, r2.next() % P or 3, 2 * w)[0]); c2.check(c2.mix(r2.next() % P))
                    c2.check(c2.eval_ext(np.array([r2.next() % P, r2.next() % P], dtype=np.uint64))[0])
                    c2.check(c2.fri_begin(args.blowup, rounds)[0])
                    for _ in range(1, rounds):
                        c2.check(c2.fri_deep([r2.next() % P, r2.next() % P])[0]); c2.check(c2.fri_fold_commit([r2.next() % P, r2.next() % P])[0])
                    c2.check(c2.fri_query([r2.next()], read=False)[0])
                one()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2):
                    one()
                c2.synchronize()
                el = (time.perf_counter() - t0) / 2
                c2.close()
                return {"value": 1.0 / el, "unit": "proofs/s", "ms_per_proof": el * 1e3, "in_flight": 1, "steps": 2, "rounds": rounds,
                        "workload": "BASELINE configs[4] per GPU: wide synthetic AIR, 64 trace columns + 64 linear transition polynomials (c = 128), Goldilocks, 2^22 rows, blowup 8 "
                                    "(32 GiB LDE matrix, 2^25 leaf messages of ~2.5 KB)"}
            leg("wide_air_2p22", wide_air)

            def wide_air_cubic():
                # BASELINE configs[4] AS WRITTEN - "64 trace columns, degree-3 constraints" - in the build-defined form the reference cannot express (quirk Q1): 64 transitions
                # col_j' = col_j col_{j+1} col_{j+2} + s_j col_{j+3}, composed with the TRUE quotient by x^N - 1 on the committed LDE domain (ms_mix_cubic); the LDE commits the
                # 64 trace polynomials, the DEEP-ALI opening is at z and w z, FRI runs over the 2N-coefficient validity polynomial.  Self-verified (no reference to compare with).
                from mini_stark_amd.host import cubic_rows_native
                from mini_stark_amd.synthetic import SplitMix64
                P, lr, w = 2**64 - 2**32 + 1, 22, 64
                N = 1 << lr
                tr, sc = cubic_rows_native(P, N, w, 9)
                d_tr = torch.from_numpy(tr.view(np.int64)).to(dev)
                spec = [(j, j, (j + 1) % w, (j + 2) % w, (j + 3) % w) for j in range(w)]
                c2 = ms.Context(0, device=local_rank)
                omega = c2.root_of_unity(N)
                rounds = lr + 1 + 3     # log2(2N * blowup)

                def one():
                    r2 = SplitMix64(6)
                    c2.check(c2.trace_commit_device(d_tr.data_ptr(), N, w, w)[0]); c2.check(c2.interpolate())
                    c2.check(c2.lde_commit(args.blowup, r2.next() % P or 3, w)[0])
                    c2.check(c2.mix_cubic(r2.next() % P, spec, sc))
                    z = [r2.next() % P, r2.next() % P]
                    wz = [z[0] * omega % P, z[1] * omega % P]     # (z0 + z1 u) * w, w in the base field
                    c2.check(c2.eval_ext(np.array([z, wz], dtype=np.uint64))[0])
                    c2.check(c2.fri_begin(args.blowup, rounds)[0])
                    for _ in range(1, rounds):
                        c2.check(c2.fri_deep([r2.next() % P, r2.next() % P])[0]); c2.check(c2.fri_fold_commit([r2.next() % P, r2.next() % P])[0])
                    c2.check(c2.fri_query([r2.next()], read=False)[0])
                one()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2):
                    one()
                c2.synchronize()
                el = (time.perf_counter() - t0) / 2
                c2.close()
                return {"value": 1.0 / el, "unit": "proofs/s", "ms_per_proof": el * 1e3, "in_flight": 1, "steps": 2, "rounds": rounds,
                        "workload": "BASELINE configs[4] as written, build-defined (the reference cannot express it): wide AIR, 64 trace columns, 64 DEGREE-3 transition constraints, Goldilocks, "
                                    "2^22 rows, blowup 8; true quotient by x^N - 1 (ms_mix_cubic), DEEP-ALI at z and w z, FRI over the 2N-coefficient validity polynomial (rounds 26)"}
            leg("wide_air_cubic_2p22", wide_air_cubic)

            def ntt_only():
                res = {}
                os.environ["MS_LDE_LINEAR"] = "0"   # six transforms (no linear-provenance shortcut): the kernel measurement
                try:
                    from mini_stark_amd.stark import fibonacci_air
                    stream = torch.cuda.Stream(device=dev)
                    for fld, lr, reps in ((0, 20, 20), (0, 24, 3), (1, 20, 20), (1, 22, 8)):
                        c2 = ms.Context(fld, device=local_rank)
                        c2.set_stream(stream.cuda_stream)
                        tt = fibonacci_air(c2, (1 << lr) - 1)
                        with torch.cuda.stream(stream):
                            c2.check(c2.trace_commit(tt.data, 6)[0]); c2.check(c2.interpolate())
                            for sc, idx in tt.transitions:
                                c2.check(c2.polys_lincomb(sc, idx))
                            c2.check(c2.bench_lde(args.blowup, 12345))
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            for _ in range(reps):
                                c2.check(c2.bench_lde(args.blowup, 12345))
                            e1.record(stream)
                        torch.cuda.synchronize()
                        ms_per = e0.elapsed_time(e1) / reps
                        sz = 8 if fld == 0 else 4            # bytes per base element as stored on the device
                        alg = 6 * ((1 << lr) + (1 << lr) * args.blowup) * sz
                        res[("" if fld == 0 else "babybear_") + f"coset_lde_6x2^{lr}_to_2^{lr + 3}"] = {
                            "ms": ms_per, "alg_GBps": alg / ms_per / 1e6, "frac_of_hbm_peak": alg / ms_per / 1e6 / HBM_PEAK_GBS, "alg_bytes": alg, "element_bytes": sz,
                            "what": "scale + NTT passes of six columns, device resident, HIP events on the launching stream"}
                        c2.close()
                finally:
                    del os.environ["MS_LDE_LINEAR"]
                return res
            leg("ntt_only", ntt_only)
            out["extra"] = extra
            vio = extra.get("value_with_io", {}).get("value")
            if vio:   # the contract keeps `value` = traces resident in HBM (the PCIe-inclusive rate is never `value`); it is reported beside it
                out["value_with_io"] = vio
                out["value_with_io_over_value"] = vio / out["value"]
                pr = extra.get("io_paired", {})
                if pr.get("ratio"):   # the same ratio from legs measured against each other (alternating): the figure to quote
                    out["value_with_io_over_value_paired"] = pr["ratio"]

        # ---- CPU baseline leg (N == 1): oracle "port" on the benchmark proof itself, single thread + OpenMP
        if world == 1 and not args.no_cpu_baseline:
            if lanes is not None:
                lanes.close()
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import parity_cases as pc
            from common import fibonacci_trace_fast
            from oracle import oracle as orc
            cl = min(args.cpu_log_rows, args.log_rows)
            tr = fibonacci_trace_fast(args.field, 1 << cl)
            c0 = time.perf_counter()
            pc.drive(orc.Session(args.field), args.field, tr, args.blowup, max(0, cfg.fri_queries - 2), seed=1, q_ood=cfg.constrain_queries, read_big=False)
            ct = time.perf_counter() - c0
            scale = float(1 << (args.log_rows - cl))
            try:
                cpu_model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
            except Exception:
                cpu_model = "unknown"
            out["cpu_baseline"] = {"value": 1.0 / (ct * scale), "unit": "proofs/s", "cores": 1, "kind": "port", "cpu_model": cpu_model,
                                   "sample": f"one 2^{cl}-row proof of the same AIR on the oracle (oracle/ministark_oracle.cpp, 1 thread, Goldilocks multiply = one 64x64 product + special-form reduction, "
                                             f"at least as fast as arkworks' one-limb Montgomery) took {ct:.2f} s" + (f"; scaled linearly x{int(scale)}" if scale != 1 else " (the benchmark size itself: no extrapolation)")}
            ncpu = max(1, min(orc.max_threads(), len(os.sched_getaffinity(0))))
            best = None
            for nthr in sorted({t for t in (32, 64, ncpu) if 1 < t <= ncpu}):  # the port's fork-join loops stop scaling well before 128 threads: keep the best
                orc.set_threads(nthr)
                c0 = time.perf_counter()
                pc.drive(orc.Session(args.field), args.field, tr, args.blowup, max(0, cfg.fri_queries - 2), seed=1, q_ood=cfg.constrain_queries, read_big=False)
                ctm = time.perf_counter() - c0
                if best is None or ctm < best[0]:
                    best = (ctm, nthr)
            orc.set_threads(1)
            if best is not None:
                out["cpu_baseline"]["all_cores"] = {"value": 1.0 / (best[0] * scale), "unit": "proofs/s", "cores": best[1], "kind": "port", "host_cpus": ncpu,
                                                    "sample": f"same 2^{cl}-row proof with OpenMP x{best[1]} over the port's independent loops (best of the thread counts tried) took {best[0]:.2f} s"}
            # the size north_star states its >= 10x target on: ONE 2^24-row Goldilocks proof on the port with OpenMP (context for the reader; the ratio is not a quality claim)
            if not args.no_cpu_2p24 and args.field == 0 and args.log_rows == 20 and not args.no_extras:
                try:
                    from mini_stark_amd.host import fibonacci_rows_native
                    nthr = best[1] if best is not None else 1
                    orc.set_threads(nthr)
                    tr24 = fibonacci_rows_native(2**64 - 2**32 + 1, 1 << 24, (1 << 24) - 1)
                    c0 = time.perf_counter()
                    pc.drive(orc.Session(0), 0, tr24, args.blowup, 0, seed=1, q_ood=1, read_big=False, fixed_betas=(3,))   # rounds 27, 1 OOD query, 1 FRI query: StarkConfig at 2^24 rows
                    c24 = time.perf_counter() - c0
                    orc.set_threads(1)
                    gpu24 = (out.get("extra") or {}).get("goldilocks_2p24_rows", {}).get("value")
                    out["cpu_baseline"]["at_2p24"] = {"value": 1.0 / c24, "unit": "proofs/s", "cores": nthr, "kind": "port",
                                                      "sample": f"one 2^24-row Goldilocks proof (BASELINE configs[3] per GPU: rounds 27, 1 OOD query, 1 FRI query) on the oracle with OpenMP x{nthr} took {c24:.1f} s",
                                                      "gpu_same_size_proofs_per_s": gpu24, "gpu_over_cpu": (gpu24 * c24) if gpu24 else None}
                except Exception as e:  # noqa: BLE001 - a reported baseline must not take the line down
                    out["cpu_baseline"]["at_2p24"] = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps(out), flush=True)
    if lanes is not None:   # the contexts go before the process does (a second close of the same lanes is a no-op)
        lanes.close()
    grp.close()


if __name__ == "__main__":
    main()
