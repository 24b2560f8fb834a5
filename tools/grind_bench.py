#!/usr/bin/env python3
"""Proof-of-work grinding (ms_grind) on one GPU, in ONE process; prints one JSON line and writes profiles/grind.json.
  (a) hash rate per digest: ms_grind with 40 bits over 2^28 nonces (expected answer: MS_ERR_OUT_OF_RANGE; a hit - probability 2^-12 - takes the next seed), median
      of 8, beside the compression rate of the same digest's binary-tree level kernels measured in the same process: ms_merkle_commit of 2^23 leaf groups under
      ms_profile_begin / ms_profile_end, class inner_hash, nodes x compressions per node / kernel ms.
  (b) the duration of one launch of the default size (MS_GRIND_LAUNCH_MAX = 2^30 nonces) per digest.
  (c) the headline shape, one proof alone: 2^20-row Goldilocks Fibonacci AIR, blowup 8, 20 security bits, MS_FLAG_LATENCY, the FRI proof read back inside the timed
      region; grinding_bits 0 against 4, legs alternated; ms per proof, proof bytes, and the grind class's kernel ms.
Only the paired figures of one run mean anything.
  python3 tools/grind_bench.py [--log-rows 20] [--steps 10] [--passes 3] [--skip-proof] [--out profiles/grind.json]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def profile(ctx, fn):
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    fn()
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    return json.loads(buf.value.decode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10, help="proofs per leg of (c)")
    ap.add_argument("--passes", type=int, default=3, help="legs per setting of (c), alternated")
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--log-nonces", type=int, default=28, help="nonces of one search of (a)")
    ap.add_argument("--log-launch", type=int, default=30, help="nonces of the launch of (b)")
    ap.add_argument("--log-groups", type=int, default=23, help="leaf groups of the Merkle commitment of (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grind.json"))
    args = ap.parse_args()
    import hashlib
    import numpy as np
    import mini_stark_amd as ms
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    Z = ms.FLAG_ZERO_DISPLAY_EMPTY
    flags = {"sha256": Z, "blake2s": Z | ms.FLAG_DIGEST_BLAKE2S, "blake3": Z | ms.FLAG_DIGEST_BLAKE3, "keccak256": Z | ms.FLAG_DIGEST_KECCAK256, "sha3_256": Z | ms.FLAG_DIGEST_SHA3_256}
    per_node = {"sha256": 2, "blake2s": 1, "blake3": 1, "keccak256": 1, "sha3_256": 1}   # compressions (permutations) of one 64-byte inner node
    out = {"metric": "grind_bench", "unit": "G hashes/s", "hash_rate": {}, "inner_level_compression_rate": {}, "default_launch_ms": {}}
    leafs = (np.arange(2 << args.log_groups, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) % np.uint64(0xFFFFFFFF00000001)
    for name, f in flags.items():
        ctx = ms.Context(ms.GOLDILOCKS, flags=f)
        k, times = 0, []
        ctx.grind(hashlib.sha256(b"warm").digest(), 40, 0, 1 << min(24, args.log_nonces))
        while len(times) < 8:
            seed = hashlib.sha256(b"grind_bench/%d" % k).digest(); k += 1
            t0 = time.perf_counter(); rc, _ = ctx.grind(seed, 40, 0, 1 << args.log_nonces); dt = time.perf_counter() - t0
            if rc == ms.ERR_OUT_OF_RANGE:
                times.append(dt)
            elif rc != 0:
                ctx.check(rc)
        out["hash_rate"][name] = round((1 << args.log_nonces) / statistics.median(times) / 1e9, 3)
        t0 = time.perf_counter(); rc, _ = ctx.grind(hashlib.sha256(b"grind_bench/launch").digest(), 40, 0, 1 << args.log_launch); dt = time.perf_counter() - t0
        out["default_launch_ms"][name] = round(dt * 1e3, 2) if rc == ms.ERR_OUT_OF_RANGE else None
        root = (C.c_uint8 * 32)()
        call = lambda: ctx.check(ctx.L.ms_merkle_commit(ctx.h, leafs.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(leafs.size), C.c_int(1), C.c_size_t(2),   # noqa: E731
                                                        C.c_size_t(2), None, C.c_size_t(0), None, root))
        call()
        prof = profile(ctx, call)
        kms = prof["inner_hash"]["ms"]   # (0 on a build without event timing)
        out["inner_level_compression_rate"][name] = round(((1 << args.log_groups) - 1) * per_node[name] / (kms * 1e-3) / 1e9, 3) if kms > 0 else None
        ctx.close()
    if not args.skip_proof:
        ctx = ms.Context(ms.GOLDILOCKS, flags=Z | ms.FLAG_LATENCY)
        steps = (1 << args.log_rows) - 1
        tt = fibonacci_air(ctx, steps)
        hs = {b: HostStark(ctx, 20, 8, steps, tt.constrain_number(), grinding_bits=b) for b in (0, 4)}
        ms_per, nbytes, grind_ms = {0: [], 4: []}, {}, {}
        for b in (0, 4):
            for _ in range(2):
                ctx.check(hs[b].prove_raw(tt, read_fri_proof=True))
        for _ in range(args.passes):
            for b in (0, 4):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    ctx.check(hs[b].prove_raw(tt, read_fri_proof=True))
                ms_per[b].append((time.perf_counter() - t0) / args.steps * 1e3)
        for b in (0, 4):
            nbytes[b] = int(hs[b].H.msh_proof_serialize(hs[b].h, None, C.c_size_t(0)))
            prof = profile(ctx, lambda: ctx.check(hs[b].prove_raw(tt, read_fri_proof=True)))
            grind_ms[b] = round(prof.get("grind", {}).get("ms", 0.0), 4)
        mean = {b: sum(v) / len(v) for b, v in ms_per.items()}
        out["headline"] = {"workload": f"Fibonacci AIR, Goldilocks, 2^{args.log_rows} rows, blowup 8, 20 security bits, one proof alone (MS_FLAG_LATENCY), trace from host memory, "
                                       f"FRI proof read back inside the timed region, {args.steps} proofs per leg, legs alternated 0 / 4 grinding bits x {args.passes}",
                           "fri_queries": {str(b): hs[b].fri_queries for b in (0, 4)}, "ms_per_proof": {str(b): round(mean[b], 4) for b in (0, 4)},
                           "legs_ms": {str(b): [round(x, 4) for x in v] for b, v in ms_per.items()}, "proof_bytes": {str(b): nbytes[b] for b in (0, 4)},
                           "grind_kernel_ms": {str(b): grind_ms[b] for b in (0, 4)}, "ratio_ms_4_over_0": round(mean[4] / mean[0], 4), "one_paired_run": True}
    else:
        out["headline"] = "not measured"
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
