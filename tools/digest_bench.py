#!/usr/bin/env python3
"""SHA-256 against BLAKE2s-256 (MS_FLAG_DIGEST_BLAKE2S), BLAKE3 (MS_FLAG_DIGEST_BLAKE3), Keccak-256 (MS_FLAG_DIGEST_KECCAK256) and SHA3-256
(MS_FLAG_DIGEST_SHA3_256) on the headline shape, in ONE process on one GPU: 2^20-row Goldilocks Fibonacci AIR, blowup 8, traces resident in HBM, 8 proofs in
flight (bench.py's Lanes), the legs alternated SHA-256 / BLAKE2s / BLAKE3 / Keccak-256 / SHA3-256 / SHA-256 / ... -
box-to-box spread is larger than the differences may be, so only the paired rates of one run mean anything.  Then one proof alone with MS_FLAG_LATENCY for each digest, and one more
(untimed) proof per digest with every launch bracketed by HIP events (ms_profile_begin / ms_profile_end): kernel milliseconds per proof by class.
Prints one JSON line.
  python3 tools/digest_bench.py [--steps 30] [--warmup 4] [--passes 2] [--log-rows 20]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class OneRank:   # the part of bench.py's process group that Lanes.timed uses
    def barrier(self):
        pass

    def max_over_ranks(self, v):
        return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--passes", type=int, default=2, help="legs per digest (alternated)")
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--blowup", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=8)
    args = ap.parse_args()
    if args.steps < 30 and args.log_rows == 20:
        ap.error("at least 30 steps per leg on the headline shape")
    import torch
    import bench
    import mini_stark_amd as ms
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = {"sha256": ms.FLAG_ZERO_DISPLAY_EMPTY, "blake2s": ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_DIGEST_BLAKE2S, "blake3": ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_DIGEST_BLAKE3,
             "keccak256": ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_DIGEST_KECCAK256, "sha3_256": ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_DIGEST_SHA3_256}
    ids = {"sha256": ms.DIGEST_SHA256, "blake2s": ms.DIGEST_BLAKE2S256, "blake3": ms.DIGEST_BLAKE3, "keccak256": ms.DIGEST_KECCAK256, "sha3_256": ms.DIGEST_SHA3_256}
    grp = OneRank()
    lanes = {k: bench.Lanes(0, args.log_rows, args.blowup, args.inflight, 0, dev, flags=f) for k, f in names.items()}
    for k, ln in lanes.items():
        assert ln.ctxs[0].digest == ids[k]
    rates = {k: [] for k in names}
    for p in range(args.passes):
        for k in names:
            el = lanes[k].timed(grp, args.steps, args.warmup if p == 0 else 1)
            rates[k].append(args.steps * args.inflight / el)
    for ln in lanes.values():
        ln.close()
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    # one proof alone, latency mode; then the per-kernel profile of one more proof on the same context
    single, kernel_ms = {}, {}
    for k, f in names.items():
        ln = bench.Lanes(0, args.log_rows, args.blowup, 1, 0, dev, flags=f | ms.FLAG_LATENCY)
        ln._prove_n(0, 3)
        t0 = time.perf_counter(); ln._prove_n(0, 10); single[k] = (time.perf_counter() - t0) / 10 * 1e3
        ctx = ln.ctxs[0]
        buf = C.create_string_buffer(1 << 15)
        ctx.check(ctx.L.ms_profile_begin(ctx.h))
        ln._prove_n(0, 1)
        ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
        prof = json.loads(buf.value.decode())
        kernel_ms[k] = {n: round(v["ms"], 4) for n, v in prof.items() if isinstance(v, dict) and "ms" in v and v.get("launches")}
        kernel_ms[k]["launches"] = sum(v["launches"] for v in prof.values() if isinstance(v, dict) and "launches" in v)
        kernel_ms[k]["total"] = round(sum(v for n, v in kernel_ms[k].items() if n != "launches"), 4)
        ln.close()
    print(json.dumps({"metric": "digest_bench", "workload": f"Fibonacci AIR, Goldilocks, 2^{args.log_rows} rows, blowup {args.blowup}, traces resident, {args.inflight} proofs in flight, "
                      f"{args.steps} steps per leg, legs alternated sha256 / blake2s / blake3 / keccak256 / sha3_256 x {args.passes}", "unit": "proofs/s",
                      "sha256": mean["sha256"], "blake2s": mean["blake2s"], "blake3": mean["blake3"], "keccak256": mean["keccak256"], "sha3_256": mean["sha3_256"],
                      "ratio_keccak256_over_sha256": mean["keccak256"] / mean["sha256"], "ratio_sha3_256_over_sha256": mean["sha3_256"] / mean["sha256"],
                      "single_proof_ratio_keccak256_over_sha256": single["keccak256"] / single["sha256"], "ratio_blake2s_over_sha256": mean["blake2s"] / mean["sha256"],
                      "ratio_blake3_over_sha256": mean["blake3"] / mean["sha256"], "ratio_blake3_over_blake2s": mean["blake3"] / mean["blake2s"], "passes": rates,
                      "ms_single_proof_latency_flag": single, "single_proof_ratio_sha256_over_blake2s": single["sha256"] / single["blake2s"],
                      "single_proof_ratio_sha256_over_blake3": single["sha256"] / single["blake3"], "single_proof_ratio_blake2s_over_blake3": single["blake2s"] / single["blake3"],
                      "kernel_ms_per_proof": kernel_ms, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
