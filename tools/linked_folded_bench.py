#!/usr/bin/env python3
"""A v1 linked proof against v3 linked proofs (folded FRI over coset-grouped row trees) on one GPU, in ONE process and ONE context; prints one JSON line and writes
profiles/linked_folded.json.  It gates nothing.
Shape: Goldilocks, 2^20 rows, blowup 8, 20 security bits, SIX trace columns - the Fibonacci AIR of tools/linked_bench.py twice, on the columns 0..2 and 3..5, as one
ms_air program -, the configuration's own queries; v1 with the configuration's own rounds, v3 at log_arity k = 1, 2, 3 with floor(log2 N / k) folds.
Legs: msh_stark_prove_linked and msh_stark_prove_linked_folded at k = 1, 2, 3, the MSLP bytes at the caller, alternated `passes` times, `proofs` proofs per leg (host
clock around the calls, which end synchronised).  Then each once under ms_profile_begin / ms_profile_end: kernel milliseconds split by launch name, and the launch
count.  Proof bytes at the configuration's queries, and at 32 queries (the proof's bytes with its query blob replaced by the blob for 32 betas).
The comparison is v1 in the same paired run: neither an absolute time nor any figure derived elsewhere counts.
  python3 tools/linked_folded_bench.py [--log-rows 20] [--proofs 3] [--passes 5] [--out profiles/linked_folded.json] [--lib PATH]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def six_column_program(p, N):
    """tools/linked_bench.py's Fibonacci program on the columns 0..2 and again on 3..5: (constraints, exempt, periodic, boundary)"""
    from linked_bench import fibonacci_program
    cons, exempt, periodic, boundary = fibonacci_program(p, N)
    shift = lambda t: [(coef, [(col + 3, row) for col, row in facs]) for coef, facs in t]   # noqa: E731
    return cons + [shift(t) for t in cons], exempt + exempt, periodic, boundary + [(col + 3, row, v) for col, row, v in boundary]


def profile(ctx, fn):
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    fn()
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    prof = json.loads(buf.value.decode())
    classes = {k: v for k, v in prof.items() if isinstance(v, dict) and v.get("launches")}
    return {"kernel_ms": round(sum(v["ms"] for v in classes.values()), 4), "launches": sum(v["launches"] for v in classes.values()),
            "by_launch_name": {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in classes.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--proofs", type=int, default=3, help="proofs per leg")
    ap.add_argument("--passes", type=int, default=5, help="legs per variant, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linked_folded.json"))
    ap.add_argument("--lib", default=None, help="another libministark build (the emulation build: a dry run of the tool, its times mean nothing)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import mini_stark_amd as ms
    from common import MODULUS, SplitMix64
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    N, blowup = 1 << args.log_rows, 8
    steps = N - 1
    air = ms.flatten_air(*six_column_program(MODULUS[ms.GOLDILOCKS], N))
    lib = {"lib_path": args.lib} if args.lib else {}
    ctx = ms.Context(ms.GOLDILOCKS, flags=ms.FLAG_ZERO_DISPLAY_EMPTY, **lib)
    one = fibonacci_air(ctx, steps).data
    trace = np.ascontiguousarray(np.hstack([one, one]), dtype=np.uint64)
    hs = HostStark(ctx, 20, blowup, steps, 6)
    nq = hs.fri_queries
    legs = {"v1": lambda: (ctx.check(hs.prove_linked(trace, air)), hs.linked_proof())[1]}
    for k in (1, 2, 3):
        legs["v3/k=%d" % k] = lambda k=k: (ctx.check(hs.prove_linked_folded(trace, air, k)), hs.linked_proof())[1]
    for fn in legs.values():                                       # every shape of the timed window, twice
        fn(); fn()
    per = {name: [] for name in legs}
    for _ in range(args.passes):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(args.proofs):
                fn()
            per[name].append((time.perf_counter() - t0) / args.proofs * 1e3)
    rng = SplitMix64(0x11CED)
    betas32 = np.array([rng.next() for _ in range(32)], dtype=np.uint64)
    out = {"metric": "linked_folded_bench", "unit": "ms", "one_paired_run": True, "gates": None,
           "workload": f"two Fibonacci AIRs side by side as one ms_air program (6 trace columns), Goldilocks, 2^{args.log_rows} rows, blowup {blowup}, 20 security bits, {nq} queries "
                       f"(the configuration's own); v1: {hs.rounds} FRI rounds; v3: floor(log2 N / k) folds; one process, one context, legs alternated x {args.passes}",
           "proofs_per_leg": args.proofs, "legs": {}}
    for name, fn in legs.items():
        proof = fn()                                               # (leaves the context behind this leg's commit phase: the query blobs below are this proof's)
        own = ctx.query_linked(betas32[:nq]) if name == "v1" else ctx.query_linked_folded(betas32[:nq])
        at32 = ctx.query_linked(betas32) if name == "v1" else ctx.query_linked_folded(betas32)
        rec = {"ms_per_proof": round(statistics.mean(per[name]), 4), "legs_ms": [round(x, 4) for x in per[name]],
               "proof_bytes": {"at_%d_queries" % nq: len(proof), "at_32_queries": len(proof) - len(own) + len(at32)}}
        rec.update(profile(ctx, fn))
        out["legs"][name] = rec
    v1 = out["legs"]["v1"]["ms_per_proof"]
    out["v3_over_v1"] = {name: round(rec["ms_per_proof"] / v1, 4) for name, rec in out["legs"].items() if name != "v1"}
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
