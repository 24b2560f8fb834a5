#!/usr/bin/env python3
"""The two FRI query phases on one GPU, in ONE process and on ONE context, behind the same commit phase; prints one JSON line and writes profiles/fri_index.json.
Shape: the headline proof - Fibonacci AIR, Goldilocks, 2^20 rows, blowup 8, 20 security bits, the configuration's own number of FRI queries.  One proof is made
(HostStark), which leaves the context behind its commit phase with the LDE committed; then, with the same betas,
  value   ms_fri_query            the reference's phase: leaves located by value, a quotient polynomial per (window, query); the MSFP blob stays in HBM
  value+  ms_fri_query, then ms_fri_proof_read: the same with the blob brought to the caller
  index   ms_fri_query_index      openings by position and the last round's polynomial; the MSFI blob arrives at the caller
are alternated `passes` times, `steps` calls per leg (every call ends in a stream synchronisation: host clock around it); then each phase once under
ms_profile_begin / ms_profile_end for its kernel milliseconds and launches (HIP events around every launch; taken apart from the timed legs), and one ms_tree_open
of 64 LDE rows, timed and profiled the same way.  Only the paired figures of one run mean anything.
  python3 tools/fri_index_bench.py [--log-rows 20] [--steps 10] [--passes 5] [--out profiles/fri_index.json]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def profile(ctx, fn):
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    fn()
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    prof = json.loads(buf.value.decode())
    classes = {k: v for k, v in prof.items() if isinstance(v, dict) and v.get("launches")}
    return {"kernel_ms": round(sum(v["ms"] for v in classes.values()), 4), "launches": sum(v["launches"] for v in classes.values()),
            "by_class": {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in classes.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10, help="calls per leg")
    ap.add_argument("--passes", type=int, default=5, help="legs per phase, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_index.json"))
    args = ap.parse_args()
    import mini_stark_amd as ms
    from common import SplitMix64
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    ctx = ms.Context(ms.GOLDILOCKS, flags=ms.FLAG_ZERO_DISPLAY_EMPTY)
    steps, blowup = (1 << args.log_rows) - 1, 8
    tt = fibonacci_air(ctx, steps)
    hs = HostStark(ctx, 20, blowup, steps, tt.constrain_number())
    ctx.check(hs.prove_raw(tt, read_fri_proof=False))          # the commit phase both query phases stand behind
    nq = hs.fri_queries
    rng = SplitMix64(0xF121)
    betas = [rng.next() for _ in range(nq)]
    rounds = 0
    while ctx.L.ms_fri_round_info(ctx.h, C.c_int(rounds), None, None) == 0:
        rounds += 1

    def value():
        rc, _ = ctx.fri_query(betas, read=False)
        ctx.check(rc)

    def value_read():
        rc, blob = ctx.fri_query(betas, read=True)
        ctx.check(rc)
        return blob
    legs = {"value": value, "value_with_readback": value_read, "index": lambda: ctx.fri_query_index(betas)}
    for fn in legs.values():                                   # every shape of the timed window, twice
        fn(); fn()
    per = {k: [] for k in legs}
    for _ in range(args.passes):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            per[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"metric": "fri_index_bench", "unit": "ms per call",
           "workload": f"Fibonacci AIR, Goldilocks, 2^{args.log_rows} rows, blowup {blowup}, 20 security bits, {rounds} FRI rounds, {nq} queries (the configuration's own); one context, "
                       f"both query phases behind the same commit phase, {args.steps} calls per leg, legs alternated x {args.passes}",
           "fri_queries": nq, "rounds": rounds, "one_paired_run": True, "phases": {}}
    sizes = {"value": len(value_read()), "value_with_readback": ctx.fri_proof_size(), "index": len(ctx.fri_query_index(betas))}
    for k, fn in legs.items():
        rec = {"ms_per_call": round(statistics.mean(per[k]), 4), "legs_ms": [round(x, 4) for x in per[k]], "blob_bytes": sizes[k]}
        if k != "value_with_readback":
            rec.update(profile(ctx, fn))
        out["phases"][k] = rec
    out["kernel_ms_index_over_value"] = round(out["phases"]["index"]["kernel_ms"] / out["phases"]["value"]["kernel_ms"], 6) if out["phases"]["value"]["kernel_ms"] > 0 else None
    out["ms_per_call_index_over_value"] = round(out["phases"]["index"]["ms_per_call"] / out["phases"]["value"]["ms_per_call"], 6)
    rows = [(rng.next() % (blowup << args.log_rows)) for _ in range(64)]
    opening = lambda: ctx.tree_open(ms.TREE_LDE, rows)         # noqa: E731
    opening(); opening()
    times = []
    for _ in range(20):
        t0 = time.perf_counter(); blob = opening(); times.append((time.perf_counter() - t0) * 1e3)
    rec = {"rows": 64, "ms_per_call_median": round(statistics.median(times), 4), "ms_per_call_min": round(min(times), 4), "bytes": len(blob)}
    rec.update(profile(ctx, opening))
    out["tree_open_lde"] = rec
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
