#!/usr/bin/env python3
"""The FRI commit phase as it is (ms_fri_begin .. ms_fri_fold_commit, arity 2 with a DEEP quotient per round) against the folded FRI (ms_fri_begin_folded ..
ms_fri_fold_final) at arity 2, 4 and 8, and their query phases by index (ms_fri_query_index, ms_fri_query_folded), on one GPU, in ONE process and on ONE context,
from the same validity polynomial; prints one JSON line and writes profiles/fri_folded.json.  It gates nothing: the comparison leg is today's commit phase in the same
process, not a fixed number.
Shape: the headline proof - Fibonacci AIR, Goldilocks, 2^20 rows, blowup 8.  One proof is made (HostStark), which leaves the context with its validity polynomial;
then the four commit phases are alternated `passes` times (host clock around a whole phase: every call of it ends in a host round trip), each once more under
ms_profile_begin / ms_profile_end for its kernel milliseconds and launches, and behind each the query phase at 2 and at 32 queries, `steps` calls per leg.
  python3 tools/fri_folded_bench.py [--log-rows 20] [--steps 10] [--passes 5] [--out profiles/fri_folded.json]"""
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
    ap.add_argument("--steps", type=int, default=10, help="query calls per leg")
    ap.add_argument("--passes", type=int, default=5, help="commit phases per leg, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_folded.json"))
    args = ap.parse_args()
    import mini_stark_amd as ms
    from common import MODULUS, SplitMix64
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    ctx = ms.Context(ms.GOLDILOCKS, flags=ms.FLAG_ZERO_DISPLAY_EMPTY)
    steps, blowup, p, e = (1 << args.log_rows) - 1, 8, MODULUS[0], 2
    tt = fibonacci_air(ctx, steps)
    hs = HostStark(ctx, 20, blowup, steps, tt.constrain_number())
    ctx.check(hs.prove_raw(tt, read_fri_proof=False))          # leaves the validity polynomial every commit phase below starts from
    rounds = 0
    while ctx.L.ms_fri_round_info(ctx.h, C.c_int(rounds), None, None) == 0:
        rounds += 1
    rng = SplitMix64(0xF01D)
    ch = [[rng.nonzero(p) for _ in range(e)] for _ in range(2 * rounds)]

    def legacy():
        rc, _ = ctx.fri_begin(blowup, rounds)
        ctx.check(rc)
        for i in range(1, rounds):
            ctx.check(ctx.fri_deep(ch[2 * i])[0])
            ctx.check(ctx.fri_fold_commit(ch[2 * i + 1])[0])
        return 1 + 2 * (rounds - 1)

    def folded(k):
        def run():
            rc, _ = ctx.fri_begin_folded(blowup, k)
            ctx.check(rc)
            D0 = ctx.fri_round_info(0)[1]
            R = ((D0 // blowup).bit_length() - 1) // k
            for i in range(R - 1):
                ctx.check(ctx.fri_fold_folded(ch[i])[0])
            ctx.check(ctx.fri_fold_final(ch[R - 1])[0])
            return R + 1
        return run
    legs = {"legacy": legacy, "folded_k1": folded(1), "folded_k2": folded(2), "folded_k3": folded(3)}
    calls = {}
    for name, fn in legs.items():                              # every shape of the timed window, twice
        fn(); calls[name] = fn()
    per = {name: [] for name in legs}
    for _ in range(args.passes):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            per[name].append((time.perf_counter() - t0) * 1e3)
    out = {"metric": "fri_folded_bench", "unit": "ms",
           "workload": f"Fibonacci AIR, Goldilocks, 2^{args.log_rows} rows, blowup {blowup}; one context, every commit phase from the same validity polynomial, phases alternated x "
                       f"{args.passes}; query legs of {args.steps} calls behind each commit phase",
           "legacy_rounds": rounds, "one_paired_run": True, "commit": {}, "query": {}}
    betas = {2: [rng.next() for _ in range(2)], 32: [rng.next() for _ in range(32)]}
    for name, fn in legs.items():
        rec = {"host_round_trips": calls[name], "ms_per_phase": round(statistics.mean(per[name]), 4), "phases_ms": [round(x, 4) for x in per[name]],
               "ms_per_call": round(statistics.mean(per[name]) / calls[name], 4)}
        rec.update(profile(ctx, fn))                           # (leaves the context behind this leg's commit phase: its query phase follows)
        if name != "legacy":
            rec["rounds"] = calls[name] - 1
        out["commit"][name] = rec
        query = (lambda b: ctx.fri_query_index(b)) if name == "legacy" else (lambda b: ctx.fri_query_folded(b))
        out["query"][name] = {}
        for nq, b in betas.items():
            query(b); query(b)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                blob = query(b)
            q = {"ms_per_call": round((time.perf_counter() - t0) / args.steps * 1e3, 4), "blob_bytes": len(blob)}
            q.update(profile(ctx, lambda: query(b)))
            out["query"][name]["nq%d" % nq] = q
    base = out["commit"]["legacy"]
    for name in ("folded_k1", "folded_k2", "folded_k3"):
        out["commit"][name]["ms_per_phase_over_legacy"] = round(out["commit"][name]["ms_per_phase"] / base["ms_per_phase"], 4)
        out["commit"][name]["kernel_ms_over_legacy"] = round(out["commit"][name]["kernel_ms"] / base["kernel_ms"], 4) if base["kernel_ms"] > 0 else None
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
