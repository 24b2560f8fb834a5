#!/usr/bin/env python3
"""The linked proof on one GPU, in ONE process; prints one JSON line and writes profiles/linked.json.
Shape: Goldilocks, 2^20 rows, blowup 8, 20 security bits, the Fibonacci AIR written as an ms_air program (three columns a, b, c: a' = b, b' = c, c = a + b, the two
boundary values), the configuration's own rounds and queries.
  (a) the query phase.  One linked proof is made (HostStark.prove_linked), which leaves the context behind its commit phase with the DEEP polynomial installed; then,
      with the same betas and caller-owned buffers,
        linked   ms_query_linked                                                    one launch, one job upload, one read-back, one synchronisation
        three    ms_fri_query_index, ms_tree_open(LDE), ms_tree_open(VALIDITY)      the calls it replaces
      are alternated `passes` times, `steps` calls per leg (host clock around the calls, which end synchronised); then each once under ms_profile_begin /
      ms_profile_end for launches and kernel milliseconds.
  (b) the proof.  msh_stark_prove_linked (the MSLP bytes at the caller) against msh_stark_prove with the MSFP blob left in HBM and with the blob read back, each on a
      context without and with MS_FLAG_LATENCY; legs alternated `passes` times, `proofs` proofs per leg; proof bytes of each.
Only the paired figures of one run mean anything.
  python3 tools/linked_bench.py [--log-rows 20] [--steps 20] [--proofs 3] [--passes 5] [--out profiles/linked.json] [--lib PATH]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fibonacci_program(p, N):
    """the benchmark's Fibonacci trace (steps = N - 1 rows and one padding row) as an ms_air program: (constraints, exempt, periodic, boundary)"""
    m1 = p - 1
    cons = [[(1, [(0, 1)]), (m1, [(1, 0)])],                       # a' = b
            [(1, [(1, 1)]), (m1, [(2, 0)])],                       # b' = c
            [(1, [(2, 0)]), (m1, [(0, 0)]), (m1, [(1, 0)])]]       # c = a + b
    return cons, [[N - 2, N - 1], [N - 2, N - 1], [N - 1]], (), [(0, 0, 1), (1, 0, 2)]


def profile(ctx, fn):
    buf = C.create_string_buffer(1 << 15)
    ctx.check(ctx.L.ms_profile_begin(ctx.h))
    fn()
    ctx.check(ctx.L.ms_profile_end(ctx.h, buf, C.c_size_t(len(buf))))
    prof = json.loads(buf.value.decode())
    classes = {k: v for k, v in prof.items() if isinstance(v, dict) and v.get("launches")}
    return {"kernel_ms": round(sum(v["ms"] for v in classes.values()), 4), "launches": sum(v["launches"] for v in classes.values()),
            "by_class": {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in classes.items()}}


def alternate(legs, passes, steps):
    for fn in legs.values():                                       # every shape of the timed window, twice
        fn(); fn()
    per = {k: [] for k in legs}
    for _ in range(passes):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            per[k].append((time.perf_counter() - t0) / steps * 1e3)
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20, help="query-phase calls per leg")
    ap.add_argument("--proofs", type=int, default=3, help="proofs per leg")
    ap.add_argument("--passes", type=int, default=5, help="legs per variant, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linked.json"))
    ap.add_argument("--lib", default=None, help="another libministark build (the emulation build: a dry run of the tool, its times mean nothing)")
    args = ap.parse_args()
    import numpy as np
    import mini_stark_amd as ms
    from common import MODULUS, SplitMix64
    from pyref_linked import link_rows
    from mini_stark_amd.host import HostStark, build_host_library
    from mini_stark_amd.stark import fibonacci_air
    build_host_library()
    N, blowup = 1 << args.log_rows, 8
    steps, L = N - 1, N * blowup
    air = ms.flatten_air(*fibonacci_program(MODULUS[ms.GOLDILOCKS], N))
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    lib = {"lib_path": args.lib} if args.lib else {}
    ctxs = {"default": ms.Context(ms.GOLDILOCKS, flags=ms.FLAG_ZERO_DISPLAY_EMPTY, **lib), "latency": ms.Context(ms.GOLDILOCKS, flags=ms.FLAG_ZERO_DISPLAY_EMPTY | ms.FLAG_LATENCY, **lib)}
    tt = fibonacci_air(ctxs["default"], steps)
    hss = {k: HostStark(c, 20, blowup, steps, 3) for k, c in ctxs.items()}
    out = {"metric": "linked_bench", "unit": "ms", "one_paired_run": True,
           "workload": f"Fibonacci AIR as an ms_air program, Goldilocks, 2^{args.log_rows} rows, blowup {blowup}, 20 security bits, {hss['default'].rounds} FRI rounds, "
                       f"{hss['default'].fri_queries} queries (the configuration's own); one process, legs alternated x {args.passes}"}
    # ---- (a) the query phase behind one commit phase
    ctx, hs = ctxs["default"], hss["default"]
    ctx.check(hs.prove_linked(tt.data, air))
    nq = hs.fri_queries
    rng = SplitMix64(0x11CED)
    betas = np.array([rng.next() for _ in range(nq)], dtype=np.uint64)
    D0 = ctx.fri_round_info(0)[1]
    rows = np.array(link_rows(betas.tolist(), D0, L), dtype=np.uint64)
    whole = ctx.query_linked(betas)
    parts = [ctx.fri_query_index(betas), ctx.tree_open(ms.TREE_LDE, rows), ctx.tree_open(ms.TREE_VALIDITY, rows)]
    assert whole[32:] == b"".join(parts), "ms_query_linked is not the three calls' bytes"
    bufs = [np.zeros(len(x) + 8, dtype=np.uint8) for x in [whole] + parts]
    n = C.c_size_t(0)
    bp, rp = betas.ctypes.data_as(u64p), rows.ctypes.data_as(u64p)

    def linked():
        ctx.check(ctx.L.ms_query_linked(ctx.h, bp, C.c_int(nq), bufs[0].ctypes.data_as(u8p), C.c_size_t(bufs[0].size), C.byref(n)))

    def three():
        ctx.check(ctx.L.ms_fri_query_index(ctx.h, bp, C.c_int(nq), bufs[1].ctypes.data_as(u8p), C.c_size_t(bufs[1].size), C.byref(n)))
        ctx.check(ctx.L.ms_tree_open(ctx.h, C.c_int(ms.TREE_LDE), C.c_int(0), rp, C.c_size_t(rows.size), bufs[2].ctypes.data_as(u8p), C.c_size_t(bufs[2].size), C.byref(n)))
        ctx.check(ctx.L.ms_tree_open(ctx.h, C.c_int(ms.TREE_VALIDITY), C.c_int(0), rp, C.c_size_t(rows.size), bufs[3].ctypes.data_as(u8p), C.c_size_t(bufs[3].size), C.byref(n)))
    legs = {"linked": linked, "three_calls": three}
    per = alternate(legs, args.passes, args.steps)
    out["query_phase"] = {"calls_per_leg": args.steps, "bytes": {"linked": len(whole), "three_calls": sum(len(x) for x in parts)}}
    for k, fn in legs.items():
        rec = {"ms_per_call": round(statistics.mean(per[k]), 4), "legs_ms": [round(x, 4) for x in per[k]]}
        rec.update(profile(ctx, fn))
        out["query_phase"][k] = rec
    out["query_phase"]["ms_saved_per_query_phase"] = round(out["query_phase"]["three_calls"]["ms_per_call"] - out["query_phase"]["linked"]["ms_per_call"], 4)
    # ---- (b) the proof
    legs, sizes = {}, {}
    for k, c in ctxs.items():
        h = hss[k]
        legs[f"linked/{k}"] = lambda h=h, c=c: (c.check(h.prove_linked(tt.data, air)), h.linked_proof())
        legs[f"unlinked_blob_in_hbm/{k}"] = lambda h=h, c=c: c.check(h.prove_raw(tt, read_fri_proof=False))
        legs[f"unlinked_blob_read_back/{k}"] = lambda h=h, c=c: c.check(h.prove_raw(tt, read_fri_proof=True))
    per = alternate(legs, args.passes, args.proofs)
    hs.prove_linked(tt.data, air)
    sizes["linked"] = len(hs.linked_proof())
    hs.prove_raw(tt, read_fri_proof=True)
    sizes["unlinked"] = len(hs.proof_bytes())
    out["proof"] = {"proofs_per_leg": args.proofs, "proof_bytes": sizes,
                    "legs": {k: {"ms_per_proof": round(statistics.mean(v), 4), "legs_ms": [round(x, 4) for x in v]} for k, v in per.items()}}
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
